#!/usr/bin/env python
"""Gaussians seeded from a point cloud on the MI355X: the reference's PcdInitializer and GaussianSkyInitializer
(gaustudio/pipelines/initializers/pcd.py, gaussiansky.py), both of which end in VanillaPointCloud.create_from_attribute with
scales from the 3-nearest-neighbour distance (simple-knn's distCUDA2 in the reference).

    sampled coloured sphere (points, colours, outward normals) -> pcd_init      \\
                                                                                 > seeds.ply -> GaussianRasterizer
    Fibonacci sky shell around it                                 -> sky_seeds  /

    python examples/pcd_init_synthetic.py [out_dir] [--points 200000] [--sky-resolution 60] [--sky-radius 20]

Writes <out>/seeds.ply (the Gaussian PLY a trainer starts from; the object's seeds first, then the sky's) and
<out>/seeds_000.ppm (the seeds rendered once from outside the object, the white sky shell behind it).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, formats, scenes  # noqa: E402
from gaustudio_amd import pcd_init as pi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="pcd_init_out")
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--sky-resolution", type=int, default=60)
    ap.add_argument("--sky-radius", type=float, default=20.0)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    d = rng.normal(size=(args.points, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    points = torch.from_numpy(d.astype(np.float32)).to(dev)
    obj = pi.pcd_init(points, colors=points * 0.5 + 0.5, normals=points.clone())
    sky = pi.sky_seeds(args.sky_resolution, args.sky_radius, device=dev)
    cloud = formats.GaussianCloud(*(torch.cat([getattr(obj, k), getattr(sky, k)]) for k in ("xyz", "f_dc", "f_rest", "opacity", "scale", "rot")))
    path = os.path.join(args.out, "seeds.ply")
    formats.export_gaussian_ply(path, cloud)
    back = formats.load_gaussian_ply(path)
    assert back.num_points == cloud.num_points and torch.equal(back.scale, cloud.scale.cpu())

    cam = scenes.look_at_camera(480, 360, [0.0, -0.6, -2.6], [0.0, 0.0, 0.0])
    rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0, cam.viewmatrix.to(dev),
                                       cam.projmatrix.to(dev), 3, cam.campos.to(dev), False, False)
    act = cloud.activated()
    with torch.no_grad():
        color, _, _, _, opacity = GaussianRasterizer(rs)(means3D=act["means3D"], means2D=torch.zeros_like(act["means3D"]),
                                                          opacities=act["opacities"], shs=act["shs"], scales=act["scales"],
                                                          rotations=act["rotations"])
    rgb = (color.clamp(0, 1).permute(1, 2, 0) * 255 + 0.5).to(torch.uint8).cpu().numpy()
    with open(os.path.join(args.out, "seeds_000.ppm"), "wb") as fh:
        fh.write(f"P6 {rgb.shape[1]} {rgb.shape[0]} 255\n".encode())
        fh.write(rgb.tobytes())
    s = obj.scale[:, 0].exp()
    print(f"{obj.num_points} object seeds (scale median {float(s.median()):.4g}) + {sky.num_points} sky seeds; rendered: "
          f"{float((opacity > 0.05).float().mean()) * 100:.1f} % of the pixels touched; wrote {path} ({back.num_points} Gaussians "
          f"read back) and seeds_000.ppm")


if __name__ == "__main__":
    main()
