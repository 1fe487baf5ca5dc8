#!/usr/bin/env python
"""The VisualHull initializer on the MI355X, end to end on a synthetic object: render a ball of Gaussians (scenes.py) from two
camera rings, threshold final_opacity > 0.5 into silhouette masks, carve the voxel grid against them, mesh the hull, seed one
Gaussian per mesh vertex, and render the hull back through the mesh rasterizer -- masks, grid and mesh never leave the GPU.

    python examples/visual_hull_synthetic.py [out_dir] [--resolution 128]

Writes <out>/visual_hull.ply (the mesh), <out>/seeds.ply (the Gaussian PLY a trainer starts from) and <out>/hull_000.ppm
(the hull's silhouette in the first view, next to <out>/mask_000.ppm, the mask it was carved from).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, formats, scenes, visual_hull_init  # noqa: E402
from gaustudio_amd.mesh_raster import MeshRasterizer  # noqa: E402


def write_ppm(path, grey):
    rgb = np.repeat(np.clip(grey, 0, 255).astype(np.uint8)[..., None], 3, -1)
    with open(path, "wb") as fh:
        fh.write(f"P6 {rgb.shape[1]} {rgb.shape[0]} 255\n".encode())
        fh.write(rgb.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="visual_hull_out")
    ap.add_argument("--resolution", type=int, default=128)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    dev = torch.device("cuda:0")
    sc = scenes.make_ball_scene(60_000, radius=1.0, seed=0, sigma=0.03)
    leaves = {k: getattr(sc, k).to(dev) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
    cams = scenes.ring_cameras(16, 320, 240, radius=3.5, elevation=0.35) + scenes.ring_cameras(8, 320, 240, radius=3.5, elevation=-0.9)
    masks = []
    with torch.no_grad():
        for cam in cams:
            rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0,
                                               cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 3, cam.campos.to(dev), False, False)
            out = GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=torch.zeros_like(leaves["means3D"]),
                                         opacities=leaves["opacities"], shs=leaves["shs"], scales=leaves["scales"],
                                         rotations=leaves["rotations"])
            masks.append(out[4][0] > 0.5)                                       # final_opacity -> bool [H,W]
    cameras = [(cam.projmatrix, cam.width, cam.height) for cam in cams]       # full_proj_transform triples
    hull, (vertices, faces), cloud = visual_hull_init(cameras, masks, resolution=args.resolution, translate=np.zeros(3), radius=1.5)
    formats.write_ply_mesh(os.path.join(args.out, "visual_hull.ply"), vertices, faces)
    formats.export_gaussian_ply(os.path.join(args.out, "seeds.ply"), cloud)
    # the hull seen from the first camera again
    cam = cams[0]
    f = cam.width / (2 * cam.tanfovx)
    K = torch.tensor([[f, 0, cam.width / 2], [0, f, cam.height / 2], [0, 0, 1]])
    frags = MeshRasterizer(vertices, faces).rasterize(K, cam.viewmatrix.t().contiguous(), cam.height, cam.width)
    sil = frags.pix_to_face >= 0
    write_ppm(os.path.join(args.out, "hull_000.ppm"), sil.cpu().numpy() * 255)
    write_ppm(os.path.join(args.out, "mask_000.ppm"), masks[0].cpu().numpy() * 255)
    inter, union = int((sil & masks[0]).sum()), int((sil | masks[0]).sum())
    print(f"{len(cams)} masks -> {hull.count} of {args.resolution}^3 voxels filled, {vertices.shape[0]} vertices / {faces.shape[0]} "
          f"triangles, {cloud.num_points} seeds; hull silhouette vs mask of view 0: IoU {inter / max(union, 1):.3f}; "
          f"wrote {args.out}/visual_hull.ply and {args.out}/seeds.ply")


if __name__ == "__main__":
    main()
