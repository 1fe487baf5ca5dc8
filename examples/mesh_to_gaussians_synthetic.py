#!/usr/bin/env python
"""The way back from a coloured triangle mesh to Gaussians on the MI355X: the reference's VoxelInitializer
(gaustudio/pipelines/initializers/mesh.py:252-442, what `gs-init` / `mesh2gs` run with the 'voxel' initializer).

    coloured mesh -> normalise to the unit cube -> voxelize (float64 triangle / box test) -> one Gaussian per occupied voxel,
                     coloured from the closest point of the mesh -> seeds.ply -> GaussianRasterizer

    python examples/mesh_to_gaussians_synthetic.py [out_dir] [--mesh sphere|fused_mesh.ply] [--voxel-size 0.0078125]

--mesh sphere (default): a built-in icosphere of 20 480 triangles coloured by position.  --mesh <path>: a coloured PLY, for
instance the fused_mesh.ply that `examples/extract_mesh_synthetic.py --fusion rgbd` writes.  Mesh, voxels and seeds never leave
the GPU.  Writes <out>/seeds.ply (the Gaussian PLY a trainer starts from) and <out>/seeds_000.ppm (the seeds rendered once).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, formats, scenes, voxel_init  # noqa: E402


def colored_sphere(subdivisions=5):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.array(v)
    return v.astype(np.float32), np.array(f, dtype=np.int32), (v * 0.5 + 0.5).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="mesh_to_gaussians_out")
    ap.add_argument("--mesh", default="sphere")
    ap.add_argument("--voxel-size", type=float, default=1 / 128)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    dev = torch.device("cuda:0")
    if args.mesh == "sphere":
        v, f, col = (torch.from_numpy(a).to(dev) for a in colored_sphere())
    else:
        v, f, attrs = formats.read_ply_mesh(args.mesh, return_attributes=True)
        col = attrs.get("colors")
        to = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, dt)
        if col is not None:                      # uchar red green blue, or floats in [0, 1]
            is_u8 = (col.dtype == torch.uint8) if torch.is_tensor(col) else (col.dtype == np.uint8)
            col = to(col, torch.float32) / 255.0 if is_u8 else to(col, torch.float32)
        v, f = to(v, torch.float32), to(f, torch.int32)
    grid, cloud = voxel_init(v, f, col, voxel_size=args.voxel_size, generator=torch.Generator(device=dev).manual_seed(0))
    formats.export_gaussian_ply(os.path.join(args.out, "seeds.ply"), cloud)
    # the seeds seen from outside the mesh's bounding sphere
    centre = (v.min(dim=0).values + v.max(dim=0).values) / 2
    radius = float((v - centre).norm(dim=1).max())
    eye = (centre + torch.tensor([0.0, -0.6, -2.6], device=dev) * radius).tolist()
    cam = scenes.look_at_camera(480, 360, eye, centre.tolist())
    rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0, cam.viewmatrix.to(dev),
                                       cam.projmatrix.to(dev), 3, cam.campos.to(dev), False, False)
    act = cloud.activated()                      # the raw opacity is +inf (the reference's inverse_sigmoid(1)): its sigmoid is 1
    with torch.no_grad():
        color, _, _, _, opacity = GaussianRasterizer(rs)(means3D=act["means3D"], means2D=torch.zeros_like(act["means3D"]),
                                                          opacities=act["opacities"], shs=act["shs"], scales=act["scales"],
                                                          rotations=act["rotations"])
    rgb = (color.clamp(0, 1).permute(1, 2, 0) * 255 + 0.5).to(torch.uint8).cpu().numpy()
    with open(os.path.join(args.out, "seeds_000.ppm"), "wb") as fh:
        fh.write(f"P6 {rgb.shape[1]} {rgb.shape[0]} 255\n".encode())
        fh.write(rgb.tobytes())
    print(f"{v.shape[0]} vertices / {f.shape[0]} triangles -> {grid.num_voxels} of {grid.shape[0]}^3 voxels, "
          f"{int(grid.pair_tri.shape[0])} (voxel, triangle) pairs, {cloud.num_points} seeds; rendered: "
          f"{float((opacity > 0.5).float().mean()) * 100:.1f} % of the pixels covered; wrote {args.out}/seeds.ply and seeds_000.ppm")


if __name__ == "__main__":
    main()
