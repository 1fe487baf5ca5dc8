#!/usr/bin/env python
"""Gaussians -> mesh -> coloured mesh -> Gaussians without leaving the MI355X: gs-extract-mesh, gs-texture-mesh
(gaustudio/scripts/texture_mesh.py) and the reference's default mesh initializer (MeshInitializer, mesh.py:74-250) in a row.

    GaussianRasterizer (RGB, median depth) -> TSDFVolume (depth only) -> mesh_clean -> TextureBaker (the rendered RGB of every
    view baked into vertex colours, later views overwriting) -> textured_mesh.ply -> mesh_seeds (one flat Gaussian per
    triangle) -> seeds.ply -> GaussianRasterizer

    python examples/texture_mesh_synthetic.py [out_dir] [--sampling reference|exact] [--views 24] [--n-per-triangle 1]

Runs on a synthetic shell of Gaussians coloured by position, so it needs no dataset.  out_dir defaults to texture_mesh_out in
the system's temporary directory.  Writes <out>/textured_mesh.ply (the mesh with uchar vertex colours), <out>/seeds.ply (the
Gaussian PLY a trainer starts from) and <out>/seeds_000.ppm (the seeds rendered into the first camera).
"""
import argparse
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, formats, mesh_clean, postprocess as pp, scenes  # noqa: E402
from gaustudio_amd.mesh_init import mesh_seeds  # noqa: E402
from gaustudio_amd.texture_bake import TextureBaker  # noqa: E402
from gaustudio_amd.tsdf import TSDFVolume  # noqa: E402

C0 = 0.28209479177387814


def shell(P=200_000):
    """A bumpy unit shell of small opaque Gaussians whose colour is their direction."""
    g = torch.Generator().manual_seed(0)
    d = torch.randn(P, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    xyz = d * (1.0 + 0.08 * torch.sin(5 * d[:, 0:1]) * torch.cos(4 * d[:, 1:2]))
    rgb = d * 0.4 + 0.5
    return formats.GaussianCloud(xyz=xyz, f_dc=((rgb - 0.5) / C0).reshape(P, 1, 3), f_rest=torch.zeros(P, 15, 3),
                                 opacity=torch.full((P, 1), 3.0), scale=torch.full((P, 3), math.log(0.008)),
                                 rot=torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1))


def render(cam, act, dev, sh_degree=0):
    rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0, cam.viewmatrix.to(dev),
                                       cam.projmatrix.to(dev), sh_degree, cam.campos.to(dev), False, False)
    with torch.no_grad():
        color, _, _, median, opacity = GaussianRasterizer(rs)(means3D=act["means3D"], means2D=torch.zeros_like(act["means3D"]),
                                                               opacities=act["opacities"], shs=act["shs"], scales=act["scales"],
                                                               rotations=act["rotations"])
    return color, median, opacity


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(tempfile.gettempdir(), "texture_mesh_out"))
    ap.add_argument("--sampling", default="reference", choices=("reference", "exact"))
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--n-per-triangle", type=int, default=1, choices=(1, 3, 4, 6))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    dev = torch.device("cuda:0")
    act = shell().to(dev).activated()
    cams = scenes.ring_cameras(args.views, 640, 480, radius=3.2, elevation=0.35) + \
        scenes.ring_cameras(max(args.views // 2, 1), 640, 480, radius=3.2, elevation=-0.8)

    # gs-extract-mesh: median depth -> depth-only TSDF -> mesh -> clean; the rendered RGB is kept for the bake
    volume = TSDFVolume(voxel_size=0.01, sdf_trunc=0.04, space_carving=False, capacity_blocks=1 << 18)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    views = []
    for cam in cams:
        color, median, opacity = render(cam, act, dev)
        depth = median[0].clone()
        depth[opacity[0] < 0.5] = 0
        f = cam.width / (2 * cam.tanfovx)
        K = torch.tensor([[f, 0, cam.width / 2], [0, f, cam.height / 2], [0, 0, 1]])
        E = cam.viewmatrix.t().contiguous()                                  # world-to-camera, OpenCV axes
        volume.integrate(pp.depth_to_points(depth, K, E, "world"), cam.campos)
        views.append((color.clamp(0, 1).permute(1, 2, 0).contiguous(), K, E))
    vertices, faces = volume.extract_triangle_mesh_device(min_weight=5)
    vertices, faces, _ = mesh_clean.remove_small_components(vertices, faces, ratio_threshold=0.5)
    torch.cuda.synchronize()
    t1 = time.perf_counter()

    # gs-texture-mesh
    baker = TextureBaker(vertices, faces, sampling=args.sampling)
    stats = [baker.add_view(image, K, E) for image, K, E in views]
    colors, baked_by = baker.vertex_colors, baker.baked_by
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    formats.write_ply_mesh(os.path.join(args.out, "textured_mesh.ply"), vertices, faces, vertex_colors=colors)

    # the mesh initializer, and the seeds seen from the first camera
    cloud = mesh_seeds(vertices, faces, vertex_colors=colors, n_per_triangle=args.n_per_triangle)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    formats.export_gaussian_ply(os.path.join(args.out, "seeds.ply"), cloud)
    color, _, opacity = render(cams[0], cloud.activated(), dev, sh_degree=3)   # raw opacity +inf: its sigmoid is 1
    rgb = (color.clamp(0, 1).permute(1, 2, 0) * 255 + 0.5).to(torch.uint8).cpu().numpy()
    with open(os.path.join(args.out, "seeds_000.ppm"), "wb") as fh:
        fh.write(f"P6 {rgb.shape[1]} {rgb.shape[0]} 255\n".encode())
        fh.write(rgb.tobytes())
    want = (vertices / vertices.norm(dim=1, keepdim=True)) * 0.4 + 0.5           # the shell's colour at the vertex's direction
    done = baked_by >= 0
    err = float((colors[done] - want[done]).abs().mean()) if bool(done.any()) else float("nan")
    seen = views[0][0]
    both = opacity[0] > 0.5
    rerr = float((color.clamp(0, 1).permute(1, 2, 0)[both] - seen[both]).abs().mean()) if bool(both.any()) else float("nan")
    print(f"{len(cams)} views rendered, fused, meshed and cleaned in {(t1 - t0) * 1e3:.0f} ms: {vertices.shape[0]} vertices, "
          f"{faces.shape[0]} triangles; baked ({args.sampling}) in {(t2 - t1) * 1e3:.0f} ms: {int(done.sum())} vertices coloured, "
          f"{sum(s.selected_faces for s in stats)} face selections, mean |colour - shell colour| = {err:.3f}; "
          f"{cloud.num_points} seeds in {(t3 - t2) * 1e3:.1f} ms, rendered into view 0: mean |seeds - Gaussians| = {rerr:.3f} over "
          f"{int(both.sum())} pixels; wrote {args.out}/textured_mesh.ply, seeds.ply and seeds_000.ppm")


if __name__ == "__main__":
    main()
