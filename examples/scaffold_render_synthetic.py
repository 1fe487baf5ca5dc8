#!/usr/bin/env python
"""Scaffold-GS inference end to end on the MI355X, on a synthetic scene (no dataset, no checkpoint):

    anchors on a sphere + random small MLPs  ->  scaffold.render_scaffold (visible filter, MLP decode, GaussianRasterizer)
                                             ->  median depth  ->  depth_to_points  ->  TSDFVolume  ->  mesh PLY

It shows that the anchor-based family enters the same extraction path as the other two: the fused median depth of the
Scaffold render is what TSDFVolume.integrate takes.   python examples/scaffold_render_synthetic.py [out_dir]
Writes render_000.npy (uint8 [H,W,3] of the first view) and scaffold_mesh.ply."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import GaussianRasterizationSettings, ScaffoldModel, formats, postprocess as pp, render_scaffold, scenes  # noqa: E402
from gaustudio_amd.tsdf import TSDFVolume  # noqa: E402


def synthetic_model(n, k, dev):
    g = torch.Generator().manual_seed(0)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev)
    d = torch.nn.functional.normalize(r(n, 3))
    anchor = d * (1.0 + 0.08 * torch.sin(5 * d[:, 0:1]) * torch.cos(4 * d[:, 1:2]))
    lin = lambda n_in, n_out, bias=0.0: (r(32, n_in, scale=0.2), r(32, scale=0.1), r(n_out, 32, scale=0.2), r(n_out, scale=0.1) + bias)
    scaling = torch.cat([torch.full((n, 3), 0.02), torch.full((n, 3), 0.012)], dim=1).to(dev)     # offsets: 2 cm; covariance: < 1.2 cm
    return ScaffoldModel(anchor, r(n, 32), r(n, k, 3), scaling, torch.tensor([[1.0, 0, 0, 0]], device=dev).repeat(n, 1),
                         lin(36, k, bias=1.5), lin(36, 7 * k), lin(36, 3 * k), lin(4, 3))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "scaffold_render_out"
    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda:0")
    model = synthetic_model(60_000, 10, dev)
    cams = scenes.ring_cameras(16, 480, 360, radius=3.2, elevation=0.35) + scenes.ring_cameras(8, 480, 360, radius=3.2, elevation=-0.8)
    volume = TSDFVolume(voxel_size=0.01, sdf_trunc=0.04, space_carving=False, capacity_blocks=1 << 18)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = []
    for i, cam in enumerate(cams):
        rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0,
                                           cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 1, cam.campos.to(dev), False, False)
        with torch.no_grad():
            res = render_scaffold(model, rs)
        g = res["gaussians"]
        stats.append((int(g.visible.sum()), g.xyz.shape[0]))
        depth = res["median_depth"][0].clone()
        depth[res["opacity"][0] < 0.5] = 0
        f = cam.width / (2 * cam.tanfovx)
        K = torch.tensor([[f, 0, cam.width / 2], [0, f, cam.height / 2], [0, 0, 1]])
        volume.integrate(pp.depth_to_points(depth, K, cam.viewmatrix.t().contiguous(), "world"), cam.campos)
        if i == 0:
            img = (res["render"].clamp(0, 1).permute(1, 2, 0) * 255 + 0.5).to(torch.uint8).cpu().numpy()
            np.save(os.path.join(out, "render_000.npy"), img)
    vertices, faces = volume.extract_triangle_mesh_device(min_weight=3)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    formats.write_ply_mesh(os.path.join(out, "scaffold_mesh.ply"), vertices, faces)
    rad = vertices.norm(dim=1)
    vis, m = np.mean([s[0] for s in stats]), np.mean([s[1] for s in stats])
    print(f"{len(cams)} views decoded, rendered, fused and meshed in {dt * 1e3:.0f} ms: per view {vis:.0f} of {model.num_anchors} anchors "
          f"visible, {m:.0f} Gaussians; mesh with {vertices.shape[0]} vertices, {faces.shape[0]} triangles, radius "
          f"{float(rad.min()):.3f} .. {float(rad.max()):.3f} (anchors at 0.92 .. 1.08); first view: mean RGB {img.mean():.1f} / 255")
    assert faces.shape[0] > 1000, "the extraction path produced no surface"


if __name__ == "__main__":
    main()
