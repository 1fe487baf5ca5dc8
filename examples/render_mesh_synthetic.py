#!/usr/bin/env python
"""The extract-then-render loop on the MI355X: the gs-extract-mesh steps (render Gaussians -> median depth -> TSDF ->
marching cubes), then what gaustudio/scripts/render_mesh.py does with the mesh (depth, mask and camera-space normal maps
from each camera) -- with the mesh never leaving the GPU.

    python examples/render_mesh_synthetic.py [out_dir]

Writes per view <out>/depth_XXX.npy (zbuf, -1 on background), normal_XXX.npy (render_mesh.py's normal map) and
mask_XXX.npy, plus mask_XXX.ppm / normal_XXX.ppm previews, and <out>/visible_faces.npy (texture_mesh.py's visible faces
of the first view).
"""
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, postprocess as pp, scenes  # noqa: E402
from gaustudio_amd.mesh_raster import MeshRasterizer  # noqa: E402
from gaustudio_amd.tsdf import TSDFVolume  # noqa: E402


def write_ppm(path, rgb):
    rgb = np.clip(rgb, 0, 255).astype(np.uint8)
    with open(path, "wb") as fh:
        fh.write(f"P6 {rgb.shape[1]} {rgb.shape[0]} 255\n".encode())
        fh.write(rgb.tobytes())


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "render_mesh_out"
    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    P = 200_000
    d = torch.randn(P, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    xyz = (d * (1.0 + 0.08 * torch.sin(5 * d[:, 0:1]) * torch.cos(4 * d[:, 1:2]))).to(dev)
    scales = torch.full((P, 3), 0.008, device=dev)
    rots = torch.tensor([[1.0, 0, 0, 0]], device=dev).repeat(P, 1)
    opac = torch.full((P, 1), 0.95, device=dev)
    cols = torch.rand(P, 3, generator=g).to(dev)
    cams = scenes.ring_cameras(24, 640, 480, radius=3.2, elevation=0.35) + scenes.ring_cameras(12, 640, 480, radius=3.2, elevation=-0.8)
    volume = TSDFVolume(voxel_size=0.01, sdf_trunc=0.04, capacity_blocks=1 << 18)
    views = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for cam in cams:
        rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0,
                                           cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 0, cam.campos.to(dev), False, False)
        with torch.no_grad():
            _, _, _, median, opacity = GaussianRasterizer(rs)(means3D=xyz, means2D=torch.zeros_like(xyz), opacities=opac,
                                                               colors_precomp=cols, scales=scales, rotations=rots)
        depth = median[0].clone()
        depth[opacity[0] < 0.5] = 0
        f = cam.width / (2 * cam.tanfovx)
        K = torch.tensor([[f, 0, cam.width / 2], [0, f, cam.height / 2], [0, 0, 1]])
        E = cam.viewmatrix.t().contiguous()                                         # Camera.extrinsics (world-to-camera)
        volume.integrate(pp.depth_to_points(depth, K, E, "world"), cam.campos)
        views.append((K, E, cam.height, cam.width, depth))
    verts, faces = volume.extract_triangle_mesh_device(min_weight=5)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    mesh = MeshRasterizer(verts, faces)
    agree = total = agree_c = total_a = 0
    for n, (K, E, H, W, depth) in enumerate(views):
        frags = mesh.rasterize(K, E, H, W)                                          # render_mesh.py:304-318
        mask = frags.pix_to_face >= 0
        normal = mesh.normal_map(frags, E)                                          # render_mesh.py:348-353
        if n == 0:
            np.save(os.path.join(out, "visible_faces.npy"), mesh.visible_faces(frags).nonzero().flatten().cpu().numpy())
        np.save(os.path.join(out, f"depth_{n:03d}.npy"), frags.zbuf.cpu().numpy())
        np.save(os.path.join(out, f"normal_{n:03d}.npy"), normal.cpu().numpy())
        np.save(os.path.join(out, f"mask_{n:03d}.npy"), mask.cpu().numpy())
        write_ppm(os.path.join(out, f"mask_{n:03d}.ppm"), np.repeat(mask.cpu().numpy()[..., None], 3, -1) * 255)
        write_ppm(os.path.join(out, f"normal_{n:03d}.ppm"), (normal.cpu().numpy() + 1) / 2 * 255)
        both = mask & (depth > 0)
        total += int(both.sum())
        agree_c += int(((frags.zbuf - depth).abs() <= 0.02)[both].sum())
        # depth_to_points unprojected pixel (i, j) at (j, i), not at its centre: along those very rays (cx, cy + 0.5) the
        # mesh depth is the fused depth; along the pixel-centre rays it is sampled half a pixel away
        Ka = K.clone()
        Ka[0, 2] += 0.5
        Ka[1, 2] += 0.5
        fa = mesh.rasterize(Ka, E, H, W)
        both_a = (fa.pix_to_face >= 0) & (depth > 0)
        total_a += int(both_a.sum())
        agree += int(((fa.zbuf - depth).abs() <= 0.02)[both_a].sum())
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"{len(views)} views rendered, fused and meshed in {(t1 - t0) * 1e3:.0f} ms: {verts.shape[0]} vertices, "
          f"{faces.shape[0]} triangles; mesh depth / normal / mask maps of every view in {(t2 - t1) * 1e3:.0f} ms "
          f"(with the file writes); mesh depth within 2 voxels of the Gaussians' median depth on "
          f"{100.0 * agree / max(total_a, 1):.2f} % of {total_a} pixels along the fused rays, "
          f"{100.0 * agree_c / max(total, 1):.2f} % of {total} along the pixel-centre rays")


if __name__ == "__main__":
    main()
