#!/usr/bin/env python
"""The gs-extract-mesh loop (gaustudio/scripts/extract_mesh.py:86-146) with every stage on the MI355X:

    Gaussian PLY + cameras.json  ->  GaussianRasterizer (median depth, opacity)  ->  depth_to_points
                                 ->  TSDFVolume.integrate                         ->  extract_triangle_mesh -> PLY

Runs on a synthetic shell of Gaussians written to / read back from the reference's on-disk formats, so it needs no
dataset:   python examples/extract_mesh_synthetic.py [out_dir] [--clean] [--fusion rgbd]

--clean (extract_mesh.py:149-186): the scene gets a small detached blob of Gaussians, the mesh is clustered into connected
components and the clusters with at most half the triangles of the largest one are removed, all on the device
(gaustudio_amd.mesh_clean); the result is written as fused_mesh.ply.

--fusion rgbd: every view's rendered RGB goes into a ColorTSDFVolume together with its median depth (voxel-projective fusion
with a running colour average, gaustudio_amd.tsdf_rgbd) instead of the depth points into a TSDFVolume; the mesh is cleaned,
written as a COLOURED fused_mesh.ply and rendered back with mesh_raster, the vertex colours as the interpolated attribute.
"""
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, formats, postprocess as pp, scenes  # noqa: E402
from gaustudio_amd.tsdf import TSDFVolume  # noqa: E402


def write_inputs(out, floater=False):
    g = torch.Generator().manual_seed(0)
    P = 200_000
    d = torch.randn(P, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    bumps = 1.0 + 0.08 * torch.sin(5 * d[:, 0:1]) * torch.cos(4 * d[:, 1:2])
    xyz = d * bumps
    if floater:                                   # a detached shell of radius 0.12 beside the object: something to remove
        Q = 6_000
        e = torch.randn(Q, 3, generator=g)
        xyz = torch.cat([xyz, 0.12 * e / e.norm(dim=1, keepdim=True) + torch.tensor([1.5, 0.3, 0.0])])
        P += Q
    cloud = formats.GaussianCloud(xyz=xyz, f_dc=(torch.rand(P, 1, 3, generator=g) - 0.5) / 0.28209479177387814,
                                  f_rest=torch.zeros(P, 15, 3), opacity=torch.full((P, 1), 3.0),      # sigmoid -> 0.95
                                  scale=torch.full((P, 3), math.log(0.008)), rot=torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1))
    formats.export_gaussian_ply(os.path.join(out, "point_cloud.ply"), cloud)
    cams = []
    for i, c in enumerate(scenes.ring_cameras(24, 640, 480, radius=3.2, elevation=0.35)
                          + scenes.ring_cameras(12, 640, 480, radius=3.2, elevation=-0.8)):
        w2c = c.viewmatrix.t().numpy().astype(np.float64)
        c2w = np.linalg.inv(w2c)
        f = c.width / (2 * c.tanfovx)
        cams.append({"id": i, "img_name": f"view_{i:03d}", "width": c.width, "height": c.height,
                     "position": c2w[:3, 3].tolist(), "rotation": c2w[:3, :3].tolist(), "fx": f, "fy": f})
    with open(os.path.join(out, "cameras.json"), "w") as fjson:
        json.dump(cams, fjson)


def render_rgbd(cam, act, dev):
    """One view as an RGB-D frame: (median depth [H,W] with 0 where the opacity is below 0.5, RGB [3,H,W] in [0,1],
    (fx, fy, cx, cy), world-to-camera 4x4)."""
    rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0,
                                       cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 0, cam.campos.to(dev), False, False)
    with torch.no_grad():
        color, _, _, median, opacity = GaussianRasterizer(rs)(means3D=act["means3D"], means2D=torch.zeros_like(act["means3D"]),
                                                               opacities=act["opacities"], shs=act["shs"], scales=act["scales"],
                                                               rotations=act["rotations"])
    depth = median[0].clone()
    depth[opacity[0] < 0.5] = 0                                                     # extract_mesh.py:104-107
    f = cam.width / (2 * cam.tanfovx)
    return depth, color.clamp(0.0, 1.0).contiguous(), (f, f, cam.width / 2, cam.height / 2), cam.viewmatrix.t().numpy().astype(np.float64)


def fuse_rgbd_mesh(out, act, cameras, dev):
    from gaustudio_amd import ColorTSDFVolume
    from gaustudio_amd.mesh_raster import MeshRasterizer
    volume = ColorTSDFVolume(voxel_length=0.01, sdf_trunc=0.04, capacity_blocks=1 << 16)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for rec in cameras:
        depth, rgb, K, E = render_rgbd(rec.cam, act, dev)
        volume.integrate(depth, rgb, K, E, depth_trunc=10.0)                         # images never leave the GPU
    v, f, c, n = volume.extract_triangle_mesh_device(min_weight=5, clean_ratio=0.5, with_normals=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    formats.write_ply_mesh(os.path.join(out, "fused_mesh.ply"), v, f, vertex_colors=c, vertex_normals=n)
    # render the coloured mesh back into the first camera: the vertex colours are the interpolated attribute
    cam = cameras[0].cam
    depth, rgb, K, E = render_rgbd(cam, act, dev)
    Kmat = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    mr = MeshRasterizer(v, f)
    frags = mr.rasterize(Kmat, E, cam.height, cam.width)
    img = mr.interpolate(frags, c)
    both = (frags.pix_to_face >= 0) & (depth > 0)
    err = (img[both] - rgb.permute(1, 2, 0)[both]).abs().mean().item() if bool(both.any()) else float("nan")
    np.save(os.path.join(out, "fused_mesh_render.npy"), (img.clamp(0, 1) * 255 + 0.5).to(torch.uint8).cpu().numpy())
    r = v.norm(dim=1)
    print(f"{len(cameras)} views rendered, RGB-D fused, meshed and cleaned in {dt * 1e3:.0f} ms: coloured fused_mesh.ply with "
          f"{v.shape[0]} vertices, {f.shape[0]} triangles, radius {r.min():.3f} .. {r.max():.3f} (shell at 0.92 .. 1.08); "
          f"rendered back into view 0: mean |colour - rendered RGB| = {err:.3f} over {int(both.sum())} pixels")


def main():
    argv = sys.argv[1:]
    fusion = "points"
    if "--fusion" in argv:
        i = argv.index("--fusion")
        fusion = argv[i + 1]
        del argv[i:i + 2]
        if fusion not in ("points", "rgbd"):
            sys.exit("--fusion takes points or rgbd")
    args = [a for a in argv if a != "--clean"]
    clean = "--clean" in argv
    out = args[0] if args else "extract_mesh_out"
    os.makedirs(out, exist_ok=True)
    write_inputs(out, floater=clean)
    dev = torch.device("cuda:0")
    pcd = formats.load_gaussian_ply(os.path.join(out, "point_cloud.ply"), device=dev)
    cameras = formats.load_cameras_json(os.path.join(out, "cameras.json"))
    act = pcd.activated()
    if fusion == "rgbd":
        fuse_rgbd_mesh(out, act, cameras, dev)
        return
    volume = TSDFVolume(voxel_size=0.01, sdf_trunc=0.04, space_carving=False, capacity_blocks=1 << 18)   # extract_mesh.py:86
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for rec in cameras:
        cam = rec.cam
        rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0,
                                           cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 0, cam.campos.to(dev), False, False)
        with torch.no_grad():
            _, _, _, median, opacity = GaussianRasterizer(rs)(means3D=act["means3D"], means2D=torch.zeros_like(act["means3D"]),
                                                               opacities=act["opacities"], shs=act["shs"], scales=act["scales"],
                                                               rotations=act["rotations"])
        depth = median[0].clone()
        invalid = opacity[0] < 0.5                                                  # extract_mesh.py:104-107
        depth[invalid] = 0
        f = cam.width / (2 * cam.tanfovx)
        K = torch.tensor([[f, 0, cam.width / 2], [0, f, cam.height / 2], [0, 0, 1]])
        # :110 compacts `pts[~invalid]` for the CPU library.  Here a masked pixel (depth 0) unprojects to the sensor origin,
        # which the integrate kernel skips, so the whole [H,W,3] map goes in -- as a map: the kernel then works in 32 x 32
        # pixel patches whose rays share voxels in both image directions (same volume, 2.3x faster than a flat list)
        pts = pp.depth_to_points(depth, K, cam.viewmatrix.t().contiguous(), "world")
        volume.integrate(pts, cam.campos)                                           # :115, points never leave the GPU
    if clean:
        clean_mesh(out, volume, len(cameras), t0)
        return
    vertices, faces = volume.extract_triangle_mesh(min_weight=5)                    # :145
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    mesh = np.zeros(len(vertices), dtype=[("x", "f4"), ("y", "f4"), ("z", "f4")])
    mesh["x"], mesh["y"], mesh["z"] = vertices[:, 0], vertices[:, 1], vertices[:, 2]
    formats.write_ply_vertices(os.path.join(out, "fused_mesh_vertices.ply"), mesh)
    np.save(os.path.join(out, "fused_mesh_faces.npy"), faces)
    r = np.linalg.norm(vertices, axis=1)
    print(f"{len(cameras)} views rendered, fused and meshed in {dt * 1e3:.0f} ms: {len(vertices)} vertices, {len(faces)} triangles, "
          f"radius {r.min():.3f} .. {r.max():.3f} (shell at 0.92 .. 1.08)")


def clean_mesh(out, volume, num_views, t0):
    from gaustudio_amd import mesh_clean
    vertices, faces = volume.extract_triangle_mesh_device(min_weight=5)             # :145, the mesh stays in HBM
    _, n_triangles, area = mesh_clean.cluster_connected_triangles(faces, vertices=vertices)              # :158-160
    v2, f2, removed = mesh_clean.remove_small_components(vertices, faces, ratio_threshold=0.5)          # :152-182
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    formats.write_ply_mesh(os.path.join(out, "fused_mesh.ply"), v2, f2)                                # :186
    order = torch.argsort(n_triangles, descending=True)[:5].cpu()
    top = ", ".join(f"{int(n_triangles[i])} triangles / area {float(area[i]):.4f}" for i in order)
    print(f"{num_views} views rendered, fused, meshed and cleaned in {dt * 1e3:.0f} ms: {faces.shape[0]} triangles in "
          f"{n_triangles.numel()} clusters ({mesh_clean.last_rounds} rounds; largest: {top}); removed {removed} triangles and "
          f"{vertices.shape[0] - v2.shape[0]} vertices -> fused_mesh.ply with {v2.shape[0]} vertices, {f2.shape[0]} triangles")


if __name__ == "__main__":
    main()
