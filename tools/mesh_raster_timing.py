#!/usr/bin/env python
"""Device-synchronised times of gaustudio_amd.mesh_raster (csrc/gsr_mesh.hip) at 1080p:

  * the TSDF mesh of a synthetic Gaussian shell (operator renders -> TSDF -> marching cubes, voxel 0.01);
  * a 2 M-face bumpy sphere (1024 x 1000 lat-long grid);
each for rasterize (the whole call: setup, binning with its one host read, sort, walk), interpolate (3 channels),
normal_map, visible_faces and vertex_normals.

    python tools/mesh_raster_timing.py [--repeat 10]
Prints one line per measurement (median of --repeat runs after one warm-up) and a JSON summary line; the summary also
holds each measurement's least and greatest repeat ("<name>_range"), the run-to-run spread to judge a difference by.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, postprocess as pp, scenes  # noqa: E402
from gaustudio_amd.mesh_raster import MeshRasterizer  # noqa: E402
from gaustudio_amd.tsdf import TSDFVolume  # noqa: E402

DEV = torch.device("cuda", 0)


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """World-to-camera 4x4 in OpenCV axes (x right, y down, z forward) for a camera at `eye` looking at `target`."""
    eye, target, up = (np.asarray(x, dtype=np.float64) for x in (eye, target, up))
    zc = target - eye
    zc /= np.linalg.norm(zc)
    xc = np.cross(zc, up)
    xc /= np.linalg.norm(xc)
    R = np.stack([xc, np.cross(zc, xc), zc])
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ eye
    return E


def sphere_grid(nu, nv, seed=0):
    """A bumpy sphere from an nu x nv lat-long grid: 2 nu nv faces."""
    rng = np.random.default_rng(seed)
    th = (np.arange(nv + 1) + 0.5) / (nv + 1) * np.pi
    ph = np.arange(nu) / nu * 2 * np.pi
    T, P = np.meshgrid(th, ph, indexing="ij")
    r = 1 + 0.05 * np.sin(7 * P) * np.sin(5 * T) + 0.002 * rng.random(T.shape)
    v = np.stack([r * np.sin(T) * np.cos(P), r * np.cos(T), r * np.sin(T) * np.sin(P)], -1).reshape(-1, 3)
    iv, iu = np.meshgrid(np.arange(nv), np.arange(nu), indexing="ij")
    a = iv * nu + iu
    b = iv * nu + (iu + 1) % nu
    c, d = a + nu, b + nu
    f = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)])
    return v.astype(np.float32), f.astype(np.int32)


def gpu_time(fn, repeat):
    fn()
    ts = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, [min(ts) * 1e3, max(ts) * 1e3]


def tsdf_mesh():
    g = torch.Generator().manual_seed(0)
    P = 200_000
    d = torch.randn(P, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    xyz = (d * (1.0 + 0.08 * torch.sin(5 * d[:, 0:1]) * torch.cos(4 * d[:, 1:2]))).to(DEV)
    scales = torch.full((P, 3), 0.008, device=DEV)
    rots = torch.tensor([[1.0, 0, 0, 0]], device=DEV).repeat(P, 1)
    opac = torch.full((P, 1), 0.95, device=DEV)
    cols = torch.rand(P, 3, generator=g).to(DEV)
    vol = TSDFVolume(voxel_size=0.01, sdf_trunc=0.04, capacity_blocks=1 << 18)
    for cam in scenes.ring_cameras(24, 640, 480, radius=3.2, elevation=0.35) + scenes.ring_cameras(12, 640, 480, radius=3.2, elevation=-0.8):
        rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0,
                                           cam.viewmatrix.to(DEV), cam.projmatrix.to(DEV), 0, cam.campos.to(DEV), False, False)
        with torch.no_grad():
            _, _, _, median, opacity = GaussianRasterizer(rs)(means3D=xyz, means2D=torch.zeros_like(xyz), opacities=opac,
                                                               colors_precomp=cols, scales=scales, rotations=rots)
        depth = median[0].clone()
        depth[opacity[0] < 0.5] = 0
        f = cam.width / (2 * cam.tanfovx)
        K = torch.tensor([[f, 0, cam.width / 2], [0, f, cam.height / 2], [0, 0, 1]])
        vol.integrate(pp.depth_to_points(depth, K, cam.viewmatrix.t().contiguous(), "world"), cam.campos)
    return vol.extract_triangle_mesh_device(min_weight=5)


def measure(name, verts, faces, K, E, H, W, repeat):
    r = MeshRasterizer(verts, faces)
    res = {"faces": int(faces.shape[0]), "vertices": int(verts.shape[0])}
    fr = r.rasterize(K, E, H, W)
    res["covered_pixels"] = int((fr.pix_to_face >= 0).sum())
    res["binned_entries"] = int(r.last_binned)
    attr = torch.rand((verts.shape[0], 3), device=DEV)

    def timed(key, fn):
        res[key], res[key + "_range"] = gpu_time(fn, repeat)
    timed("rasterize_ms", lambda: r.rasterize(K, E, H, W))
    timed("rasterize_cull_ms", lambda: r.rasterize(K, E, H, W, cull_backfaces=True))
    timed("interpolate3_ms", lambda: r.interpolate(fr, attr))
    r.vertex_normals()
    timed("normal_map_ms", lambda: r.normal_map(fr, E))
    timed("visible_faces_ms", lambda: r.visible_faces(fr))

    def vn():
        r._normals = None
        r.vertex_normals()
    timed("vertex_normals_ms", vn)
    print(name, " ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in res.items() if not k.endswith("_range")),
          flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    a = ap.parse_args()
    H, W = 1080, 1920
    f = 1400.0
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
    E = look_at([1.2, 0.9, -2.6], [0, 0, 0])
    out = {}
    v, t = tsdf_mesh()
    out["tsdf_mesh_1080p"] = measure("tsdf_mesh_1080p", v, t, K, E, H, W, a.repeat)
    vs, fs = sphere_grid(1024, 1000)
    out["sphere_2M_1080p"] = measure("sphere_2M_1080p", torch.from_numpy(vs).to(DEV), torch.from_numpy(fs).to(DEV), K,
                                     look_at([0.3, 0.4, -2.6], [0, 0, 0]), H, W, a.repeat)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
