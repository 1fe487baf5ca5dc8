#!/usr/bin/env python
"""Device-synchronised times of gaustudio_amd.mesh_clean (csrc/gsr_mesh_clean.hip) on two meshes:

  * the TSDF mesh of examples/extract_mesh_synthetic.py --clean (a Gaussian shell and a small detached blob: operator renders
    -> TSDF -> marching cubes, voxel 0.01), together with the time of extract_triangle_mesh_device on the same volume;
  * a ~2 M-face mesh: two icospheres (20 * 4^8 and 20 * 4^7 faces) and 4000 detached 80-face pieces, faces shuffled;
each for clustering (gsr_mesh_cluster_triangles: edge sort, union edges, hook-and-jump rounds, renumbering, counts), the areas
(gsr_mesh_cluster_area), the compaction (gsr_mesh_compact) and remove_small_components as a whole, with the round count, and
against the host route it replaces: device -> host copy, scipy.sparse.csgraph.connected_components + numpy mask removal
(tests/mesh_clean_model.py), host -> device copy.

    python tools/mesh_clean_timing.py [--repeat 10]
Prints one line per mesh (median of --repeat runs after one warm-up) and a JSON summary line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import mesh_clean_model as cm  # noqa: E402
import mesh_raster_model as mm  # noqa: E402
from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, _C, formats, mesh_clean, postprocess as pp  # noqa: E402
from gaustudio_amd._abi import Workspace  # noqa: E402
from gaustudio_amd.tsdf import TSDFVolume  # noqa: E402

DEV = torch.device("cuda", 0)


def gpu_time(fn, repeat):
    fn()
    ts = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def example_volume(out_dir):
    """The volume of examples/extract_mesh_synthetic.py --clean."""
    import extract_mesh_synthetic as ex
    os.makedirs(out_dir, exist_ok=True)
    ex.write_inputs(out_dir, floater=True)
    act = formats.load_gaussian_ply(os.path.join(out_dir, "point_cloud.ply"), device=DEV).activated()
    vol = TSDFVolume(voxel_size=0.01, sdf_trunc=0.04, capacity_blocks=1 << 18)
    for rec in formats.load_cameras_json(os.path.join(out_dir, "cameras.json")):
        cam = rec.cam
        rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0,
                                           cam.viewmatrix.to(DEV), cam.projmatrix.to(DEV), 0, cam.campos.to(DEV), False, False)
        with torch.no_grad():
            _, _, _, median, opacity = GaussianRasterizer(rs)(means3D=act["means3D"], means2D=torch.zeros_like(act["means3D"]),
                                                               opacities=act["opacities"], shs=act["shs"], scales=act["scales"],
                                                               rotations=act["rotations"])
        depth = median[0].clone()
        depth[opacity[0] < 0.5] = 0
        f = cam.width / (2 * cam.tanfovx)
        K = torch.tensor([[f, 0, cam.width / 2], [0, f, cam.height / 2], [0, 0, 1]])
        vol.integrate(pp.depth_to_points(depth, K, cam.viewmatrix.t().contiguous(), "world"), cam.campos)
    return vol


def big_mesh(seed=21):
    rng = np.random.default_rng(seed)
    v1, f1 = cm.subdivide_sphere(*mm.icosphere(3), times=4)
    v0, f0 = cm.subdivide_sphere(v1, f1)
    vs, fs, base = [v0, v1 * 0.5 + [3, 0, 0]], [f0, f1 + len(v0)], len(v0) + len(v1)
    vt, ft = mm.icosphere(1)
    for _ in range(4000):
        vs.append(vt * 0.01 + rng.normal(size=3) * 5)
        fs.append(ft + base)
        base += len(vt)
    faces = np.concatenate(fs).astype(np.int32)
    return np.concatenate(vs).astype(np.float32), faces[rng.permutation(len(faces))]


def measure(name, verts, faces, repeat):
    F, V = faces.shape[0], verts.shape[0]
    L = _C.lib()
    clusters = torch.empty(F, dtype=torch.int32, device=DEV)
    counts = torch.empty(F, dtype=torch.int32, device=DEV)
    rounds = ctypes.c_int(0)
    st = _C._stream(DEV)

    def cluster():
        ws = Workspace(DEV)
        return L.gsr_mesh_cluster_triangles(ws.fn, None, _C._ptr(faces), ctypes.c_int(F), ctypes.c_int(V), _C._ptr(clusters),
                                            _C._ptr(counts), ctypes.byref(rounds), st)
    C = cluster()
    assert C > 0
    area = torch.empty(C, dtype=torch.float64, device=DEV)

    def areas():
        ws = Workspace(DEV)
        assert L.gsr_mesh_cluster_area(ws.fn, None, _C._ptr(verts), ctypes.c_int(V), _C._ptr(faces), ctypes.c_int(F),
                                       _C._ptr(clusters), ctypes.c_int(C), _C._ptr(area), st) == 0
    remove = ~mesh_clean.keep_clusters(counts[:C], 0.5)[clusters.long()]
    res = {"faces": F, "vertices": V, "clusters": C, "removed": int(remove.sum())}
    res["cluster_ms"] = gpu_time(cluster, repeat)
    res["rounds"] = int(rounds.value)
    res["area_ms"] = gpu_time(areas, repeat)
    res["compact_ms"] = gpu_time(lambda: mesh_clean.remove_triangles_by_mask(verts, faces, remove), repeat)
    res["remove_small_components_ms"] = gpu_time(lambda: mesh_clean.remove_small_components(verts, faces, 0.5), repeat)

    # the host route: D2H, scipy connected components + numpy removal, H2D
    def host():
        t0 = time.perf_counter()
        v, f = verts.cpu().numpy(), faces.cpu().numpy()
        t1 = time.perf_counter()
        out = cm.remove_small_components(v, f, 0.5, cluster=cm.cluster_scipy)
        t2 = time.perf_counter()
        torch.from_numpy(np.ascontiguousarray(out[0])).to(DEV), torch.from_numpy(out[1]).to(DEV)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3
    host()
    runs = [host() for _ in range(3)]
    res["host_d2h_ms"], res["host_scipy_model_ms"], res["host_h2d_ms"] = (statistics.median(r[k] for r in runs) for k in range(3))
    res["host_route_ms"] = statistics.median(sum(r) for r in runs)
    print(name, " ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in res.items()), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out", default="mesh_clean_timing_out")
    a = ap.parse_args()
    out = {}
    vol = example_volume(a.out)
    v, t = vol.extract_triangle_mesh_device(min_weight=5)
    out["tsdf_mesh"] = measure("tsdf_mesh", v, t, a.repeat)
    out["tsdf_mesh"]["extract_triangle_mesh_device_ms"] = gpu_time(lambda: vol.extract_triangle_mesh_device(min_weight=5), a.repeat)
    out["tsdf_mesh"]["extract_with_clean_ratio_ms"] = gpu_time(lambda: vol.extract_triangle_mesh_device(min_weight=5, clean_ratio=0.5), a.repeat)
    print("tsdf_mesh extract_triangle_mesh_device_ms=%.3f with clean_ratio=0.5: %.3f" % (
        out["tsdf_mesh"]["extract_triangle_mesh_device_ms"], out["tsdf_mesh"]["extract_with_clean_ratio_ms"]), flush=True)
    del vol
    vs, fs = big_mesh()
    out["big_mesh_2M"] = measure("big_mesh_2M", torch.from_numpy(vs).to(DEV), torch.from_numpy(fs).to(DEV), a.repeat)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
