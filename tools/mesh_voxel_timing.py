#!/usr/bin/env python
"""GPU times of the mesh voxelizer's stages -- plan, count, emit, sort, closest -- next to the reference's formulation of the
voxelization (every voxel against every triangle) on the same GPU in the same run.

    python tools/mesh_voxel_timing.py [--sizes 64 128 256] [--subdivisions 5] [--out profiles/mesh_voxel_timing.json]

Mesh: an icosphere of 20 * 4^subdivisions triangles (20 480 by default) with vertex colours, normalised to the unit cube.
Baseline: a torch restatement, in float64, of what Open3D's create_from_triangle_mesh_within_bounds computes for the
reference's VoxelInitializer (mesh.py:354-379) -- the triangle / box separating-axis test for ALL n^3 voxels x ALL triangles,
in chunks of voxels.  It is the reference's formulation, not the code under test; its voxel set is compared with ours.  It is
quadratic and runs at 1/64 only, once.  Our times are HIP events on the stream around each stage after one warm-up call, the
median of `--repeats` calls; a stage's time includes its read-back of the count that sizes the next stage (one host wait).
No threshold and no promised ratio: the JSON is the record."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaustudio_amd import voxelize as vx  # noqa: E402

STAGES = ("plan", "count", "emit", "sort")


def icosphere(subdivisions):
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


def stage_times(vn, faces, colors, vs, repeats):
    """Median per-stage milliseconds over `repeats` calls after one warm-up, and the last call's results."""
    rows = []
    for it in range(repeats + 1):
        marks = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))
        grid = vx.voxelize_stages(vn, faces, vs, vx.UNIT_MIN, vx.UNIT_MAX, on_stage=mark)
        a = torch.cuda.Event(enable_timing=True)
        a.record()
        near = vx.closest_on_mesh(grid, vn, faces, colors)
        b = torch.cuda.Event(enable_timing=True)
        b.record()
        torch.cuda.synchronize()
        row = {marks[k][0]: marks[k][1].elapsed_time(marks[k + 1][1]) for k in range(len(marks) - 1)}
        row["closest"] = a.elapsed_time(b)
        if it:
            rows.append(row)
    med = {k + "_ms": statistics.median(r[k] for r in rows) for k in STAGES + ("closest",)}
    totals = [sum(r[k] for k in STAGES) for r in rows]
    med["voxelize_ms"] = statistics.median(totals)
    med["voxelize_ms_min_max"] = [min(totals), max(totals)]                      # the spread of the repeats
    med["closest_ms_min_max"] = [min(r["closest"] for r in rows), max(r["closest"] for r in rows)]
    return med, grid, near


def tribox_all(c, h, t0, t1, t2):
    """The separating-axis test for voxel centres c [V,1,3] against triangles t0, t1, t2 [1,F,3] in float64: bool [V,F]."""
    v0, v1, v2 = t0 - c, t1 - c, t2 - c
    e0, e1, e2 = v1 - v0, v2 - v1, v0 - v2
    X, Y, Z = 0, 1, 2
    out = torch.zeros(v0.shape[:2], dtype=torch.bool, device=c.device)

    def axis(pa, pb, rad):
        return (torch.minimum(pa, pb) > rad) | (torch.maximum(pa, pb) < -rad)

    def rad(a, b):
        return a.abs() * h + b.abs() * h
    for e, (xa, xb), (ya, yb), (za, zb) in ((e0, (v0, v2), (v0, v2), (v1, v2)), (e1, (v0, v2), (v0, v2), (v0, v1)),
                                            (e2, (v0, v1), (v0, v1), (v1, v2))):
        a, b = e[..., Z], e[..., Y]
        out |= axis(a * xa[..., Y] - b * xa[..., Z], a * xb[..., Y] - b * xb[..., Z], rad(a, b))
        a, b = e[..., Z], e[..., X]
        out |= axis(-a * ya[..., X] + b * ya[..., Z], -a * yb[..., X] + b * yb[..., Z], rad(a, b))
        a, b = e[..., Y], e[..., X]
        out |= axis(a * za[..., X] - b * za[..., Y], a * zb[..., X] - b * zb[..., Y], rad(a, b))
    mn = torch.minimum(torch.minimum(v0, v1), v2)
    mx = torch.maximum(torch.maximum(v0, v1), v2)
    out |= ((mn > h) | (mx < -h)).any(dim=-1)
    n = torch.stack([e0[..., Y] * e1[..., Z] - e0[..., Z] * e1[..., Y], e0[..., Z] * e1[..., X] - e0[..., X] * e1[..., Z],
                     e0[..., X] * e1[..., Y] - e0[..., Y] * e1[..., X]], dim=-1)
    vmin = torch.where(n > 0, -h - v0, h - v0)
    vmax = torch.where(n > 0, h - v0, -h - v0)
    out |= (n[..., 0] * vmin[..., 0] + n[..., 1] * vmin[..., 1] + n[..., 2] * vmin[..., 2]) > 0
    out |= ~((n[..., 0] * vmax[..., 0] + n[..., 1] * vmax[..., 1] + n[..., 2] * vmax[..., 2]) >= 0)
    return ~out


def baseline_voxelize(vn, faces, n, chunk):
    """Occupied linear indices, ascending: all n^3 voxels x all triangles."""
    vs = 1.0 / n
    h = vs / 2
    t0, t1, t2 = (vn[faces[:, k].long()].unsqueeze(0) for k in range(3))
    ax = (-0.5 + h) + torch.arange(n, dtype=torch.float64, device=vn.device) * vs
    hit = []
    for a in range(0, n ** 3, chunk):
        lin = torch.arange(a, min(a + chunk, n ** 3), device=vn.device)
        c = torch.stack([ax[lin // (n * n)], ax[(lin // n) % n], ax[lin % n]], dim=-1).unsqueeze(1)
        hit.append(lin[tribox_all(c, h, t0, t1, t2).any(dim=1)])
    return torch.cat(hit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256], help="voxel_size = 1 / size")
    ap.add_argument("--subdivisions", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-size", type=int, default=64)
    ap.add_argument("--baseline-chunk", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_voxel_timing.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    v, f, col = (torch.from_numpy(a).to(dev) for a in icosphere(args.subdivisions))
    vn, scale, center = vx.normalize_mesh(v)
    out = {"device": torch.cuda.get_device_name(0), "triangles": int(f.shape[0]), "vertices": int(v.shape[0]), "arithmetic": "float64",
           "repeats": args.repeats, "grids": []}
    for n in args.sizes:
        med, grid, near = stage_times(vn, f, col, 1.0 / n, args.repeats)
        g = {"voxel_size": f"1/{n}", "shape": list(grid.shape), "voxels": grid.num_voxels, "pairs": int(grid.pair_tri.shape[0]), **med,
             "all_stages_ms": med["voxelize_ms"] + med["closest_ms"], "unmatched_voxels": int((near["closest_tri"] < 0).sum())}
        if n == args.baseline_size:
            baseline_voxelize(vn, f[:64], 8, 64)                                 # warm-up: code objects, allocator
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ref = baseline_voxelize(vn, f, n, args.baseline_chunk)
            b.record()
            torch.cuda.synchronize()
            g["baseline_all_voxels_x_all_triangles_ms"] = a.elapsed_time(b)
            g["baseline_tests"] = n ** 3 * int(f.shape[0])
            g["baseline_over_voxelize"] = g["baseline_all_voxels_x_all_triangles_ms"] / med["voxelize_ms"]
            g["baseline_same_voxel_set"] = bool(torch.equal(ref.to(torch.int32), grid.voxel_index))
            del ref
            torch.cuda.empty_cache()
        out["grids"].append(g)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
