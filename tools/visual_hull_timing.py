#!/usr/bin/env python
"""GPU times of the visual hull stages -- mask packing, the carve, marching cubes -- next to the reference's formulation of
the carve on the same GPU in the same run.

    python tools/visual_hull_timing.py [--res 128 256 512] [--views 100] [--size 800] [--out profiles/visual_hull_timing.json]

Scene: `views` cameras on two rings around a sphere of radius 0.5, disc silhouettes at size x size, grid half-edge 0.9.
Baseline: a torch restatement of mask.py:59-68 with Camera.insideView (datasets/__init__.py:268-305) -- the materialised
[R^3, 3] float32 point array and about ten elementwise passes over it per camera.  It is the reference's formulation, not the
code under test; its `filled` is compared with ours (the clip coordinates come from torch.matmul there: voxels on a decision
boundary may differ, the count is recorded).  Times are HIP events after one warm-up call, the median of `--repeats` calls
(the baseline at the largest grid: one call).  No threshold and no promised ratio: the JSON is the record.

Algorithmic bytes of the carve = packed masks + camera table + the R^3 u8 output (+ the three axis tables); the achieved
rate is set against it, and `projections` (voxel x camera evaluations actually made, from carved_by) against the time."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaustudio_amd import scenes, visual_hull as vh  # noqa: E402
from gaustudio_amd.sap import marching_cubes  # noqa: E402

SPHERE, HALF = 0.5, 0.9


def scene(views, size, dev):
    n1 = (2 * views) // 3
    cams = scenes.ring_cameras(n1, size, size, radius=3.0, fovx_deg=40.0, elevation=0.35) + \
        scenes.ring_cameras(views - n1, size, size, radius=3.0, fovx_deg=40.0, elevation=-0.9)
    v, u = torch.meshgrid(torch.arange(size, device=dev), torch.arange(size, device=dev), indexing="ij")
    masks = []
    for cam in cams:
        d = float(cam.campos.norm())
        r = (size / 2) / cam.tanfovx * SPHERE / math.sqrt(d * d - SPHERE * SPHERE)
        masks.append((((u + 0.5 - size / 2) ** 2 + (v + 0.5 - size / 2) ** 2) <= r * r).to(torch.float32))
    return cams, masks


def timed(fn, repeats):
    fn()                                                                        # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), out


def inside_view(points, M, W, H, mask):
    """Camera.insideView, line for line."""
    if mask is None:
        mask = torch.ones(H, W, device=points.device)
    hom = torch.cat([points, torch.ones_like(points[:, :1])], dim=-1)
    clip = torch.matmul(hom, M)
    ndc = clip[:, :3] / clip[:, 3:4]
    pixel_x = (ndc[:, 0] + 1) * 0.5 * W
    pixel_y = (1 + ndc[:, 1]) * 0.5 * H
    in_front = clip[:, 2] > 0
    inside_image = (ndc[:, 0] >= -1) & (ndc[:, 0] <= 1) & (ndc[:, 1] >= -1) & (ndc[:, 1] <= 1)
    valid = in_front & inside_image
    inside_mask = torch.zeros_like(valid, dtype=torch.bool)
    if valid.any():
        vx = pixel_x[valid].long().clamp(0, W - 1)
        vy = pixel_y[valid].long().clamp(0, H - 1)
        inside_mask[valid] = mask[vy, vx].bool()
    return inside_mask


def baseline_carve(points, cams, masks, dev):
    """mask.py:57-68."""
    filled = torch.ones((points.shape[0]), device=dev).bool()
    for cam, mask in zip(cams, masks):
        M = cam.projmatrix.to(dev)
        inside = inside_view(points, M, cam.width, cam.height, None)
        idx = torch.where(inside)[0]
        inside_mask = inside_view(points[idx], M, cam.width, cam.height, mask)
        camera_filled = torch.zeros((points.shape[0]), device=dev).bool()
        camera_filled[idx] = inside_mask
        filled = filled & camera_filled
    return filled


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-max-res", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visual_hull_timing.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cams, masks = scene(args.views, args.size, dev)
    cameras = [(cam.projmatrix, cam.width, cam.height) for cam in cams]
    pack_ms, packed = timed(lambda: vh.pack_masks(masks, device=dev), args.repeats)
    mask_bytes = packed[0].numel() * 4
    out = {"device": torch.cuda.get_device_name(0), "views": args.views, "image": [args.size, args.size], "mask_dtype": "float32",
           "pack_ms_all_views": pack_ms, "packed_mask_bytes": mask_bytes, "mask_bytes_read_by_pack": sum(m.numel() * 4 for m in masks),
           "grids": []}
    translate = np.zeros(3)
    for R in args.res:
        axes = vh.grid_axes(R, HALF, translate)
        # the carve alone: masks packed once; includes the table upload and the read-back of the count (one host wait)
        carve_ms, (filled, count, _) = timed(lambda: vh.carve_axes(cameras, masks, axes, packed=packed), args.repeats)
        _, _, carved_by = vh.carve_axes(cameras, masks, axes, return_carved_by=True, packed=packed)
        projections = int(torch.where(carved_by < 0, args.views, carved_by + 1).sum(dtype=torch.int64))
        del carved_by
        hull = vh.VisualHull(filled, axes, translate, HALF, count)
        empty = (~filled).to(torch.float32)
        mc_ms, (verts, faces) = timed(lambda: marching_cubes(empty, 0.5), args.repeats)
        mesh_ms, _ = timed(hull.extract_mesh, args.repeats)
        del empty
        alg_bytes = mask_bytes + args.views * 96 + R ** 3 + 3 * R * 4
        g = {"resolution": R, "voxels": R ** 3, "filled": count, "carve_ms": carve_ms, "marching_cubes_ms": mc_ms,
             "extract_mesh_ms": mesh_ms, "vertices": int(verts.shape[0]), "triangles": int(faces.shape[0]),
             "projections": projections, "projections_per_voxel": projections / R ** 3,
             "projections_per_second": projections / (carve_ms * 1e-3), "algorithmic_bytes": alg_bytes,
             "achieved_GB_per_s": alg_bytes / (carve_ms * 1e-3) / 1e9}
        # issue-bound: the algorithmic traffic moves at a small fraction of HBM speed, the time goes to the ~60 VALU
        # instructions (two correctly rounded divides among them) of a projection
        g["issue_bound"] = bool(g["achieved_GB_per_s"] < 0.1 * 8000)
        if R <= args.baseline_max_res:
            try:
                x, y, z = np.meshgrid(*(np.linspace(-HALF, HALF, R),) * 3)
                pts = torch.from_numpy(np.stack([x.flatten(), y.flatten(), z.flatten()], axis=-1) - translate).float().to(dev)
                del x, y, z
                reps = 1 if R >= 512 else min(args.repeats, 3)
                base_ms, ref = timed(lambda: baseline_carve(pts, cams, masks, dev), reps)
                g["baseline_torch_ms"] = base_ms
                g["baseline_over_carve"] = base_ms / carve_ms
                g["baseline_over_pack_plus_carve"] = base_ms / (carve_ms + pack_ms)
                g["voxels_differing_from_baseline"] = int((ref != filled.flatten()).sum())
                del pts, ref
            except torch.cuda.OutOfMemoryError:
                g["baseline_torch_ms"] = None
                g["baseline_note"] = "skipped: the [R^3, 3] point array and its temporaries do not fit"
            torch.cuda.empty_cache()
        else:
            g["baseline_torch_ms"] = None
            g["baseline_note"] = "skipped (--baseline-max-res)"
        out["grids"].append(g)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
