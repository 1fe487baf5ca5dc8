#!/usr/bin/env python
"""Per-stage GPU times of ColorTSDFVolume on the synthetic extraction scene (examples/extract_mesh_synthetic.py): touch,
compact, integrate per frame, classify and emit per mesh -- next to TSDFVolume.integrate (depth_to_points + the ray
integration) on the same rendered frames as the comparison point, and the touch kernel's block insertions with and without
its lane-neighbour filter.

    python tools/tsdf_rgbd_timing.py [--views 36] [--out profiles/tsdf_rgbd_timing.json]

Times are HIP events around each stage, after one warm-up pass over all frames; the frames are rendered once and kept on
the device.  No threshold: the JSON is the record.
"""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import extract_mesh_synthetic as ex  # noqa: E402
from gaustudio_amd import ColorTSDFVolume, formats, postprocess as pp  # noqa: E402
from gaustudio_amd.tsdf import TSDFVolume  # noqa: E402

VOXEL, TRUNC, CAPACITY = 0.01, 0.04, 1 << 16


def fuse_color(frames, timings=None, counters=None):
    vol = ColorTSDFVolume(VOXEL, TRUNC, capacity_blocks=CAPACITY)
    vol.timings, vol.counters = timings, counters
    for depth, rgb, K, E, _, _ in frames:
        vol.integrate(depth, rgb, K, E, depth_trunc=10.0)
    return vol


def fuse_points(frames, record):
    vol = TSDFVolume(VOXEL, TRUNC, capacity_blocks=1 << 18)
    ms = {"depth_to_points_ms": 0.0, "integrate_ms": 0.0}
    for depth, _, _, _, Kmat, cam in frames:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        pts = pp.depth_to_points(depth, Kmat, cam.viewmatrix.t().contiguous(), "world")
        ev[1].record()
        vol.integrate(pts, cam.campos)
        ev[2].record()
        torch.cuda.synchronize()
        ms["depth_to_points_ms"] += ev[0].elapsed_time(ev[1])
        ms["integrate_ms"] += ev[1].elapsed_time(ev[2])
    if record is not None:
        record.update(ms)
    return vol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=36)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_rgbd_timing.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        ex.write_inputs(tmp)
        pcd = formats.load_gaussian_ply(os.path.join(tmp, "point_cloud.ply"), device=dev)
        cameras = formats.load_cameras_json(os.path.join(tmp, "cameras.json"))[:args.views]
    act = pcd.activated()
    frames = []
    for rec in cameras:
        depth, rgb, K, E = ex.render_rgbd(rec.cam, act, dev)
        Kmat = torch.tensor([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
        frames.append((depth, rgb, K, E, Kmat, rec.cam))
    H, W = frames[0][0].shape
    fuse_color(frames)                                                    # warm-up: code objects, allocator
    fuse_points(frames, None)
    torch.cuda.synchronize()
    stages, counters = {}, torch.zeros(2, dtype=torch.int64, device=dev)
    vol = fuse_color(frames, stages, counters)
    mesh_ms = {}
    v, f, c = vol._extract_triangle_mesh_device(0.0, timings=mesh_ms)
    unfiltered = fuse_color(frames[:1])                                   # the same volume with the filter off: it changes no result
    plain = ColorTSDFVolume(VOXEL, TRUNC, capacity_blocks=CAPACITY)
    plain.lane_filter = False
    plain.integrate(*frames[0][:4], depth_trunc=10.0)
    same = bool(torch.equal(plain.keys, unfiltered.keys) and torch.equal(plain.voxels, unfiltered.voxels))
    ray = {}
    fuse_points(frames, ray)
    asked, made = [int(x) for x in counters.cpu()]
    out = {
        "device": torch.cuda.get_device_name(0), "views": len(frames), "image": [H, W], "voxel_length": VOXEL, "sdf_trunc": TRUNC,
        "depth_sampling_stride": vol.depth_sampling_stride,
        "color_tsdf": {"per_frame_ms": {k: v_ / len(frames) for k, v_ in stages.items()}, "total_ms": dict(stages),
                       "mesh_ms": mesh_ms, "occupied_blocks": int(vol.occupied_blocks()[0].shape[0]),
                       "vertices": int(v.shape[0]), "triangles": int(f.shape[0])},
        "touch_insertions": {"without_lane_filter": asked, "with_lane_filter": made,
                             "ratio": (asked / made) if made else None, "filter_changes_the_volume": not same},
        "ray_tsdf": {"per_frame_ms": {k: v_ / len(frames) for k, v_ in ray.items()}, "total_ms": ray},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
