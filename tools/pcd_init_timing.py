#!/usr/bin/env python
"""Times of gaustudio_amd.pcd_init on noisy-sphere clouds of 1e5, 1e6 and 4e6 points -> profiles/pcd_init_timing.json.

  * the stages of mean_dist2 (grid build, lane-per-point query, fallback) from the library's own HIP events, and the seed
    kernel (point_seeds with the distances given) from device events;
  * the three grid occupancies 2, 4 and 8 points per occupied cell, alternated inside every repeat so that they see the same
    machine state; all three must give the same bits;
  * the baseline on the same GPU: pcd_fusion.knn(points, 4) followed by the torch mean of columns 1..3 -- the only route to
    these numbers before mean_dist2 existed -- whose result must equal mean_dist2's.

    python tools/pcd_init_timing.py [--repeat 7] [--sizes 100000 1000000 4000000] [--out profiles/pcd_init_timing.json]
Every figure is the median of --repeat calls after one warm-up call per variant; end-to-end times are host clocks around a
call that ends in a device synchronise (the calls read a few counters back, so they wait on the stream themselves)."""
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
from gaustudio_amd import pcd_fusion  # noqa: E402
from gaustudio_amd import pcd_init as pi  # noqa: E402

TARGETS = (2, 4, 8)


def noisy_sphere(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * (1 + rng.normal(0, 0.002, (n, 1)))).astype(np.float32)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def baseline(p):
    d2, _ = pcd_fusion.knn(p, 4)
    return (((d2[:, 1] + d2[:, 2]) + d2[:, 3]) / 3.0).float()


def med(xs):
    return round(statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000, 4_000_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcd_init_timing.json"))
    args = ap.parse_args()
    if args.repeat < 5:
        ap.error("--repeat must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("pcd_init_timing needs a ROCm GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeat, cloud="unit sphere, radial noise sigma 0.002",
               protocol="median of the repeats after one warm-up per variant; occupancies alternated inside each repeat",
               clouds=[])
    for n in args.sizes:
        p = torch.from_numpy(noisy_sphere(n, n % 1000)).to(dev)
        nrm = -p / p.norm(dim=1, keepdim=True)
        ref = baseline(p)                                                   # warm-up of the baseline
        same = True
        stats = {}
        for t in TARGETS:                                                   # warm-up, and the equality of every variant
            d2, stats[t] = pi.mean_dist2(p, return_stats=True, cell_target=t)
            same = same and bool(torch.equal(d2, ref))
        default_d2 = pi.mean_dist2(p)
        same = same and bool(torch.equal(default_d2, ref))
        pi.point_seeds(p, normals=nrm, dist2=default_d2)
        pi.pcd_init(p, None, nrm)
        ts = {t: dict(total=[], grid=[], query=[], fallback=[]) for t in TARGETS}
        base, seeds, e2e, dflt = [], [], [], []
        for _ in range(args.repeat):
            for t in TARGETS:
                ms, (_, st) = wall(lambda: pi.mean_dist2(p, return_stats=True, cell_target=t))
                ts[t]["total"].append(ms)
                for k in ("grid", "query", "fallback"):
                    ts[t][k].append(st[k + "_ms"])
            dflt.append(wall(lambda: pi.mean_dist2(p))[0])
            base.append(wall(lambda: baseline(p))[0])
            seeds.append(events(lambda: pi.point_seeds(p, normals=nrm, dist2=default_d2))[0])
            e2e.append(wall(lambda: pi.pcd_init(p, None, nrm))[0])
        entry = dict(points=n, results_equal_baseline_and_each_other=same, occupancy_trials=[], seeds_kernel_ms=med(seeds),
                     mean_dist2_default_ms=med(dflt), pcd_init_end_to_end_ms=med(e2e), baseline_knn4_mean_ms=med(base),
                     baseline_over_mean_dist2=round(statistics.median(base) / statistics.median(dflt), 3))
        for t in TARGETS:
            entry["occupancy_trials"].append(dict(
                cell_target=t, occupied_cells=stats[t]["occupied_cells"], shell2_lanes=stats[t]["shell2_lanes"],
                leftovers=stats[t]["leftovers"], mean_dist2_ms=med(ts[t]["total"]), grid_build_ms=med(ts[t]["grid"]),
                lane_query_ms=med(ts[t]["query"]), fallback_ms=med(ts[t]["fallback"]),
                mean_dist2_ms_min_max=[round(min(ts[t]["total"]), 4), round(max(ts[t]["total"]), 4)]))
        res["clouds"].append(entry)
        print(json.dumps(entry), flush=True)
        del p, nrm, ref, default_d2
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
