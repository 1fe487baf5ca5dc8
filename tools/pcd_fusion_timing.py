#!/usr/bin/env python
"""Device-synchronised times of gaustudio_amd.pcd_fusion at user sizes, with the float64 CPU model
(tests/pcd_fusion_model.py: scipy cKDTree + numpy) on the same inputs for scale:

  * knn on 1 M surface points at k = 10 / 20 / 50;
  * normal fusion of 100 views x 500 k records over 1 M Gaussians (finalize: sort, two reductions, 10-NN smoothing);
  * cleaning (statistical + normal test) of 1 M points.

    python tools/pcd_fusion_timing.py [--repeat 5] [--no-cpu]
Prints one line per measurement (median of --repeat runs after one warm-up) and a JSON summary line.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gaustudio_amd import pcd_fusion  # noqa: E402


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


def cpu_time(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def surface(n, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    return d * (1.0 + 0.05 * torch.sin(5 * d[:, :1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU model")
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--records", type=int, default=500_000, help="records per view")
    args = ap.parse_args()
    import pcd_fusion_model as model
    dev = torch.device("cuda", 0)
    res = {}

    pts = surface(1_000_000, 0)
    p_dev = pts.to(dev)
    for k in (10, 20, 50):
        res[f"knn_1M_k{k}_ms"] = gpu_time(lambda: pcd_fusion.knn(p_dev, k), args.repeat)
        if not args.no_cpu:
            res[f"knn_1M_k{k}_cpu_ms"] = cpu_time(lambda: model.knn(pts.numpy(), k))
        print(f"knn 1 M surface points k={k}: GPU {res[f'knn_1M_k{k}_ms']:.2f} ms"
              + ("" if args.no_cpu else f", CPU model {res[f'knn_1M_k{k}_cpu_ms']:.0f} ms"), flush=True)

    # fusion: 1 M Gaussians, views x records
    P = 1_000_000
    g = torch.Generator().manual_seed(1)
    xyz = surface(P, 1).to(dev)
    views = []
    for v in range(args.views):
        ids = torch.randint(0, P, (args.records,), generator=g, dtype=torch.int32)
        n = xyz.cpu()[ids.long()] + 0.3 * torch.randn(args.records, 3, generator=g)
        n = n / n.norm(dim=1, keepdim=True)
        conf = 0.5 + 0.5 * torch.rand(args.records, generator=g)
        a = 2 * math.pi * v / args.views
        views.append((ids.to(dev), n.to(dev), conf.to(dev), [3 * math.cos(a), 0.3, 3 * math.sin(a)]))
    fusion = pcd_fusion.NormalFusion(xyz)

    def add_all():
        fusion.num_records = 0
        for ids, n, conf, t in views:
            fusion.add_view(ids, n, conf, t)

    res["fusion_add_views_ms"] = gpu_time(add_all, args.repeat)
    res["fusion_finalize_ms"] = gpu_time(lambda: fusion.finalize(), args.repeat)
    uids, fused = fusion.finalize()
    print(f"fusion {args.views} views x {args.records} records over {P} Gaussians -> {len(uids)} fused points: "
          f"add_view total {res['fusion_add_views_ms']:.1f} ms, finalize {res['fusion_finalize_ms']:.1f} ms", flush=True)
    if not args.no_cpu:
        cv = [(i.cpu().numpy(), n.cpu().numpy(), c.cpu().numpy(), np.array(t)) for i, n, c, t in views[:10]]
        ms = cpu_time(lambda: model.normal_fusion(xyz.cpu().numpy(), *[list(x) for x in zip(*cv)]))
        res["fusion_cpu_model_10_views_ms"] = ms
        print(f"  CPU model, first 10 views only: {ms:.0f} ms", flush=True)

    cp = surface(1_000_000, 2)
    cp = cp + 0.002 * torch.randn(cp.shape, generator=g)
    cn = cp / cp.norm(dim=1, keepdim=True)
    cp_dev, cn_dev = cp.to(dev), cn.to(dev)
    res["clean_1M_ms"] = gpu_time(lambda: pcd_fusion.clean_point_cloud(cp_dev, cn_dev), args.repeat)
    line = f"cleaning 1 M points (k 50 statistical + k 20 normal): GPU {res['clean_1M_ms']:.2f} ms"
    if not args.no_cpu:
        res["clean_1M_cpu_ms"] = cpu_time(lambda: model.clean_point_cloud(cp.numpy(), cn.numpy()))
        line += f", CPU model {res['clean_1M_cpu_ms']:.0f} ms"
    print(line, flush=True)
    print(json.dumps({k: round(v, 3) for k, v in res.items()}))


if __name__ == "__main__":
    main()
