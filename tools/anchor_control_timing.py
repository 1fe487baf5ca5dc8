#!/usr/bin/env python
"""Times AnchorControl on the GPU it runs on and writes profiles/anchor_control_timing.json:

    accumulate, every level of adjust, the prune scan and the emit (each call between two device synchronisations), a whole
    adjust (one host clock around it, ended by a synchronise), and the torch restatement of the published sequence
    (tests/anchor_reference.py, float32 tensors on the same GPU in the same process) on the same inputs

at N = 1e5 and 1e6 anchors, k = 10, about 5 % of the offset slots candidates of level 0.  Warm-up first, then medians of
`--reps` (at least 7) with the min-max spread.    python tools/anchor_control_timing.py [--reps 7] [--sizes 100000 1000000]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import anchor_reference as aref  # noqa: E402
from gaustudio_amd import AnchorControl, anchor_control  # noqa: E402

NAMES = anchor_control.NAMES
CFG = dict(check_interval=100, success_threshold=0.8, grad_threshold=2e-4, min_opacity=0.005)
VOXEL = 0.01


def make_inputs(n, k, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    u = lambda *s: torch.rand(*s, device=dev, generator=g)
    extent = (n / 1e5) ** (1.0 / 3.0)                               # about 50 anchors per 0.16 voxel, 0.8 per 0.04 voxel
    params = dict(anchor=(u(n, 3) * 2 - 1) * extent, anchor_feat=r(n, 32), offset=r(n, k, 3),
                  scale_raw=(u(n, 6) * 0.08 + 0.02).log(), rot_raw=r(n, 4))
    denom = torch.randint(30, 100, (n * k,), device=dev, generator=g, dtype=torch.int32)
    hot = u(n * k) < 0.10                                            # the draw of level 0 halves them
    avg = torch.where(hot, u(n * k) * 1.4e-3 + 2.2e-4, u(n * k) * 1.8e-4)
    a_denom = torch.randint(0, 160, (n,), device=dev, generator=g, dtype=torch.int32)
    stats = dict(offset_grad_accum=avg * denom, offset_denom=denom, opacity_accum=u(n) * 0.1 * a_denom, anchor_denom=a_denom)
    moments = {name: (r(*p.shape), u(*p.shape)) for name, p in params.items()}
    rand = u(3, n * k)
    kept = u(n, k) < 0.4
    aidx, oidx = torch.nonzero(kept, as_tuple=True)
    m = aidx.shape[0]

    class View:
        anchor_index, offset_index = aidx.to(torch.int32), oidx.to(torch.int32)
        opacity, visible = u(m, 1), u(n) < 0.8
    return params, stats, moments, rand, (View, r(m, 3) * 1e-3, torch.randint(0, 3, (m,), device=dev, generator=g, dtype=torch.int32))


def fresh(params, stats, moments, dev):
    tp = {name: t.clone().requires_grad_(True) for name, t in params.items()}
    opt = torch.optim.Adam([dict(params=[tp[name]], lr=1e-3) for name in NAMES])
    for name in NAMES:
        opt.state[tp[name]] = dict(step=torch.tensor(10.0), exp_avg=moments[name][0].clone(), exp_avg_sq=moments[name][1].clone())
    ctl = AnchorControl(tp, VOXEL, optimizer=opt)
    for key, t in stats.items():
        getattr(ctl, key).copy_(t)
    return ctl


def spread(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), n=len(xs))


def measure(n, k, reps, dev):
    params, stats, moments, rand, view = make_inputs(n, k, dev)
    sync = lambda: torch.cuda.synchronize(dev)
    per_call, totals, reports = {}, [], []
    real_call = anchor_control.call

    def timed_call(name, *a, **kw):
        sync()
        t = time.perf_counter()
        rc = real_call(name, *a, **kw)
        sync()
        calls.append((name, (time.perf_counter() - t) * 1e3))
        return rc

    for rep in range(reps + 2):                                      # two warm-up rounds
        for timed in (False, True):
            ctl = fresh(params, stats, moments, dev)
            calls = []
            anchor_control.call = timed_call if timed else real_call
            sync()
            t = time.perf_counter()
            report = ctl.adjust(rand=rand, **CFG)
            sync()
            dt = (time.perf_counter() - t) * 1e3
            anchor_control.call = real_call
            if rep < 2:
                continue
            if timed:
                level = 0
                for name, ms in calls:
                    key = name
                    if name == "gsr_anchor_level":
                        key, level = f"level_{level}", level + 1
                    per_call.setdefault(key, []).append(ms)
            else:
                totals.append(dt)
                reports.append(report)
    acc = []
    ctl = fresh(params, stats, moments, dev)
    for rep in range(reps + 2):
        sync()
        t = time.perf_counter()
        for _ in range(20):
            ctl.accumulate(*view)
        sync()
        if rep >= 2:
            acc.append((time.perf_counter() - t) * 1e3 / 20)
    ref, ref_report = [], None
    p32 = {name: t.clone() for name, t in params.items()}
    s32 = {key: t.to(torch.float32) for key, t in stats.items()}
    for rep in range(reps + 1):                                      # one warm-up round
        sync()
        t = time.perf_counter()
        res = aref.adjust_anchor(p32, {name: m[0] for name, m in moments.items()}, {name: m[1] for name, m in moments.items()}, s32,
                                 k, VOXEL, rand, **CFG)
        sync()
        if rep >= 1:
            ref.append((time.perf_counter() - t) * 1e3)
        ref_report = (res.n_grown, int(res.prune_mask.sum()), int(res.params["anchor"].shape[0]))
        del res
    out = dict(n=n, k=k, gaussians_per_view=int(view[0].anchor_index.shape[0]), report=reports[0]._asdict(),
               same_report_every_run=all(r == reports[0] for r in reports),
               reference_report=dict(n_grown=ref_report[0], n_pruned=ref_report[1], n_after=ref_report[2]),
               accumulate=spread(acc), adjust=spread(totals), reference_adjust=spread(ref),
               calls={key: spread(v) for key, v in sorted(per_call.items())})
    out["reference_over_hip"] = out["reference_adjust"]["median_ms"] / out["adjust"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_control_timing.json"))
    args = ap.parse_args()
    assert args.reps >= 7, "medians of at least 7"
    assert torch.cuda.is_available(), "this tool measures on a ROCm GPU"
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(dev), torch=torch.__version__, k=10, config=CFG, voxel_size=VOXEL,
                  method="host clock around work ended by a device synchronise; medians of `n` with min and max; the per-call "
                         "figures come from separate runs that synchronise around every library call",
                  sizes=[])
    for n in args.sizes:
        result["sizes"].append(measure(n, 10, args.reps, dev))
        print(json.dumps(result["sizes"][-1]), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
