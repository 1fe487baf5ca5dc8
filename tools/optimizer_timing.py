#!/usr/bin/env python
"""Times gaustudio_amd.optim on an MI355X beside torch on the same GPU in the same process, and writes
profiles/optimizer_timing.json.

  * GaussianAdam.step() dense and step(visible=) with 10 / 30 / 100 % of the rows visible (random rows, and the same fraction
    as one contiguous block of rows) against torch.optim.Adam(fused=True) and (foreach=True) over the same six tensors;
  * DensityControl.densify_and_prune with about 5 % cloned, 5 % split and 5 % pruned against the torch restatement of the
    published mask-and-cat sequence with its optimizer-state surgery (tests/optim_reference.py, float32, same GPU);
  * peak memory of both (the allocator's high-water mark above what was allocated before the call).

N = 10^5 and 10^6 rows, K = 15 (59 floats per row).  A step figure is the median of `--windows` timed windows (device events
around `inner` calls, after a warm-up), the candidates alternating, with the min-max spread.  A densification is timed call
by call on a fresh state.  At N = 10^5 the whole state (165 MB) fits the last-level cache; at 10^6 (1.65 GB) it does not.
No GPU: it fails, it does not fall back.

    python tools/optimizer_timing.py [--out FILE] [--windows 7] [--sizes 100000,1000000]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gaustudio_amd import DensityControl, GaussianAdam  # noqa: E402
from gaustudio_amd.optim import GROUPS  # noqa: E402

K = 15
LR = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=1.25e-4, opacity=5e-2, scaling=5e-3, rotation=1e-3)
CFG = dict(max_grad=2e-4, min_opacity=0.05, extent=4.0)


def tail(name):
    return dict(xyz=(3,), f_dc=(1, 3), f_rest=(K, 3), opacity=(1,), scaling=(3,), rotation=(4,))[name]


def make_params(n, dev, gen):
    return {name: torch.randn((n,) + tail(name), generator=gen, device=dev).requires_grad_(True) for name in GROUPS}


def window_ms(step, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "windows": len(ms)}


def time_steps(n, dev, windows):
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    params = make_params(n, dev, gen)
    grads = {name: 1e-3 * torch.randn(p.shape, generator=gen, device=dev) for name, p in params.items()}
    ours = GaussianAdam(params, LR)
    clones = {kind: [p.detach().clone().requires_grad_(True) for p in params.values()] for kind in ("fused", "foreach")}
    torch_opts = {kind: torch.optim.Adam([dict(params=[p], lr=LR[name]) for name, p in zip(GROUPS, ps)], eps=1e-15,
                                         **{kind: True}) for kind, ps in clones.items()}
    for p, g in zip(params.values(), grads.values()):
        p.grad = g
    for ps in clones.values():
        for p, g in zip(ps, grads.values()):
            p.grad = g
    vis = {}
    for pct in (10, 30, 100):
        r = torch.rand(n, generator=gen, device=dev)
        vis[f"random_{pct}"] = (r < pct / 100.0).to(torch.int32) * 5
        vis[f"block_{pct}"] = (torch.arange(n, device=dev) < n * pct // 100).to(torch.int32) * 5
    steps = {"hip_dense": lambda: ours.step()}
    steps.update({f"hip_visible_{k}": (lambda v=v: ours.step(visible=v)) for k, v in vis.items()})
    steps.update({f"torch_{kind}": o.step for kind, o in torch_opts.items()})
    inner = max(20, min(400, int(2e8 // n)))        # windows of a tenth of a second or more
    for s in steps.values():
        for _ in range(3):
            s()
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for _ in range(windows):
        for k, s in steps.items():
            ms[k].append(window_ms(s, inner))
    out = {k: summary(v) for k, v in ms.items()}
    out["calls_per_window"] = inner
    out["bytes_per_dense_step"] = n * (14 + 3 * K) * 4 * 7
    for k in steps:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        steps[k]()
        torch.cuda.synchronize()
        out[k]["peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
    return out


def densify_state(n, dev, seed):
    """About 5 % clone-class, 5 % split-class and 5 % below the opacity threshold (numpy, then uploaded)."""
    rng = np.random.default_rng(seed)
    cls = rng.random(n)
    scaling = np.full((n, 3), -5.0, np.float32) + rng.random((n, 3)).astype(np.float32) * 0.1
    scaling[(cls >= 0.05) & (cls < 0.10)] += 3.0
    opacity = np.full((n, 1), 2.0, np.float32)
    opacity[(cls >= 0.10) & (cls < 0.15)] = -10.0
    stats = dict(grad_accum=np.where(cls < 0.10, 1.0, 0.0).astype(np.float32), denom=np.ones(n, np.int32),
                 max_radii=rng.integers(0, 15, n).astype(np.int32))
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    params = make_params(n, dev, gen)
    params["scaling"] = torch.tensor(scaling, device=dev).requires_grad_(True)
    params["opacity"] = torch.tensor(opacity, device=dev).requires_grad_(True)
    return params, {k: torch.tensor(v, device=dev) for k, v in stats.items()}


def time_densify(n, dev, repeats):
    import optim_reference as oref
    ms = {"hip": [], "torch": []}
    peak = {}
    report = None
    for r in range(repeats + 1):                       # the first repeat warms up and is dropped
        for who in ("hip", "torch"):
            params, stats = densify_state(n, dev, seed=r)
            noise = torch.randn((n, 2, 3), device=dev)
            opt = GaussianAdam(params, LR)
            for name in GROUPS:
                opt.exp_avg[name].normal_()
                opt.exp_avg_sq[name].uniform_()
            dc = DensityControl(opt)
            dc.grad_accum.copy_(stats["grad_accum"])
            dc.denom.copy_(stats["denom"])
            dc.max_radii.copy_(stats["max_radii"])
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if who == "hip":
                report = dc.densify_and_prune(CFG["max_grad"], CFG["min_opacity"], CFG["extent"], 20, 2, noise)
            else:
                with torch.no_grad():
                    st = oref.densify_and_prune({k: v.detach() for k, v in params.items()}, opt.exp_avg, opt.exp_avg_sq,
                                                stats["grad_accum"], stats["denom"].float(), stats["max_radii"], CFG["max_grad"],
                                                CFG["min_opacity"], CFG["extent"], 20, 2, noise)
                assert st.n == report.n_after, (st.n, report)
            b.record()
            b.synchronize()
            if r:
                ms[who].append(a.elapsed_time(b))
            peak[who] = int(torch.cuda.max_memory_allocated() - base)
            del opt, dc, params, stats, noise
    out = {who: dict(summary(v), peak_bytes=peak[who]) for who, v in ms.items()}
    out["report"] = report._asdict()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_timing.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sizes", default="100000,1000000")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optimizer_timing needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    cases = {}
    for n in (int(s) for s in args.sizes.split(",")):
        cases[f"N={n}/step"] = time_steps(n, dev, args.windows)
        torch.cuda.empty_cache()
        cases[f"N={n}/densify_and_prune"] = time_densify(n, dev, args.windows)
        torch.cuda.empty_cache()
        for name, rec in cases.items():
            if name.startswith(f"N={n}/"):
                for k, v in rec.items():
                    if isinstance(v, dict) and "median_ms" in v:
                        print(f"{name:28s} {k:24s} {v['median_ms']:9.4f} ms [{v['min_ms']:.4f}, {v['max_ms']:.4f}]"
                              f"  peak {v['peak_bytes'] >> 20} MiB", flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "K": K,
           "what": "call time from device events: median of the windows with min and max.  step: GaussianAdam against "
                   "torch.optim.Adam fused / foreach over the same six tensors; visible_random_P / visible_block_P: P per cent of "
                   "the rows visible, scattered or as one block.  densify_and_prune: one call on a fresh state, about 5 % cloned, "
                   "5 % split in two, 5 % pruned, against tests/optim_reference.py in float32 on the same GPU",
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
