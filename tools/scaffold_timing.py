#!/usr/bin/env python
"""Times of gaustudio_amd.scaffold.decode against its torch restatement -> profiles/scaffold_timing.json.

  * decode's two passes (count: filter-by-mask, view direction, bank, opacity MLP, scan, the 4-byte read-back; emit: covariance
    and colour MLPs, activations, compaction) and the whole call;
  * decode_torch (get_gaussians_properties in plain torch ops, under no_grad) for the SAME visible mask on the same GPU;
  * N = 1e5 and 1e6 anchors, k = 10, with and without the feature bank, about 30 % and 100 % of the anchors visible;
  * per case a `training` block: forward + backward of decode(backward="hip") against decode(backward="torch") with the same
    mask and cotangents, and the peak memory of each (see training()).

    python tools/scaffold_timing.py [--repeat 7] [--sizes 100000 1000000] [--out profiles/scaffold_timing.json]
Every figure is the median of --repeat calls after one warm-up call per variant, with the min-max spread beside it; the variants
alternate inside each repeat.  count and the totals are host clocks around a call that ends in a device synchronise (count
reads its total back, so it waits on the stream itself); emit is a pair of device events.  No threshold is set here: the file
reports, README quotes it."""
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
from gaustudio_amd import GaussianRasterizationSettings  # noqa: E402
from gaustudio_amd import scaffold as sc  # noqa: E402


def random_model(n, k, bank, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s, sc_=1.0: (torch.randn(*s, generator=g) * sc_).to(dev)
    lin = lambda n_in, n_out: (r(32, n_in, sc_=0.3), r(32, sc_=0.1), r(n_out, 32, sc_=0.3), r(n_out, sc_=0.1))
    anchor = torch.nn.functional.normalize(r(n, 3)) * 3.0
    return sc.ScaffoldModel(anchor, r(n, 32), r(n, k, 3, sc_=0.5), torch.exp(r(n, 6, sc_=0.3) - 3.0), torch.nn.functional.normalize(r(n, 4)),
                            lin(36, k), lin(36, 7 * k), lin(36, 3 * k), lin(4, 3) if bank else None)


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


def summary(xs):
    return dict(median_ms=round(statistics.median(xs), 4), min_ms=round(min(xs), 4), max_ms=round(max(xs), 4))


OUTS = ("xyz", "colors", "opacity", "scales", "rotations")


def training(model, view, mask, repeat):
    """Forward + backward of decode(backward="hip") against decode(backward="torch") (decode_torch under autograd: what trains a
    model without the HIP backward): every tensor of the model but rot requires grad, the same visible mask, the same seeded
    cotangents of the five outputs when both paths keep the same number of Gaussians (otherwise each path gets its own, and
    `same_cotangents` says so).  Per path: median (min, max) of `repeat` calls after one warm-up, alternated, host clocks around
    a call that ends in a device synchronise; peak_mib = torch.cuda.max_memory_allocated over one call minus what was
    allocated before it."""
    leaves = [t for name, t in model.tensors().items() if name != "rot"]
    for t in leaves:
        t.requires_grad_(True)
    dev = model.anchor.device
    cots = {}

    def cot(m):
        if m not in cots:
            g = torch.Generator(device="cpu").manual_seed(11)
            cots[m] = [torch.randn(m, c, generator=g).to(dev) for c in (3, 3, 1, 3, 4)]
        return cots[m]

    def step(path):
        for t in leaves:
            t.grad = None
        g = sc.decode(model, view, mask, backward=path)
        torch.autograd.backward([getattr(g, n) for n in OUTS], cot(g.xyz.shape[0]))
        return int(g.xyz.shape[0])

    ts, peak, rows = dict(hip=[], torch=[]), {}, {}
    for path in ts:
        rows[path] = step(path)                                   # warm-up (and the cotangents)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step(path)
        torch.cuda.synchronize()
        peak[path] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    for _ in range(repeat):
        for path in ts:
            ts[path].append(wall(lambda: step(path))[0])
    for t in leaves:
        t.grad = None
        t.requires_grad_(False)
    out = dict(gaussians=rows, same_cotangents=rows["hip"] == rows["torch"],
               hip=dict(summary(ts["hip"]), peak_mib=peak["hip"]), torch=dict(summary(ts["torch"]), peak_mib=peak["torch"]))
    out["torch_over_hip"] = round(out["torch"]["median_ms"] / out["hip"]["median_ms"], 3)
    spreads = (out["hip"]["max_ms"] - out["hip"]["min_ms"]) + (out["torch"]["max_ms"] - out["torch"]["min_ms"])
    out["hip_below_torch_by_more_than_both_spreads"] = bool(out["torch"]["median_ms"] - out["hip"]["median_ms"] > spreads)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scaffold_timing.json"))
    args = ap.parse_args()
    if args.repeat < 5:
        ap.error("--repeat must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("scaffold_timing needs a ROCm GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    k = 10
    eye = torch.eye(4, device=dev)
    view = GaussianRasterizationSettings(480, 640, 0.5, 0.4, torch.zeros(3, device=dev), 1.0, eye, eye, 1,
                                         torch.tensor([0.0, 0.0, -8.0], device=dev), False, False)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeat, n_offsets=k,
               protocol="median (min, max) of the repeats after one warm-up per variant; variants alternated inside each repeat; "
                        "the same visible mask for decode and decode_torch", cases=[])
    for n in args.sizes:
        for bank in (False, True):
            model = random_model(n, k, bank, dev, seed=n % 1000 + bank)
            for frac in (0.3, 1.0):
                mask = torch.from_numpy(np.random.default_rng(7).uniform(size=n) < frac).to(dev)
                with torch.no_grad():
                    g = sc.decode(model, view, mask)                     # warm-ups
                    t = sc.decode_torch(model, view, mask)
                    ts = dict(count=[], emit=[], decode=[], decode_torch=[])
                    for _ in range(args.repeat):
                        ms, counted = wall(lambda: sc._count(model, view, mask, "decode"))
                        ts["count"].append(ms)
                        ts["emit"].append(events(lambda: sc._emit(model, counted))[0])
                        ts["decode"].append(wall(lambda: sc.decode(model, view, mask))[0])
                        ts["decode_torch"].append(wall(lambda: sc.decode_torch(model, view, mask))[0])
                entry = dict(anchors=n, feature_bank=bank, visible_fraction=round(float(mask.float().mean()), 4),
                             gaussians=int(g.xyz.shape[0]), gaussians_torch=int(t.xyz.shape[0]),
                             max_abs_difference_of_opacity=(float((g.opacity - t.opacity).abs().max())
                                                            if g.xyz.shape[0] == t.xyz.shape[0] and g.xyz.shape[0] else None),
                             **{name: summary(v) for name, v in ts.items()})
                entry["decode_torch_over_decode"] = round(entry["decode_torch"]["median_ms"] / entry["decode"]["median_ms"], 3)
                entry["training"] = training(model, view, mask, args.repeat)
                res["cases"].append(entry)
                print(json.dumps(entry), flush=True)
                del g, t, mask
            del model
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
