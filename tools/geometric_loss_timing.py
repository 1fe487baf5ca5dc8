#!/usr/bin/env python
"""Times gaustudio_amd.surfel_losses.surfel_geometric_loss on an MI355X beside a torch restatement of the same formula (the
post-render block of the surfel renderer, the published depth_to_normal and the two loss terms, with autograd) on the same GPU
in the same process, and writes profiles/geometric_loss_timing.json.

Cases: forward, forward + backward and no_grad, at 400 x 400, 1080p and 4K.  A figure is the median of 7 timed windows (device
events around `inner` calls, after a warm-up of both paths at that shape), HIP and torch windows alternating, with the min-max
spread; peak memory is the allocator's high-water mark above what was allocated before the call.  No GPU: it fails, it does
not fall back.

    python tools/geometric_loss_timing.py [--out FILE] [--windows 7] [--only 1080p,4k]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaustudio_amd import surfel_losses  # noqa: E402

SHAPES = {"400x400": (400, 400), "1080p": (1080, 1920), "4k": (2160, 3840)}
LAMBDA_NORMAL, LAMBDA_DIST, DEPTH_RATIO = 0.05, 100.0, 0.5


def torch_loss(a, intr, ln=LAMBDA_NORMAL, ld=LAMBDA_DIST, rho=DEPTH_RATIO):
    fx, fy, cx, cy = intr
    H, W = a.shape[1:]
    alpha = a[1]
    d_med = torch.nan_to_num(a[5], 0, 0, 0)
    d_exp = torch.nan_to_num(a[0] / alpha, 0, 0, 0)
    d = (1.0 - rho) * d_exp + rho * d_med
    ys, xs = torch.meshgrid(torch.arange(H, dtype=a.dtype, device=a.device), torch.arange(W, dtype=a.dtype, device=a.device),
                            indexing="ij")
    pts = torch.stack([d * ((xs - cx) / fx), d * ((ys - cy) / fy), d], -1)
    n = torch.zeros_like(pts)
    dy = pts[2:, 1:-1] - pts[:-2, 1:-1]
    dx = pts[1:-1, 2:] - pts[1:-1, :-2]
    n[1:-1, 1:-1] = F.normalize(torch.cross(dy, dx, dim=-1), dim=-1)
    ns = n.permute(2, 0, 1) * alpha.detach()
    return ln * (1.0 - (a[2:5] * ns).sum(0)).mean() + ld * a[6].mean()


def make_allmap(H, W, dev):
    """A wavy depth surface with alpha in (0.2, 1], noisy unit normals, and a fifth of the pixels uncovered (alpha 0)."""
    gen = torch.Generator().manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    d = 4.0 + 0.5 * torch.sin(xs * 0.01) * torch.cos(ys * 0.013)
    alpha = 1.0 - 0.8 * torch.rand(H, W, generator=gen)
    alpha[torch.rand(H, W, generator=gen) < 0.2] = 0.0
    nrm = F.normalize(torch.tensor([0.0, 0.0, -1.0]).view(3, 1, 1) + 0.2 * torch.randn(3, H, W, generator=gen), dim=0)
    a = torch.stack([d * alpha, alpha, nrm[0], nrm[1], nrm[2], d * (alpha > 0), 0.01 * torch.rand(H, W, generator=gen)])
    return a.to(dev).requires_grad_(True)


def make_step(fn, mode, leaf):
    def fwd():
        return fn()

    def fwd_bwd():
        leaf.grad = None
        fn().backward()

    def no_grad():
        with torch.no_grad():
            return fn()
    return {"forward": fwd, "forward_backward": fwd_bwd, "no_grad": no_grad}[mode]


def window_ms(step, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def peak_bytes(step, leaf):
    leaf.grad = None                                # (or forward_backward would reuse the block of the gradient it drops)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometric_loss_timing.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--only", default=None, help="comma-separated shape names (default: all of " + ", ".join(SHAPES) + ")")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geometric_loss_timing needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    cases = {}
    for sname, (H, W) in SHAPES.items():
        if args.only and sname not in args.only.split(","):
            continue
        allmap = make_allmap(H, W, dev)
        f = W / (2.0 * math.tan(math.radians(30.0)))
        intr = (f, f, (W - 1) / 2.0, (H - 1) / 2.0)
        hip = lambda: surfel_losses.surfel_geometric_loss(allmap, intr, LAMBDA_NORMAL, LAMBDA_DIST, DEPTH_RATIO)
        ref = lambda: torch_loss(allmap, intr)
        with torch.no_grad():
            agree = abs(float(hip()) - float(ref()))
        inner = max(2, min(50, int(1e8 // (H * W))))      # a window of tens of milliseconds or more of torch work
        for mode in ("forward", "forward_backward", "no_grad"):
            steps = {"hip": make_step(hip, mode, allmap), "torch": make_step(ref, mode, allmap)}
            for s in steps.values():                    # warm-up at this shape: code objects, allocator
                for _ in range(3):
                    s()
            torch.cuda.synchronize()
            ms = {"hip": [], "torch": []}
            for _ in range(args.windows):               # alternating
                for k, s in steps.items():
                    ms[k].append(window_ms(s, inner * (8 if k == "hip" else 1)))   # the shorter call gets more of them
            rec = {"calls_per_window": {"hip": 8 * inner, "torch": inner}, "windows": args.windows,
                   "abs_loss_difference_hip_torch": agree}
            for k in ("hip", "torch"):
                rec[k] = {"median_ms": statistics.median(ms[k]), "min_ms": min(ms[k]), "max_ms": max(ms[k]),
                          "peak_bytes": peak_bytes(steps[k], allmap)}
            rec["torch_over_hip_median"] = rec["torch"]["median_ms"] / rec["hip"]["median_ms"]
            cases[f"{sname}/{mode}"] = rec
            print(f"{sname:8s} {mode:17s} hip {rec['hip']['median_ms']:8.4f} ms [{rec['hip']['min_ms']:.4f}, {rec['hip']['max_ms']:.4f}]"
                  f"  torch {rec['torch']['median_ms']:8.4f} ms [{rec['torch']['min_ms']:.4f}, {rec['torch']['max_ms']:.4f}]"
                  f"  peak {rec['hip']['peak_bytes'] >> 20} / {rec['torch']['peak_bytes'] >> 20} MiB", flush=True)
        del allmap
        torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "what": "surfel_geometric_loss (lambda_normal 0.05, lambda_dist 100, depth_ratio 0.5) on allmap [7,H,W]: call time from "
                   "device events, median of the windows with min and max; torch = the same formula in about 25 torch ops with "
                   "autograd, float32, same GPU, same process.  forward_backward includes the [7,H,W] gradient.",
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
