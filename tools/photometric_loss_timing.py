#!/usr/bin/env python
"""Times gaustudio_amd.losses.photometric_loss on an MI355X beside a torch restatement of the same formula (five depthwise
F.conv2d and autograd) on the same GPU in the same process, and writes profiles/photometric_loss_timing.json.

Cases: forward (with the maps a backward needs), forward + backward and no_grad, at 400 x 400, 1080p and 4K with 3 planes
and at 1080p with 8 x 3 planes.  A figure is the median of 7 timed windows (device events around `inner` calls, after a
warm-up of both paths at that shape), HIP and torch windows alternating, with the min-max spread; peak memory is the
allocator's high-water mark above what was allocated before the call.  No GPU: it fails, it does not fall back.

    python tools/photometric_loss_timing.py [--out FILE] [--windows 7] [--only 1080p_x3,4k_x3]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gaustudio_amd import losses  # noqa: E402

SHAPES = {"400x400x3": (3, 400, 400), "1080p_x3": (3, 1080, 1920), "4k_x3": (3, 2160, 3840), "1080p_8x3": (8, 3, 1080, 1920)}


def torch_loss(image, target, window, lam=0.2):
    H, W = image.shape[-2:]
    x, y = image.reshape(1, -1, H, W), target.reshape(1, -1, H, W)
    P = x.shape[1]
    w = window.expand(P, 1, 11, 11)
    cv = lambda v: F.conv2d(v, w, padding=5, groups=P)
    mu1, mu2 = cv(x), cv(y)
    mu1sq, mu2sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = cv(x * x) - mu1sq, cv(y * y) - mu2sq, cv(x * y) - mu12
    smap = ((2 * mu12 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1sq + mu2sq + 1e-4) * (s1 + s2 + 9e-4))
    return (1.0 - lam) * (x - y).abs().mean() + lam * (1.0 - smap.mean())


def make_step(fn, mode, image):
    def fwd():
        return fn()

    def fwd_bwd():
        image.grad = None
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


def peak_bytes(step):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric_loss_timing.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--only", default=None, help="comma-separated shape names (default: all of " + ", ".join(SHAPES) + ")")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("photometric_loss_timing needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    import loss_model
    g = torch.from_numpy(loss_model.WINDOW).to(dev)
    window = (g[:, None] * g[None, :]).reshape(1, 1, 11, 11)
    cases = {}
    for sname, shape in SHAPES.items():
        if args.only and sname not in args.only.split(","):
            continue
        gen = torch.Generator().manual_seed(0)
        image = torch.rand(shape, generator=gen).to(dev).requires_grad_(True)
        target = torch.rand(shape, generator=gen).to(dev)
        hip = lambda: losses.photometric_loss(image, target)
        ref = lambda: torch_loss(image, target, window)
        with torch.no_grad():
            agree = abs(float(hip()) - float(ref()))
        n = image.numel()
        inner = max(2, min(50, int(2e8 // n)))          # a window of tens of milliseconds or more of torch work
        for mode in ("forward", "forward_backward", "no_grad"):
            steps = {"hip": make_step(hip, mode, image), "torch": make_step(ref, mode, image)}
            for s in steps.values():                    # warm-up at this shape: code objects, algorithm choice, allocator
                for _ in range(3):
                    s()
            torch.cuda.synchronize()
            ms = {"hip": [], "torch": []}
            for _ in range(args.windows):               # alternating
                for k, s in steps.items():
                    ms[k].append(window_ms(s, inner * (8 if k == "hip" else 1)))   # the shorter call gets more of them
            rec = {"calls_per_window": {"hip": 8 * inner, "torch": inner},"windows": args.windows, "abs_loss_difference_hip_torch": agree}
            for k in ("hip", "torch"):
                rec[k] = {"median_ms": statistics.median(ms[k]), "min_ms": min(ms[k]), "max_ms": max(ms[k]),
                          "peak_bytes": peak_bytes(steps[k])}
            rec["torch_over_hip_median"] = rec["torch"]["median_ms"] / rec["hip"]["median_ms"]
            cases[f"{sname}/{mode}"] = rec
            print(f"{sname:10s} {mode:17s} hip {rec['hip']['median_ms']:8.4f} ms [{rec['hip']['min_ms']:.4f}, {rec['hip']['max_ms']:.4f}]"
                  f"  torch {rec['torch']['median_ms']:8.4f} ms [{rec['torch']['min_ms']:.4f}, {rec['torch']['max_ms']:.4f}]"
                  f"  peak {rec['hip']['peak_bytes'] >> 20} / {rec['torch']['peak_bytes'] >> 20} MiB", flush=True)
        del image, target
        torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "what": "photometric_loss (lambda 0.2): call time from device events, median of the windows with min and max; "
                   "torch = the same formula with five depthwise F.conv2d and autograd, float32, same GPU, same process",
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
