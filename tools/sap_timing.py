#!/usr/bin/env python
"""Stage times of gaustudio_amd.sap on the GPU, next to a plain-torch composition of the same stages on the same GPU
(index_add_ for the scatter, torch.fft, broadcast arithmetic for the spectral solve, advanced indexing for the gather;
written for this comparison).  The torch side stops at the grid: torch has no marching cubes.  The backward stages
(`*_bwd`, `dpsr_fwd_bwd`, `psr2mesh_bwd`) are timed the same way, the torch side through torch autograd of that composition
(the reference's formulation: index_add_ / advanced indexing and their autograd adjoints).

    python tools/sap_timing.py [--res 128 256] [--points 100000 1000000] [--repeats 20] [--out sap_timing_out]

Every figure is the median over `repeats` of a host clock around work that ends in a device synchronise, after 3 warm-up
calls of the same shape.  Prints one table per (res, N) and writes them to <out>/sap_timing.json (the run quoted in README
is kept as profiles/sap_timing.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import sap  # noqa: E402


def cloud(n, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    axes = torch.tensor([1.0, 0.7, 0.5])
    p = u * axes + 0.01 * torch.randn(n, 3, generator=g)
    nrm = torch.nn.functional.normalize(u / axes, dim=1)
    c = p.mean(0)
    s = (p - c).abs().max() * 1.2
    return (((p - c) / s + 1) / 2).to(dev).contiguous(), nrm.to(dev).contiguous()


def timed(fn, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out


# ---- the plain-torch composition -----------------------------------------------------------------------------------
def torch_corners(pts, R):
    q = pts * R
    i0 = q.floor()
    fr = q - i0
    i0 = i0.long()
    i1 = (i0 + 1) % R
    idx, w = [], []
    for c in range(8):
        k = (c >> 2, (c >> 1) & 1, c & 1)
        ii = [(i1 if k[d] else i0)[:, d] for d in range(3)]
        ww = [(fr if k[d] else 1 - fr)[:, d] for d in range(3)]
        idx.append((ii[0] * R + ii[1]) * R + ii[2])
        w.append(ww[0] * ww[1] * ww[2])
    return torch.stack(idx, 1), torch.stack(w, 1)


def torch_rasterize(pts, vals, R):
    idx, w = torch_corners(pts, R)
    out = torch.zeros((vals.shape[1], R * R * R), device=pts.device)
    out.index_add_(1, idx.reshape(-1), (w[:, :, None] * vals[:, None, :]).reshape(-1, vals.shape[1]).t().contiguous())
    return out.reshape(-1, R, R, R)


def torch_spectral(spec, R, sig):
    k = torch.fft.fftfreq(R, d=1.0 / R, device=spec.device)
    kr = torch.fft.rfftfreq(R, d=1.0 / R, device=spec.device)
    K = torch.stack(torch.meshgrid(k, k, kr, indexing="ij"))
    G = torch.exp(-0.5 * (sig * 2 * K.double().pow(2).sum(0).sqrt() / R) ** 2).float()
    om = K * (2 * np.pi)
    div = (torch.complex(spec.imag, -spec.real) * G * om).sum(0)
    Phi = div / (-(om * om).sum(0) + 1e-6)
    Phi[0, 0, 0] = 0
    return Phi


def torch_interp(grid, pts):
    idx, w = torch_corners(pts, grid.shape[0])
    return (grid.reshape(-1)[idx] * w).sum(1)


def torch_normalize(phi, fv):
    phi = phi - fv.mean()
    return torch.tanh(-phi / phi[0, 0, 0].detach().abs() * 0.5)        # the reference detaches |v0|


# ---- backward timing -------------------------------------------------------------------------------------------------
def leaf(t):
    return t.detach().clone().requires_grad_(True)


def backward_ms(fn, inputs, repeats):
    """median time of the backward of fn(*inputs) alone: the graph is built once and retained."""
    leaves = [leaf(t) for t in inputs]
    out = fn(*leaves)
    g = torch.randn_like(out)
    return timed(lambda: torch.autograd.grad(out, leaves, g, retain_graph=True), repeats)[0]


def hip_step(dpsr, V, N, W):
    p, v = leaf(V), leaf(N)
    (dpsr(p, v, apply_tanh=True) * W).sum().backward()
    return p.grad, v.grad


def torch_step(V, N, R, W):
    p, v = leaf(V), leaf(N)
    res = (R, R, R)
    ph = torch.fft.irfftn(torch_spectral(torch.fft.rfftn(torch_rasterize(p, v, R), dim=(1, 2, 3)), R, 2.0), s=res, dim=(0, 1, 2))
    (torch_normalize(ph, torch_interp(ph, p)) * W).sum().backward()
    return p.grad, v.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--points", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default="sap_timing_out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sap_timing.py measures on a ROCm GPU; none is visible")
    dev = torch.device("cuda", 0)
    os.makedirs(args.out, exist_ok=True)
    rows = []

    def bwd(fn, *inputs):
        return backward_ms(fn, inputs, args.repeats)

    for R in args.res:
        for n in args.points:
            V, N = cloud(n, dev)
            res = (R, R, R)
            hip, tor = {}, {}
            hip["rasterize"], ras = timed(lambda: sap.point_rasterize(V, N, res, weighted=False), args.repeats)
            tor["rasterize"], tras = timed(lambda: torch_rasterize(V, N, R), args.repeats)
            hip["rfftn"], spec = timed(lambda: torch.fft.rfftn(ras, dim=(1, 2, 3)), args.repeats)
            tor["rfftn"] = hip["rfftn"]
            hip["spectral"], Phi = timed(lambda: sap.spectral_solve(spec, res, 2.0), args.repeats)
            tor["spectral"], _ = timed(lambda: torch_spectral(spec, R, 2.0), args.repeats)
            hip["irfftn"], phi = timed(lambda: torch.fft.irfftn(Phi, s=res, dim=(0, 1, 2)), args.repeats)
            tor["irfftn"] = hip["irfftn"]
            hip["interp"], (fv, mean) = timed(lambda: sap.grid_interp(phi, V, return_mean=True), args.repeats)
            tor["interp"], tfv = timed(lambda: torch_interp(phi, V), args.repeats)
            hip["normalize"], grid = timed(lambda: sap.normalize_grid(phi, mean, scale=True, apply_tanh=True), args.repeats)
            tor["normalize"], tgrid = timed(lambda: torch_normalize(phi, tfv), args.repeats)
            hip["marching_cubes"], (v, f) = timed(lambda: sap.marching_cubes(grid, 0.0), args.repeats)
            dpsr = sap.DPSR(res, sig=2)
            hip["dpsr_total"], _ = timed(lambda: dpsr(V, N, apply_tanh=True), args.repeats)
            tor["dpsr_total"], _ = timed(lambda: torch_normalize(*(lambda p: (p, torch_interp(p, V)))(torch.fft.irfftn(
                torch_spectral(torch.fft.rfftn(torch_rasterize(V, N, R), dim=(1, 2, 3)), R, 2.0), s=res, dim=(0, 1, 2)))), args.repeats)
            # ---- backward: each stage's backward alone (a retained graph), then the solver forward + backward
            hip["rasterize_bwd"] = bwd(lambda p, v: sap.point_rasterize(p, v, res, weighted=False), V, N)
            tor["rasterize_bwd"] = bwd(lambda p, v: torch_rasterize(p, v, R), V, N)
            hip["spectral_bwd"] = bwd(lambda x: torch.view_as_real(sap.spectral_solve(x, res, 2.0)), spec)
            tor["spectral_bwd"] = bwd(lambda x: torch.view_as_real(torch_spectral(x, R, 2.0)), spec)
            hip["interp_bwd"] = bwd(lambda g, p: sap.grid_interp(g, p), phi, V)
            tor["interp_bwd"] = bwd(lambda g, p: torch_interp(g, p), phi, V)
            hip["normalize_bwd"] = bwd(lambda g, m: sap.normalize_grid(g, m, scale=True, apply_tanh=True), phi, mean)
            tor["normalize_bwd"] = bwd(lambda g, f: torch_normalize(g, f), phi, tfv)
            hip["psr2mesh_bwd"] = bwd(lambda g: sap.psr2mesh(g)[0], grid)
            W = torch.randn(res, device=dev)

            hip["dpsr_fwd_bwd"], (gp, gv) = timed(lambda: hip_step(dpsr, V, N, W), args.repeats)
            tor["dpsr_fwd_bwd"], (tgp, tgv) = timed(lambda: torch_step(V, N, R, W), args.repeats)
            # a coordinate exactly on a node (p * R an integer; a few per 10^5 float32 points when R is a power of two) is where
            # the two formulations differ by design: |p - pos| has derivative sign(0) = 0 there, the composition's 1 - fr has -R
            off_node = ((V * R) != (V * R).floor()).all(1)
            grad_agree = dict(points=float((gp - tgp)[off_node].abs().max() / tgp.abs().max()),
                              normals=float((gv - tgv).abs().max() / tgv.abs().max()), node_aligned_points=int((~off_node).sum()))
            agree = float((grid - tgrid).abs().max())
            row = dict(res=R, points=n, hip_ms=hip, torch_ms=tor, vertices=len(v), faces=len(f), max_abs_grid_diff=agree,
                       max_rel_grad_diff=grad_agree)
            rows.append(row)
            print(f"res {R}^3, N = {n}: {len(v)} vertices, {len(f)} faces; max |hip grid - torch grid| = {agree:.2e}; "
                  f"max relative gradient difference: points {grad_agree['points']:.2e} "
                  f"(off the {grad_agree['node_aligned_points']} node-aligned points), normals {grad_agree['normals']:.2e}")
            for k in hip:
                print(f"  {k:15s} hip {hip[k]:9.3f} ms   torch {tor[k]:9.3f} ms" if k in tor else f"  {k:15s} hip {hip[k]:9.3f} ms")
            with open(os.path.join(args.out, "sap_timing.json"), "w") as fjson:
                json.dump(rows, fjson, indent=1)


if __name__ == "__main__":
    main()
