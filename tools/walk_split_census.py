#!/usr/bin/env python
"""Census for the wave-uniform phase splits of the two composite walks (DESIGN s4.3 / s4.4), on the CPU oracle's forward.

(a) composite_fwd_quarter: the median bookkeeping of a step (compare, two selects) is dead once no lane of the wave is both
    live and above T = 0.5.  The walk tests that at every group of four steps and switches, for the rest of the tile, to a
    copy of the step without it.  Counted: wave-groups walked in total, and those walked after the switch.  A lane's T
    drops to 0.5 or below with its median candidate (the oracle's median id); it is done at its stop entry (the first valid
    entry after its last contributor).  Batches of 256, per-quarter lists from the kernels' conservative block test, the
    walk's own exits (a batch is skipped once the whole workgroup is done, a wave leaves its walk at a multiple of 32
    steps once all of its lanes are done).
(b) composite_bwd_quarter: `pos < lc` is true for every entry of a 128-instance round when top <= min over the wave's lanes
    of lc (lc = 0 outside the image).  Counted: wave-steps in such rounds, out of all (groups of 4, as the kernel walks).

TOOL, not product: imports the test-only oracle.  usage: python tools/walk_split_census.py --workload C3 [--tiles 200]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gaustudio_amd import scenes  # noqa: E402
from quarter_balance_census import box_test  # noqa: E402

FWD_BATCH, BWD_BATCH, U = 256, 128, 4


def workload(name):
    sizes = {"C2": (300_000, 800, 800), "C3": (1_000_000, 1920, 1080), "C4": (5_000_000, 1297, 840), "C5": (2_500_000, 3840, 2160)}
    P, W, H = sizes[name]
    cam = scenes.make_camera(W, H)
    return scenes.make_scene(P, cam, seed=0), cam


def forward_state(sc, cam):
    from oracle import pyoracle as po
    from util import oracle_forward, scene_kwargs
    st = oracle_forward(po, sc, cam, 3, scene_kwargs(sc, True, False), tight=True)
    keys = ("ranges", "point_list", "means2D", "conic_opacity", "n_contrib", "median")
    return {k: torch.from_numpy(np.ascontiguousarray(st[k]).astype(np.int64 if st[k].dtype.kind in "ui" else np.float32)) for k in keys}


def census_tile(t, st, W, H, gx):
    r, pl, xy, co = st["ranges"], st["point_list"], st["means2D"], st["conic_opacity"]
    ids = pl[int(r[t, 0]):int(r[t, 1])]
    L = ids.numel()
    tx, ty = t % gx, t // gx
    # per pixel of the tile (row-major 16x16): coordinates, inside, n_contrib, median id
    yy, xx = torch.meshgrid(torch.arange(16), torch.arange(16), indexing="ij")
    px, py = (tx * 16 + xx).flatten(), (ty * 16 + yy).flatten()
    inside = (px < W) & (py < H)
    pxc, pyc = px.clamp(max=W - 1), py.clamp(max=H - 1)
    nc = torch.where(inside, st["n_contrib"][pyc, pxc], torch.zeros_like(px))
    med_w, med_id = st["median"][1][pyc, pxc], st["median"][2][pyc, pxc]
    # quarter masks [16 blocks][L] and each pixel's block
    qm = torch.zeros(16, L, dtype=torch.bool)
    for b in range(16):
        bx0, by0 = tx * 16 + 4 * (b & 3), ty * 16 + 4 * (b >> 2)
        if bx0 < W and by0 < H:
            qm[b] = box_test(xy[ids], co[ids], bx0, by0, min(bx0 + 3, W - 1), min(by0 + 3, H - 1))
    blk = (yy.flatten() // 4) * 4 + xx.flatten() // 4
    wave = (yy.flatten() // 8) * 2 + xx.flatten() // 8
    # per pixel: list position that brings T to 0.5 or below (the median candidate), and of the stop entry
    INF = 1 << 30
    pos_of = {int(g): i for i, g in enumerate(ids.tolist())}
    pm = torch.full((256,), INF, dtype=torch.long)
    for p in range(256):
        if inside[p] and (med_w[p] > 0 or med_id[p] > 0):
            pm[p] = pos_of.get(int(med_id[p]), INF)
    g = xy[ids]
    dx = g[None, :, 0] - px[:, None].float()
    dy = g[None, :, 1] - py[:, None].float()
    c = co[ids]
    power = -0.5 * (c[None, :, 0] * dx * dx + c[None, :, 2] * dy * dy) - c[None, :, 1] * dx * dy
    alpha = torch.clamp_max(c[None, :, 3] * torch.exp(power), 0.99)
    valid = (power <= 0) & (alpha >= 1.0 / 255.0)
    after = torch.arange(L)[None, :] >= nc[:, None]
    cand = valid & after
    ps = torch.where(cand.any(1), cand.float().argmax(1), torch.full((256,), INF)).long()
    ps = torch.where(inside, ps, torch.full_like(ps, -1))              # outside: done from the start
    # (a) forward walk, batch by batch
    fwd_total = fwd_after = 0
    med_live = [True] * 4
    for base in range(0, L, FWD_BATCH):
        if bool((ps < base).all()):
            break                                                       # __syncthreads_and(done)
        cnt = min(FWD_BATCH, L - base)
        rank = torch.full((16, cnt), -1, dtype=torch.long)
        n_q = torch.zeros(16, dtype=torch.long)
        for b in range(16):
            hit = qm[b, base:base + cnt]
            rank[b, hit] = torch.arange(int(hit.sum()))
            n_q[b] = hit.sum()
        for w in range(4):
            lanes = torch.nonzero(wave == w).flatten()
            n = int(max(n_q[blk[lanes]].tolist()))
            ngroups = (n + U - 1) // U

            def steps_until(pos):                                       # per lane: steps of this batch walked before `pos` is behind
                out = []
                for p, x in zip(lanes.tolist(), pos[lanes].tolist()):
                    if x < base:
                        out.append(0)
                    elif x >= base + cnt:
                        out.append(INF)
                    else:
                        out.append(int(rank[blk[p], x - base]) + 1)
                return torch.tensor(out)
            s_stop = steps_until(ps)
            sat = int(s_stop.max())                                     # every lane of the wave done after this many steps
            if sat == 0:
                continue                                                # the wave's walk of this batch ends at once
            med = int(torch.minimum(steps_until(pm), s_stop).max()) if med_live[w] else 0
            if med >= INF:
                fwd_total += ngroups                                    # the whole batch in the median phase
                continue
            g_med = min(ngroups, (med + U - 1) // U)
            if g_med == ngroups:
                fwd_total += ngroups
                continue
            med_live[w] = False
            # the second phase leaves at the first multiple of 8 groups at which the wave has saturated
            g_end = ngroups if sat >= INF else min(ngroups, max(g_med, ((sat + U - 1) // U + 7) // 8 * 8))
            if sat <= U * g_med:
                g_end = g_med
            fwd_total += g_end
            fwd_after += g_end - g_med
    # (b) backward rounds, back to front from the tile's deepest last contributor
    bwd_total = bwd_clean = 0
    bmax = int(min(int(nc.max()), L))
    qmax = torch.zeros(16, dtype=torch.long)
    for b in range(16):
        qmax[b] = int(nc[blk == b].max())
    pos = torch.arange(L)
    for top in range(bmax, 0, -BWD_BATCH):
        lo = max(0, top - BWD_BATCH)
        for w in range(4):
            lanes = wave == w
            qs = sorted(set(blk[lanes].tolist()))
            n = max(int((qm[b, lo:top] & (pos[lo:top] < qmax[b])).sum()) for b in qs)
            s = (n + U - 1) // U * U
            bwd_total += s
            if top <= int(nc[lanes].min()):
                bwd_clean += s
    return fwd_total, fwd_after, bwd_total, bwd_clean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C3")
    ap.add_argument("--tiles", type=int, default=200)
    a = ap.parse_args()
    sc, cam = workload(a.workload)
    W, H = cam.width, cam.height
    st = forward_state(sc, cam)
    gx = (W + 15) // 16
    r = st["ranges"]
    cand = torch.nonzero((r[:, 1] - r[:, 0]) > 0).flatten()
    g = torch.Generator().manual_seed(0)
    tiles = cand[torch.randperm(cand.numel(), generator=g)[:a.tiles]]
    tot = np.zeros(4, np.int64)
    per_tile = []
    for t in tiles.tolist():
        v = census_tile(t, st, W, H, gx)
        tot += v
        if v[0]:
            per_tile.append(v[1] / v[0])
    q = np.percentile(per_tile, [10, 50, 90]) if per_tile else [0, 0, 0]
    print(f"{a.workload}: {len(tiles)} tiles")
    print(f"  (a) fwd  wave-groups walked {tot[0]:8d}, after the median switch {tot[1]:8d} = {tot[1] / max(tot[0], 1):.3f}"
          f"   (per tile p10/p50/p90 {q[0]:.3f}/{q[1]:.3f}/{q[2]:.3f})")
    print(f"  (b) bwd  wave-steps walked  {tot[2]:8d}, in rounds with top <= min lc {tot[3]:8d} = {tot[3] / max(tot[2], 1):.3f}")


if __name__ == "__main__":
    main()
