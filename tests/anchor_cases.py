"""Seeded inputs for the anchor-control tests (tests/test_anchor_model.py, tests/test_gpu_anchor.py): clouds whose every decision
keeps a margin from its threshold, built by rejection -- an entry that comes too close is drawn again, so no case is left out
-- and the margin itself, measured on the float64 restatement alone."""
import numpy as np
import torch

F32 = np.float32
CFG = dict(voxel_size=0.01, check_interval=100, success_threshold=0.8, grad_threshold=2e-4, min_opacity=0.005, update_depth=3,
           update_init_factor=16, update_hierarchy_factor=4)
MARGIN = 1e-3


def level_sizes(cfg=CFG):
    return [cfg["voxel_size"] * (cfg["update_init_factor"] // cfg["update_hierarchy_factor"] ** i) for i in range(cfg["update_depth"])]


def level_thresholds(cfg=CFG):
    return [cfg["grad_threshold"] * (cfg["update_hierarchy_factor"] // 2) ** i for i in range(cfg["update_depth"])]


def _half_margin(p64, sizes):
    """The distance of p / cur from the nearest half-integer, the smallest over the levels, per row."""
    worst = np.full(p64.shape[0], np.inf)
    for cur in sizes:
        q = p64 / cur
        worst = np.minimum(worst, np.abs(np.abs(q - np.floor(q)) - 0.5).min(axis=1))
    return worst


def slot_positions64(params):
    s = np.exp(params["scale_raw"][:, 0:3].astype(np.float64))
    return (params["anchor"].astype(np.float64)[:, None, :] + params["offset"].astype(np.float64) * s[:, None, :]).reshape(-1, 3)


def margin(params, stats, cfg=CFG):
    """The smallest margin of any decision, in float64 on the float32 inputs: avg against every level's threshold (relative),
    p / cur against a half-integer for every slot, every anchor and every level (absolute, in cells), the prune quantity
    against its threshold (relative)."""
    sizes = level_sizes(cfg)
    m = min(_half_margin(slot_positions64(params), sizes).min(initial=np.inf),
            _half_margin(params["anchor"].astype(np.float64), sizes).min(initial=np.inf))
    d = stats["offset_denom"].astype(np.float64)
    has = d > 0
    avg = stats["offset_grad_accum"].astype(np.float64)[has] / d[has]
    for t in level_thresholds(cfg):
        m = min(m, (np.abs(avg - t) / t).min(initial=np.inf))
    ad = stats["anchor_denom"].astype(np.float64)
    settled = ad > cfg["check_interval"] * cfg["success_threshold"]
    if cfg["min_opacity"] > 0 and settled.any():
        thr = cfg["min_opacity"] * ad[settled]
        m = min(m, (np.abs(stats["opacity_accum"].astype(np.float64)[settled] - thr) / thr).min())
    return float(m)


def make_cloud(n, k, seed, extent=1.0, cfg=CFG, hot=0.35):
    """(params, stats): n anchors in a cube of half-width `extent` (dense enough that candidate cells collide with anchors and
    with each other at the coarse levels), offsets that leave their anchor's cell, statistics on both sides of every threshold."""
    rng = np.random.default_rng(seed)
    sizes = level_sizes(cfg)
    anchor = rng.uniform(-extent, extent, (n, 3)).astype(F32)
    for _ in range(200):
        bad = _half_margin(anchor.astype(np.float64), sizes) < 2 * MARGIN
        if not bad.any():
            break
        anchor[bad] = rng.uniform(-extent, extent, (int(bad.sum()), 3)).astype(F32)
    params = dict(anchor=anchor, anchor_feat=rng.standard_normal((n, 32)).astype(F32),
                  offset=(rng.standard_normal((n, k, 3)) * 1.5).astype(F32),
                  scale_raw=np.log(rng.uniform(0.02, 0.2, (n, 6))).astype(F32),
                  rot_raw=rng.standard_normal((n, 4)).astype(F32))
    for _ in range(200):
        bad = (_half_margin(slot_positions64(params), sizes) < 2 * MARGIN).reshape(n, k)
        if not bad.any():
            break
        params["offset"][bad] = (rng.standard_normal((int(bad.sum()), 3)) * 1.5).astype(F32)
    denom = rng.integers(0, 100, n * k).astype(np.int32)
    denom[rng.random(n * k) < 0.05] = 0
    ths = level_thresholds(cfg)
    avg = np.where(rng.random(n * k) < hot, rng.uniform(1.0, 8.0, n * k), rng.uniform(0.05, 1.0, n * k)) * cfg["grad_threshold"]
    accum = (avg * denom).astype(F32)
    for _ in range(200):
        with np.errstate(all="ignore"):
            a64 = accum.astype(np.float64) / np.maximum(denom, 1)
        bad = np.zeros(n * k, bool)
        for t in ths:
            bad |= (denom > 0) & (np.abs(a64 - t) / t < 2 * MARGIN)
        if not bad.any():
            break
        accum[bad] = (rng.uniform(0.05, 8.0, int(bad.sum())) * cfg["grad_threshold"] * denom[bad]).astype(F32)
    a_denom = rng.integers(0, 160, n).astype(np.int32)
    op = (rng.uniform(0.0, 0.012, n) * a_denom).astype(F32)
    for _ in range(200):
        thr = cfg["min_opacity"] * a_denom.astype(np.float64)
        bad = (a_denom > 0) & (np.abs(op.astype(np.float64) - thr) < 2 * MARGIN * thr)
        if not bad.any():
            break
        op[bad] = (rng.uniform(0.0, 0.012, int(bad.sum())) * a_denom[bad]).astype(F32)
    stats = dict(offset_grad_accum=accum, offset_denom=denom, opacity_accum=op, anchor_denom=a_denom)
    return params, stats


def make_rand(n, k, seed, depth=3):
    return np.random.default_rng(seed + 1000).random((depth, n * k), dtype=F32)


def make_moments(params, seed):
    """Moments that identify their row."""
    rng = np.random.default_rng(seed + 2000)
    return {name: (rng.standard_normal(p.shape).astype(F32), rng.random(p.shape).astype(F32)) for name, p in params.items()}


def t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)
