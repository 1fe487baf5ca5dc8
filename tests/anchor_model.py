"""The numpy model of gaustudio_amd.anchor_control (csrc/gsr_anchor.hip): every operation in the kernels'
order, every intermediate float32.  It is the DEFINITION of what AnchorControl.accumulate and .adjust compute -- parameters,
moments, statistics and the report; the GPU tests compare with it bit for bit, tests/test_anchor_model.py compares it with the
float64 restatement of the published sequence (tests/anchor_reference.py).

A candidate's position per component: anchor + offset * s, one product and one sum, s = gs_exp(clamp(scale_raw[:, 0:3], -80,
80)) (scaffold_model.gs_exp, the library's polynomial exp); its cell rint(p / cur), a correctly rounded float32 divide and
round-half-to-even.  Keys: three signed 21-bit fields, biased, x most significant.  The per-cell maximum feature is taken in the
total order of the floats in which -0 < +0, so it does not depend on the order of a cell's candidates."""
import math
from collections import namedtuple

import numpy as np

from scaffold_model import gs_exp

F32 = np.float32
NAMES = ("anchor", "anchor_feat", "offset", "scale_raw", "rot_raw")
STATS = ("offset_grad_accum", "offset_denom", "opacity_accum", "anchor_denom")
CELL_MIN, CELL_MAX = -(1 << 20), (1 << 20) - 1
MAX_ANCHORS, SLOT_LIMIT = 1 << 24, 1 << 31

Report = namedtuple("Report", "n_grown n_pruned n_before n_after")


def zero_stats(n, k):
    return dict(offset_grad_accum=np.zeros(n * k, F32), offset_denom=np.zeros(n * k, np.int32), opacity_accum=np.zeros(n, F32),
                anchor_denom=np.zeros(n, np.int32))


def accumulate(stats, k, anchor_index, offset_index, opacity, viewspace_grad, radii, visible):
    """In place on `stats`.  anchor_index / offset_index int [M] (anchor-major runs), opacity [M,1], viewspace_grad [M,3],
    radii [M], visible bool [N]."""
    aidx, oidx = np.asarray(anchor_index, np.int64), np.asarray(offset_index, np.int64)
    op = np.asarray(opacity, F32).reshape(-1)
    vg = np.asarray(viewspace_grad, F32)
    seen = np.asarray(radii) > 0
    slot = aidx[seen] * k + oidx[seen]
    gx, gy = vg[seen, 0], vg[seen, 1]
    with np.errstate(all="ignore"):
        norm = np.sqrt(((gx * gx).astype(F32) + (gy * gy).astype(F32)).astype(F32)).astype(F32)
        stats["offset_grad_accum"][slot] = (stats["offset_grad_accum"][slot] + norm).astype(F32)
    stats["offset_denom"][slot] += 1
    stats["anchor_denom"][np.asarray(visible, bool)] += 1
    m = len(aidx)
    i = 0
    while i < m:                                    # the head of a run sums it in order, then one addition to the accumulator
        e, s = i + 1, op[i]
        while e < m and aidx[e] == aidx[i]:
            with np.errstate(all="ignore"):
                s = F32(s + op[e])
            e += 1
        with np.errstate(all="ignore"):
            stats["opacity_accum"][aidx[i]] = F32(stats["opacity_accum"][aidx[i]] + s)
        i = e
    return stats


def level_plan(voxel_size, grad_threshold, update_depth, update_init_factor, update_hierarchy_factor):
    """[(cur_i, t_i, rand_min_i)], float32."""
    return [(F32(voxel_size * (update_init_factor // update_hierarchy_factor ** i)),
             F32(grad_threshold * (update_hierarchy_factor // 2) ** i), F32(0.5 ** (i + 1))) for i in range(update_depth)]


def slot_positions(params):
    """float32 [N k, 3]."""
    anchor, offset, scale_raw = (np.asarray(params[n], F32) for n in ("anchor", "offset", "scale_raw"))
    with np.errstate(all="ignore"):
        s = gs_exp(np.clip(scale_raw[:, 0:3], F32(-80), F32(80)))
        p = (anchor[:, None, :] + (offset * s[:, None, :]).astype(F32)).astype(F32)
    return p.reshape(-1, 3)


def cells_of(p, cur):
    """float32 cells (not yet integers: NaN and infinities stay)."""
    with np.errstate(all="ignore"):
        return np.rint((np.asarray(p, F32) / F32(cur)).astype(F32)).astype(F32)


def fits(cells):
    with np.errstate(all="ignore"):
        return ((cells >= F32(CELL_MIN)) & (cells <= F32(CELL_MAX))).all(axis=-1)


def keys_of(cells_int):
    c = np.asarray(cells_int, np.int64) - CELL_MIN
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def cells_from_keys(keys):
    keys = np.asarray(keys, np.int64)
    return np.stack([(keys >> 42) & 0x1FFFFF, (keys >> 21) & 0x1FFFFF, keys & 0x1FFFFF], axis=1) + CELL_MIN


def f2ord(x):
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def ord2f(o):
    o = np.ascontiguousarray(o, dtype=np.uint32)
    return np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(F32)


def grow(params, stats, k, plan, mature_min, rand):
    """The levels: [(cur, cells int64 [c,3] in ascending key order, features float32 [c,32])] for every level that ran and added
    something, and the counts per level.  Raises ValueError for a candidate out of range; nothing is modified."""
    n = params["anchor"].shape[0]
    accum, denom = stats["offset_grad_accum"], stats["offset_denom"]
    with np.errstate(all="ignore"):
        avg = np.where(denom > 0, accum / np.maximum(denom, 1).astype(F32), F32(0)).astype(F32)
    mature = denom > mature_min
    pos = slot_positions(params)
    levels, counts = [], []
    for i, (cur, t_i, rand_min) in enumerate(plan):
        if n == 0 or (i > 0 and sum(counts) == 0):
            counts.append(0)
            continue
        with np.errstate(all="ignore"):
            cand = (avg >= t_i) & mature & (np.asarray(rand[i], F32) > rand_min)
        slots = np.nonzero(cand)[0]
        cc = cells_of(pos[slots], cur)
        if not fits(cc).all():
            raise ValueError("a growing candidate's position is not finite or its voxel cell is outside [-2^20, 2^20)")
        current = [np.asarray(params["anchor"], F32)] + [(c.astype(F32) * lc).astype(F32) for lc, c, _ in levels]
        ac = cells_of(np.concatenate(current, axis=0), cur)
        ac = ac[fits(ac)]
        occupied = np.unique(keys_of(ac.astype(np.int64)))
        ukeys, inv = np.unique(keys_of(cc.astype(np.int64)), return_inverse=True)
        fresh = ~np.isin(ukeys, occupied)
        best = np.zeros((len(ukeys), 32), np.uint32)
        np.maximum.at(best, inv.reshape(-1), f2ord(np.asarray(params["anchor_feat"], F32)[slots // k]))
        counts.append(int(fresh.sum()))
        if counts[-1]:
            levels.append((cur, cells_from_keys(ukeys[fresh]), ord2f(best[fresh])))
    return levels, counts


def adjust(params, moments, stats, k, voxel_size, rand, check_interval=100, success_threshold=0.8, grad_threshold=2e-4,
           min_opacity=0.005, update_depth=3, update_init_factor=16, update_hierarchy_factor=4):
    """params: name -> float32 array; moments: name -> (exp_avg, exp_avg_sq) for the leaves that have them (may be {});
    stats: the four statistics.  Returns (params, moments, stats, Report, levels) -- all new arrays."""
    n = params["anchor"].shape[0]
    mature_min = int(math.floor(check_interval * success_threshold * 0.5))
    settled_min = int(math.floor(check_interval * success_threshold))
    plan = level_plan(voxel_size, grad_threshold, update_depth, update_init_factor, update_hierarchy_factor)
    levels, counts = grow(params, stats, k, plan, mature_min, rand)
    a_denom, op_accum = stats["anchor_denom"], stats["opacity_accum"]
    settled = a_denom > settled_min
    with np.errstate(all="ignore"):
        prune = settled & (op_accum < (F32(min_opacity) * a_denom.astype(F32)).astype(F32))
    keep = ~prune
    n_new = sum(counts)
    n_after = int(keep.sum()) + n_new
    if n_after > MAX_ANCHORS or n_after * k >= SLOT_LIMIT:
        raise ValueError("the model after this pass is too large")

    def rows(old, fresh):
        return np.concatenate([np.asarray(old)[keep]] + fresh, axis=0)

    fresh = dict(
        anchor=[(c.astype(F32) * cur).astype(F32) for cur, c, _ in levels],
        anchor_feat=[f for _, _, f in levels],
        offset=[np.zeros((len(c), k, 3), F32) for _, c, _ in levels],
        scale_raw=[np.full((len(c), 6), F32(math.log(float(cur))), F32) for cur, c, _ in levels],
        rot_raw=[np.tile(np.array([1, 0, 0, 0], F32), (len(c), 1)) for _, c, _ in levels])
    new_params = {name: rows(np.asarray(params[name], F32), fresh[name]) for name in NAMES}
    new_moments = {name: tuple(rows(np.asarray(mv, F32), [np.zeros_like(f) for f in fresh[name]]) for mv in moments[name])
                   for name in moments}
    mature = stats["offset_denom"] > mature_min
    accum = np.where(mature, F32(0), stats["offset_grad_accum"]).astype(F32).reshape(n, k)
    denom = np.where(mature, 0, stats["offset_denom"]).astype(np.int32).reshape(n, k)
    new_stats = dict(
        offset_grad_accum=np.concatenate([accum[keep].reshape(-1), np.zeros(n_new * k, F32)]),
        offset_denom=np.concatenate([denom[keep].reshape(-1), np.zeros(n_new * k, np.int32)]),
        opacity_accum=np.concatenate([np.where(settled, F32(0), op_accum).astype(F32)[keep], np.zeros(n_new, F32)]),
        anchor_denom=np.concatenate([np.where(settled, 0, a_denom).astype(np.int32)[keep], np.zeros(n_new, np.int32)]))
    return new_params, new_moments, new_stats, Report(tuple(counts), int(prune.sum()), n, n_after), levels
