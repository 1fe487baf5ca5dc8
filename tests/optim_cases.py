"""Inputs shared by tests/test_optim_model.py and tests/test_gpu_optim.py: random Gaussian models, gradients and density
statistics (numpy float32), and clouds whose every densification decision keeps a relative margin from its threshold."""
import math

import numpy as np

F32 = np.float32
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
LR = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=1.25e-4, opacity=5e-2, scaling=5e-3, rotation=1e-3)
CFG = dict(max_grad=2e-4, min_opacity=0.05, extent=4.0, percent_dense=0.01)     # the densification of the tests


def tail(name, k):
    return dict(xyz=(3,), f_dc=(1, 3), f_rest=(k, 3), opacity=(1,), scaling=(3,), rotation=(4,))[name]


def make_params(n, k, seed=0):
    """exp(scaling) spreads over [0.004, 1]: both sides of percent_dense * extent = 0.04 and of 0.1 * extent = 0.4."""
    rng = np.random.default_rng(seed)
    p = dict(xyz=rng.standard_normal((n, 3)) * 2.0, f_dc=rng.standard_normal((n, 1, 3)),
             f_rest=rng.standard_normal((n, k, 3)) * 0.1, opacity=rng.standard_normal((n, 1)) * 2.5,
             scaling=np.log(np.exp(rng.uniform(math.log(0.004), 0.0, (n, 3)))), rotation=rng.standard_normal((n, 4)))
    return {name: np.ascontiguousarray(v, dtype=F32) for name, v in p.items()}


def make_grads(params, seed=1, scale=1e-3):
    rng = np.random.default_rng(seed)
    return {name: (rng.standard_normal(v.shape) * scale).astype(F32) for name, v in params.items()}


def make_stats(n, seed=2, max_grad=CFG["max_grad"]):
    """denom in 0 .. 5 (0: never seen), the average gradient log-uniform within a factor 8 of max_grad, radii in 0 .. 39."""
    rng = np.random.default_rng(seed)
    denom = rng.integers(0, 6, n).astype(np.int32)
    avg = max_grad * np.exp(rng.uniform(-math.log(8.0), math.log(8.0), n))
    return dict(grad_accum=(avg * denom).astype(F32), denom=denom, max_radii=rng.integers(0, 40, n).astype(np.int32))


def decision_ratios(params, stats, n_split, max_screen_size, cfg=CFG):
    """Every decision quantity over its threshold, in float64 from the float32 inputs: a list of arrays (1 = on the threshold)."""
    d = stats["denom"].astype(np.float64)
    with np.errstate(all="ignore"):
        avg = np.where(d > 0, stats["grad_accum"].astype(np.float64) / np.where(d > 0, d, 1.0), 0.0)
    smax = np.exp(params["scaling"].astype(np.float64)).max(axis=1)
    sig = 1.0 / (1.0 + np.exp(-params["opacity"].astype(np.float64).reshape(-1)))
    out = [avg / cfg["max_grad"], smax / (cfg["percent_dense"] * cfg["extent"]), sig / cfg["min_opacity"]]
    if max_screen_size is not None:
        out += [smax / (0.1 * cfg["extent"]), smax / (0.8 * n_split) / (0.1 * cfg["extent"])]
    return out


def margin(params, stats, n_split, max_screen_size, cfg=CFG):
    return min(float(np.abs(r - 1.0).min()) for r in decision_ratios(params, stats, n_split, max_screen_size, cfg) if r.size)


def make_cloud(n, k, seed, n_split=2, max_screen_size=20, cfg=CFG, need=1e-3):
    """(params, stats) with margin >= need: rows that sit nearer to a threshold are moved by two per cent, until none does."""
    params, stats = make_params(n, k, seed), make_stats(n, seed + 1, cfg["max_grad"])
    for _ in range(20):
        r = decision_ratios(params, stats, n_split, max_screen_size, cfg)
        near_avg = np.abs(r[0] - 1.0) < 2 * need
        near_s = np.zeros(n, bool)
        for q in [r[1]] + r[3:]:
            near_s |= np.abs(q - 1.0) < 2 * need
        near_o = np.abs(r[2] - 1.0) < 2 * need
        if not (near_avg.any() or near_s.any() or near_o.any()):
            break
        stats["grad_accum"][near_avg] *= F32(1.02)
        params["scaling"][near_s] += F32(0.02)
        params["opacity"][near_o] += F32(0.05)
    return params, stats


def make_noise(n, n_split, seed=3):
    return np.random.default_rng(seed).standard_normal((n, n_split, 3)).astype(F32)
