"""The float32 numpy model of gaustudio_amd.optim (csrc/gsr_optim.hip): every operation in the kernels'
order, every intermediate float32.  It is the DEFINITION of what GaussianAdam and DensityControl compute: the GPU tests compare
with it bit for bit (NaN in the same places); tests/test_optim_model.py compares it with torch.optim.Adam and with the float64
restatement of the published densification (tests/optim_reference.py).

Adam, per element, plain IEEE operations, none contracted:
    m' = m + (g - m) c1;   v' = v + (g g - v) c2;   p' = p - s (m' / (sqrt(v') / b + eps))
with c1 = f32(1 - beta1), c2 = f32(1 - beta2), b = f32(sqrt(1 - beta2^t)), s = f32(lr / (1 - beta1^t)), each formed in float64
(Python floats: the C library's pow, sqrt and log, as the host code of the kernels uses them) and rounded once.

Child of a split source: xyz + ((R0 a0 + R1 a1) + R2 a2) per component, a = gs_exp(clamp(scaling, -80, 80)) * noise, R the
rotation of q / |q| with |q|^2 = ((w w + x x) + y y) + z z; scaling - d_split.  gs_exp is the library's polynomial exp
(scaffold_model.gs_exp)."""
import math
from collections import namedtuple

import numpy as np

from scaffold_model import gs_exp

F32 = np.float32
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")

Report = namedtuple("Report", "n_cloned n_split n_pruned n_before n_after")


# ------------------------------------------------------------------------------------------------------------------ Adam
def adam_consts(lr, beta1, beta2, step):
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    return F32(1.0 - beta1), F32(1.0 - beta2), F32(math.sqrt(bc2)), F32(lr / bc1)


def adam_update(p, g, m, v, consts, eps):
    """(p', m', v') of float32 arrays of one shape."""
    c1, c2, b, s = consts
    p, g, m, v = (np.asarray(a, dtype=F32) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        m2 = (m + (g - m) * c1).astype(F32)
        v2 = (v + (g * g - v) * c2).astype(F32)
        den = (np.sqrt(v2) / b + F32(eps)).astype(F32)
        p2 = (p - s * (m2 / den)).astype(F32)
    return p2, m2, v2


class AdamModel:
    """GaussianAdam: params / grads are dicts of float32 arrays; a group whose grad is None is skipped."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-15):
        self.params = {k: np.array(params[k], dtype=F32) for k in GROUPS}
        self.lr = dict(lr)
        self.betas, self.eps = betas, eps
        self.step_count = 0
        self.exp_avg = {k: np.zeros_like(self.params[k]) for k in GROUPS}
        self.exp_avg_sq = {k: np.zeros_like(self.params[k]) for k in GROUPS}

    def step(self, grads, visible=None):
        self.step_count += 1
        rows = None if visible is None else np.asarray(visible) > 0
        for k in GROUPS:
            g = grads.get(k)
            if g is None or self.params[k].size == 0:
                continue
            consts = adam_consts(self.lr[k], self.betas[0], self.betas[1], self.step_count)
            p2, m2, v2 = adam_update(self.params[k], g, self.exp_avg[k], self.exp_avg_sq[k], consts, self.eps)
            if rows is None:
                self.params[k], self.exp_avg[k], self.exp_avg_sq[k] = p2, m2, v2
            else:
                self.params[k][rows], self.exp_avg[k][rows], self.exp_avg_sq[k][rows] = p2[rows], m2[rows], v2[rows]


# ------------------------------------------------------------------------------------------------------------------ statistics
def new_stats(n):
    return dict(grad_accum=np.zeros(n, F32), denom=np.zeros(n, np.int32), max_radii=np.zeros(n, np.int32))


def accumulate(stats, means2d_grad, radii):
    mg, r = np.asarray(means2d_grad, dtype=F32), np.asarray(radii, dtype=np.int32)
    seen = r > 0
    with np.errstate(all="ignore"):
        norm = np.sqrt((mg[:, 0] * mg[:, 0] + mg[:, 1] * mg[:, 1]).astype(F32)).astype(F32)
        stats["grad_accum"][seen] = (stats["grad_accum"] + norm).astype(F32)[seen]
    stats["denom"][seen] += 1
    stats["max_radii"][seen] = np.maximum(stats["max_radii"], r)[seen]


# ------------------------------------------------------------------------------------------------------------------ densify
def thresholds(percent_dense, extent, min_opacity, n_split):
    """(t_big, t_world, t_op, d_split): float64 on the host, rounded once."""
    t_op = -math.inf if min_opacity == 0 else math.log(min_opacity / (1.0 - min_opacity))
    return (F32(math.log(percent_dense * extent)), F32(math.log(0.1 * extent)), F32(t_op), F32(math.log(0.8 * n_split)))


def classify(scaling, opacity, stats, max_grad, th, max_screen_size):
    """(survives, clone emitted, children emitted, clone-class, split-class) per source row."""
    t_big, t_world, t_op, d_split = th
    s = np.asarray(scaling, dtype=F32)
    with np.errstate(all="ignore"):
        d = stats["denom"]
        avg = np.where(d > 0, stats["grad_accum"] / np.where(d > 0, d, 1).astype(F32), F32(0)).astype(F32)
        hot = avg >= F32(max_grad)
        smax = s[:, 0].copy()
        smax = np.where(s[:, 1] > smax, s[:, 1], smax)
        smax = np.where(s[:, 2] > smax, s[:, 2], smax)
        big = smax > t_big
        clone, split = hot & ~big, hot & big
        low = np.asarray(opacity, dtype=F32).reshape(-1) < t_op
        if max_screen_size is None:
            fail_self, fail_child = low, low
        else:
            fail_self = low | (stats["max_radii"] > int(math.floor(max_screen_size))) | (smax > t_world)
            fail_child = low | ((smax - d_split).astype(F32) > t_world)
    return ~split & ~fail_self, clone & ~fail_self, split & ~fail_child, clone, split


def child_xyz(xyz, scaling, rotation, noise):
    """[n,3] children of n split sources for one child index: noise [n,3]."""
    q = np.asarray(rotation, dtype=F32)
    with np.errstate(all="ignore"):
        qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        nrm = np.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
        r, x, y, z = qw / nrm, qx / nrm, qy / nrm, qz / nrm
        sc = np.asarray(scaling, dtype=F32)
        cl = np.where(sc < F32(-80), F32(-80), np.where(sc > F32(80), F32(80), sc)).astype(F32)
        a = (gs_exp(cl) * np.asarray(noise, dtype=F32)).astype(F32)
        one, two = F32(1), F32(2)
        rows = ((one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)),
                (two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)),
                (two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)))
        off = np.stack([(r0 * a[:, 0] + r1 * a[:, 1]) + r2 * a[:, 2] for r0, r1, r2 in rows], axis=1).astype(F32)
        return (np.asarray(xyz, dtype=F32) + off).astype(F32)


def _compact(adam, fa, fb, fc, n_split, noise, d_split):
    n_a, n_b, n_c = int(fa.sum()), int(fb.sum()), int(fc.sum())
    P, M, V = adam.params, adam.exp_avg, adam.exp_avg_sq
    new_p, new_m, new_v = {}, {}, {}
    for k in GROUPS:
        parts = [P[k][fa], P[k][fb]]
        for c in range(n_split if n_c else 0):
            src = P[k][fc]
            if k == "xyz":
                src = child_xyz(src, P["scaling"][fc], P["rotation"][fc], noise[fc, c])
            elif k == "scaling":
                src = (src - d_split).astype(F32)
            parts.append(src)
        new_p[k] = np.concatenate(parts, axis=0).astype(F32)
        extra = new_p[k].shape[0] - n_a
        zeros = np.zeros((extra,) + P[k].shape[1:], F32)
        new_m[k] = np.concatenate([M[k][fa], zeros], axis=0)
        new_v[k] = np.concatenate([V[k][fa], zeros], axis=0)
    adam.params, adam.exp_avg, adam.exp_avg_sq = new_p, new_m, new_v
    return n_a, n_b, n_c


def densify_and_prune(adam, stats, max_grad, min_opacity, extent, max_screen_size=None, n_split=2, noise=None,
                      percent_dense=0.01):
    """In place on the AdamModel; returns (Report, new zero statistics)."""
    n = adam.params["xyz"].shape[0]
    th = thresholds(percent_dense, extent, min_opacity, n_split)
    fa, fb, fc, _, _ = classify(adam.params["scaling"], adam.params["opacity"], stats, max_grad, th, max_screen_size)
    n_a, n_b, n_c = _compact(adam, fa, fb, fc, n_split, np.asarray(noise, dtype=F32), th[3])
    n_after = n_a + n_b + n_split * n_c
    return Report(n_b, n_c, n - n_a - n_c, n, n_after), new_stats(n_after)


def prune(adam, stats, mask):
    """Rows where mask is True leave; survivors carry moments and statistics."""
    mask = np.asarray(mask, dtype=bool)
    n = mask.shape[0]
    none = np.zeros(n, bool)
    n_a, _, _ = _compact(adam, ~mask, none, none, 1, None, F32(0))
    return Report(0, 0, n - n_a, n, n_a), {k: v[~mask].copy() for k, v in stats.items()}


def reset_opacity(adam, max_opacity=0.01):
    cap = F32(math.log(max_opacity / (1.0 - max_opacity)))
    adam.params["opacity"] = np.minimum(adam.params["opacity"], cap).astype(F32)
    adam.exp_avg["opacity"] = np.zeros_like(adam.exp_avg["opacity"])
    adam.exp_avg_sq["opacity"] = np.zeros_like(adam.exp_avg_sq["opacity"])


def same_bits(a, b):
    """Equal as bytes, or NaN in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    an, bn = np.isnan(a), np.isnan(b)
    ai, bi = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    return bool(np.array_equal(an, bn) and np.array_equal(ai[~an], bi[~bn]))
