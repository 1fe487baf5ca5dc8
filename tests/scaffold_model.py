"""The float32 numpy model of gaustudio_amd.scaffold.decode (csrc/gsr_scaffold.hip): every operation in the
kernel's order, every intermediate float32.  It is the DEFINITION of what decode returns for a given visible mask: the GPU
tests compare with it bit for bit; tests/test_scaffold_model.py compares it with the reference's own renderer
(tests/golden/py_scaffold.npz) within a computed rounding bound.

  * every dot product: acc = bias; acc = fma(W[o][i], x[i], acc) for i ascending;
  * relu(x) = 0 where x < 0 (a NaN stays); the kept test is logit > 0;
  * exp is the library's polynomial gs_exp (csrc/gsr_common.h), restated here; its argument is always <= 0 and clamped at -80;
  * sigmoid(x) = 1 / (1 + e^-x) for x >= 0, e^x / (1 + e^x) otherwise; tanh(x) = (1 - e) / (1 + e), e = e^(-2x), for the kept
    x > 0; softmax over three values with the maximum taken out, sum (e0 + e1) + e2;
  * |v| = sqrt(fma(z, z, fma(y, y, x x))) for the view direction, the same chain over four entries for the rotation.

fma(): the float64 product of two float32 values is exact; its float64 sum with a float32 is rounded once, and rounding that
to float32 is a second rounding that differs from fmaf only when the float64 sum sits exactly on a float32 tie
(mesh_init_model.fma has the same caveat and leaves it).  Here the dot products are long enough (about 7000 per anchor) to
meet such ties, so the tie is detected and resolved by the sign of the float64 addition's error.  Not covered: results in the
float32 subnormal range, where the tie sits at another bit."""
import numpy as np

F32 = np.float32
FEAT = 32

LOG2E = F32(float.fromhex("0x1.715476p+0"))
MAGIC = F32(12582912.0)
EXP_C = [F32(float.fromhex(h)) for h in ("0x1.5c08e6p-10", "0x1.3d0c52p-7", "0x1.c6b6e4p-5", "0x1.ebf918p-3", "0x1.62e428p-1",
                                         "0x1.000002p+0")]


def fma(a, b, c):
    """fmaf(a, b, c), elementwise with broadcasting."""
    a64, b64, c64 = (np.asarray(v, dtype=F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        s = a64 * b64
        t = np.atleast_1d(s + c64)
        r = t.astype(F32)
        tie = (np.ascontiguousarray(t).view(np.int64) & 0x1FFFFFFF) == 0x10000000
        if tie.any():
            sb, cb = np.broadcast_to(s, t.shape)[tie], np.broadcast_to(c64, t.shape)[tie]
            tt = t[tie]
            bb = tt - sb
            e = (sb - (tt - bb)) + (cb - bb)                  # TwoSum: sb + cb = tt + e exactly
            toward = np.where(e > 0, np.inf, -np.inf)
            r[tie] = np.where(e != 0, np.nextafter(tt, toward), tt).astype(F32)
    return r.reshape(np.broadcast(a64, b64, c64).shape)


def gs_exp(p):
    """csrc/gsr_common.h gs_exp: exp(p) for p in [-80, 0]."""
    p = np.asarray(p, dtype=F32)
    tm = fma(p, LOG2E, MAGIC)
    nf = tm - MAGIC
    f = fma(p, LOG2E, -nf)
    y = np.broadcast_to(EXP_C[0], p.shape)
    for c in EXP_C[1:]:
        y = fma(y, f, c)
    bits = np.ascontiguousarray(y).view(np.uint32) + (np.ascontiguousarray(tm).view(np.uint32) << np.uint32(23))
    return bits.view(F32)


def clamp80(t):
    return np.where(t < F32(-80), F32(-80), t).astype(F32)


def sigmoid(x):
    x = np.asarray(x, dtype=F32)
    with np.errstate(all="ignore"):
        pos = x >= 0
        e = gs_exp(clamp80(np.where(pos, -x, x)))
        return np.where(pos, F32(1) / (F32(1) + e), e / (F32(1) + e)).astype(F32)


def tanh_pos(x):
    """tanh(x) for x > 0."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(all="ignore"):
        e = gs_exp(clamp80(F32(-2) * x))
        return ((F32(1) - e) / (F32(1) + e)).astype(F32)


def softmax3(o):
    """[n,3] -> [n,3]."""
    o = np.asarray(o, dtype=F32)
    with np.errstate(all="ignore"):
        m = o[:, 0]
        m = np.where(o[:, 1] > m, o[:, 1], m)
        m = np.where(o[:, 2] > m, o[:, 2], m)
        e = gs_exp(clamp80(o - m[:, None]))
        s = (e[:, 0] + e[:, 1]) + e[:, 2]
        return (e / s[:, None]).astype(F32)


def linear(w, b, x):
    """[n,in] -> [n,out]: bias first, then fma over the ascending input index."""
    w, b, x = np.asarray(w, dtype=F32), np.asarray(b, dtype=F32), np.asarray(x, dtype=F32)
    acc = np.broadcast_to(b[None, :], (x.shape[0], w.shape[0])).astype(F32)
    for i in range(w.shape[1]):
        acc = fma(w[None, :, i], x[:, i:i + 1], acc)
    return acc


def relu(x):
    return np.where(x < 0, F32(0), x).astype(F32)


def mlp(wts, x):
    return linear(wts[2], wts[3], relu(linear(wts[0], wts[1], x)))


def norm_chain(u):
    """sqrt(fma(u[-1], u[-1], ... fma(u[1], u[1], u[0] u[0])))."""
    acc = u[..., 0] * u[..., 0]
    for i in range(1, u.shape[-1]):
        acc = fma(u[..., i], u[..., i], acc)
    return np.sqrt(acc)


def bank_mix(feat, w):
    """feat[:, ::4].repeat(4) w0 + feat[:, ::2].repeat(2) w1 + feat w2 -- repeat tiles: channel c reads 4 (c mod 8), 2 (c mod 16)."""
    c = np.arange(FEAT)
    return ((feat[:, 4 * (c % 8)] * w[:, 0:1] + feat[:, 2 * (c % 16)] * w[:, 1:2]) + feat * w[:, 2:3]).astype(F32)


def inputs(anchor, feat, campos, bank=None):
    """x [n,36] = [feat', view, dist] of the given anchors."""
    with np.errstate(all="ignore"):
        v = (np.asarray(anchor, dtype=F32) - np.asarray(campos, dtype=F32).reshape(1, 3)).astype(F32)
        d = norm_chain(v)
        vd = np.concatenate([v / d[:, None], d[:, None]], axis=1).astype(F32)
        feat = np.asarray(feat, dtype=F32)
        if bank is not None:
            feat = bank_mix(feat, softmax3(mlp(bank, vd)))
        return np.concatenate([feat, vd], axis=1).astype(F32)


def decode(anchor, anchor_feat, offset, scaling, mlp_opacity, mlp_cov, mlp_color, campos, visible, bank=None):
    """dict(xyz, colors, opacity [M,1], scales, rotations, anchor_index, offset_index int32 [M]) and, for the visible anchors in
    order, the pre-activations logits [V,k], cov_raw [V,k,7], color_raw [V,k,3]."""
    anchor, scaling, offset = (np.asarray(t, dtype=F32) for t in (anchor, scaling, offset))
    k = offset.shape[1]
    vis = np.nonzero(np.asarray(visible).astype(bool))[0]
    with np.errstate(all="ignore"):
        x = inputs(anchor[vis], np.asarray(anchor_feat, dtype=F32)[vis], campos, bank)
        logits = mlp(mlp_opacity, x)
        keep = logits > 0
        ai, oj = np.nonzero(keep)
        cov_raw = mlp(mlp_cov, x).reshape(-1, k, 7)
        color_raw = mlp(mlp_color, x).reshape(-1, k, 3)
        cov = cov_raw[ai, oj]
        a = vis[ai]
        n = norm_chain(cov[:, 3:7])
        dn = np.where(n < F32(1e-12), F32(1e-12), n)
        out = dict(
            xyz=(anchor[a] + offset[a, oj] * scaling[a, 0:3]).astype(F32), colors=sigmoid(color_raw[ai, oj]),
            opacity=tanh_pos(logits[ai, oj]).reshape(-1, 1), scales=(scaling[a, 3:6] * sigmoid(cov[:, 0:3])).astype(F32),
            rotations=(cov[:, 3:7] / dn[:, None]).astype(F32), anchor_index=a.astype(np.int32), offset_index=oj.astype(np.int32),
            logits=logits, cov_raw=cov_raw, color_raw=color_raw)
    return out


def random_model(n, k, seed=0, bank=False, weight_scale=0.3):
    """A seeded model as float32 arrays: dict(anchor, anchor_feat, offset, scaling, rot, mlp_opacity, mlp_cov, mlp_color, bank)."""
    rng = np.random.default_rng(seed)
    f = lambda *s, sc=1.0: (rng.normal(size=s) * sc).astype(F32)
    lin = lambda n_in, n_out: (f(FEAT, n_in, sc=weight_scale), f(FEAT, sc=0.1), f(n_out, FEAT, sc=weight_scale), f(n_out, sc=0.1))
    q = rng.normal(size=(n, 4))
    return dict(anchor=f(n, 3), anchor_feat=f(n, FEAT), offset=f(n, k, 3, sc=0.5), scaling=np.exp(f(n, 6, sc=0.3) - F32(3)).astype(F32),
                rot=(q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)).astype(F32), mlp_opacity=lin(FEAT + 4, k),
                mlp_cov=lin(FEAT + 4, 7 * k), mlp_color=lin(FEAT + 4, 3 * k), bank=lin(4, 3) if bank else None)


def decode_model(m, campos, visible):
    return decode(m["anchor"], m["anchor_feat"], m["offset"], m["scaling"], m["mlp_opacity"], m["mlp_cov"], m["mlp_color"], campos,
                  visible, m["bank"])
