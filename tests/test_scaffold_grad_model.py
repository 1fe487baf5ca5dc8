"""CPU tests of the gradient of the Scaffold-GS decode: the numpy models of tests/scaffold_grad_model.py (float32: what the HIP
backward reproduces bit for bit, tests/test_gpu_scaffold_grad.py; float64: the same formulas) and autograd of
gaustudio_amd.scaffold.decode_torch(kept=...) against the reference renderer's own autograd in float64 and float32
(tests/golden/py_scaffold_grad.npz, written by tests/golden/make_scaffold_grad_fixture.py), hand cases, and the Python boundary.

The float32 bound is |model32 - ref64| <= EREF_FACTOR eref + B_exp per leaf.  eref is the reference's own float32 error for the
same inputs; B_exp is the share of the polynomial exp (relative error 1.27e-6, above libm's), computed by
scaffold_grad_model.backward64(act_err=...): the float64 backward run on absolute values, seeded with the error bounds of the
activations' derivative factors that follow from SIGMOID_ABS, TANH_ABS and EXP_REL of tests/test_scaffold_model.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import scaffold_grad_model as gm  # noqa: E402
import scaffold_model as sm  # noqa: E402
from test_scaffold_model import EXP_REL, SIGMOID_ABS, TANH_ABS, make_view  # noqa: E402
from gaustudio_amd import scaffold as sc  # noqa: E402

EREF_FACTOR = 4           # over the reference's own float32 error, as in the Shape-as-Points gradient tests
ACT_ERR = dict(sigmoid=SIGMOID_ABS, tanh=TANH_ABS, exp_rel=EXP_REL)
CAMPOS = np.array([0.3, -0.2, 4.0], dtype=np.float32)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "py_scaffold_grad.npz"))


def fixture_model(fx, p):
    w = lambda name: tuple(fx[f"{p}{name}_{n}"] for n in ("W1", "b1", "W2", "b2"))
    m = {name: fx[p + name] for name in ("anchor", "anchor_feat", "offset", "scaling", "rot")}
    m.update(mlp_opacity=w("opacity"), mlp_cov=w("cov"), mlp_color=w("color"), bank=w("bank") if p == "bank_" else None)
    cot = {name: fx[f"{p}cot_{name}"] for name in gm.COT}
    return m, fx[p + "campos"], fx[p + "visible"], fx[p + "kept"], cot


def leaf_names(p):
    return [k[len(p) + 5:] for k in np.load(os.path.join(HERE, "golden", "py_scaffold_grad.npz")).files if k.startswith(p + "grad_")]


class Model64(sc.ScaffoldModel):
    """decode_torch in float64: the container without its float32 check."""

    def check(self):
        return self


def torch_model(m, dtype=torch.float32, grad=True, cls=None):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(grad)
    w = lambda ws: None if ws is None else tuple(t(x) for x in ws)
    cls = cls or (sc.ScaffoldModel if dtype == torch.float32 else Model64)
    return cls(t(m["anchor"]), t(m["anchor_feat"]), t(m["offset"]), t(m["scaling"]), torch.from_numpy(m["rot"]).to(dtype),
               w(m["mlp_opacity"]), w(m["mlp_cov"]), w(m["mlp_color"]), w(m["bank"]), n_offsets=m["offset"].shape[1])


def torch_leaves(model):
    res = {a: getattr(model, a) for a in ("anchor", "anchor_feat", "offset", "scaling")}
    for name, w in (("opacity", model.mlp_opacity), ("cov", model.mlp_cov), ("color", model.mlp_color), ("bank", model.mlp_feature_bank)):
        if w is not None:
            res.update({f"{name}_{n}": t for n, t in zip(("W1", "b1", "W2", "b2"), w)})
    return res


def decode_torch_grads(m, campos, visible, kept, cot, dtype):
    model = torch_model(m, dtype)
    g = sc.decode_torch(model, make_view(campos), torch.from_numpy(visible), kept=torch.from_numpy(kept))
    lv = torch_leaves(model)
    names = [n for n in gm.COT if cot.get(n) is not None]
    grads = torch.autograd.grad([getattr(g, n) for n in names], list(lv.values()), [torch.from_numpy(cot[n]).to(dtype) for n in names],
                                allow_unused=True)
    grads = [torch.zeros_like(t) if g_ is None else g_ for t, g_ in zip(lv.values(), grads)]
    return {k: t.numpy() for k, t in zip(lv, grads)}


@pytest.mark.parametrize("p", ["plain_", "bank_"])
def test_fixture_conditions(fx, p):
    m, campos, visible, kept, _ = fixture_model(fx, p)
    f64 = lambda t: np.asarray(t, dtype=np.float64)
    vis = np.nonzero(visible)[0]
    v = f64(m["anchor"][vis]) - f64(campos)
    d = np.linalg.norm(v, axis=1, keepdims=True)
    vd = np.concatenate([v / d, d], axis=1)
    f = f64(m["anchor_feat"][vis])
    if m["bank"] is not None:
        wb = [f64(t) for t in m["bank"]]
        pre = vd @ wb[0].T + wb[1]
        assert np.abs(pre).min() >= 1e-5
        o = np.maximum(pre, 0) @ wb[2].T + wb[3]
        e = np.exp(o - o.max(axis=1, keepdims=True))
        w = e / e.sum(axis=1, keepdims=True)
        c = np.arange(sm.FEAT)
        f = f[:, 4 * (c % 8)] * w[:, 0:1] + f[:, 2 * (c % 16)] * w[:, 1:2] + f * w[:, 2:3]
    x = np.concatenate([f, vd], axis=1)
    for name in ("mlp_opacity", "mlp_cov", "mlp_color"):
        w = [f64(t) for t in m[name]]
        pre = x @ w[0].T + w[1]
        assert np.abs(pre).min() >= 1e-5, "the fixture's condition: no hidden pre-activation within 1e-5 of 0"
        if name == "mlp_opacity":
            lg = np.maximum(pre, 0) @ w[2].T + w[3]
            assert np.abs(lg).min() >= 1e-3 and np.array_equal(lg > 0, kept[vis])
    assert not kept[~visible].any()
    # the float32 model keeps the same set
    assert np.array_equal(gm.kept_bits(m, campos, visible)[0], kept)


@pytest.mark.parametrize("p", ["plain_", "bank_"])
def test_float64_model_against_the_reference(fx, p):
    m, campos, visible, kept, cot = fixture_model(fx, p)
    got = gm.leaves(gm.backward64(m, campos, visible, cot, kept), p == "bank_")
    assert set(got) == set(leaf_names(p)) and len(got) == (20 if p == "bank_" else 16)
    for name, g in got.items():
        want, scale = fx[f"{p}grad_{name}"], float(fx[f"{p}gscale_{name}"])
        assert g.shape == want.shape and scale > 0
        err = np.abs(g - want).max()
        print(f"{p}{name}: max |model64 - reference64| / gscale = {err / scale:.2e}")
        assert err <= 1e-12 * scale


@pytest.mark.parametrize("p", ["plain_", "bank_"])
def test_float32_model_against_the_reference(fx, p):
    """Measured on this fixture: error / bound at most 0.37 without the bank (0.25 for d offset, where the model's error IS the
    reference's own). With the bank B_exp is dominated by the softmax
    weights' 2 EXP_REL reaching x and, worst case, every hidden value behind it: the bound is up to 1e5 times the error."""
    m, campos, visible, kept, cot = fixture_model(fx, p)
    bank = p == "bank_"
    got = gm.leaves(gm.backward(m, campos, visible, cot, kept), bank)
    b_exp = gm.leaves(gm.backward64(m, campos, visible, cot, kept, act_err=ACT_ERR), bank)
    for name, g in got.items():
        assert g.dtype == np.float32
        want, eref = fx[f"{p}grad_{name}"], float(fx[f"{p}eref_{name}"])
        err = np.abs(g.astype(np.float64) - want)
        bound = EREF_FACTOR * eref + b_exp[name]
        ok = err <= bound
        ratio = np.where(err > 0, err / np.where(bound > 0, bound, 1.0), 0.0)[bound > 0]
        print(f"{p}{name}: max |model32 - reference64| = {err.max():.3e} ({err.max() / float(fx[f'{p}gscale_{name}']):.1e} of scale), "
              f"eref = {eref:.3e}, max error / bound = {ratio.max() if ratio.size else 0.0:.3f}")
        assert ok.all(), name


@pytest.mark.parametrize("p", ["plain_", "bank_"])
def test_decode_torch_with_kept_is_the_float64_model(fx, p):
    m, campos, visible, kept, cot = fixture_model(fx, p)
    want = gm.leaves(gm.backward64(m, campos, visible, cot, kept), p == "bank_")
    got = decode_torch_grads(m, campos, visible, kept, cot, torch.float64)
    for name, g in got.items():
        assert g.dtype == np.float64 and np.abs(g - want[name]).max() <= 1e-12 * float(fx[f"{p}gscale_{name}"]), name
    # the bit mask [N] of the HIP passes names the same set as the bool [N, k] mask
    packed = (kept.astype(np.int64) << np.arange(kept.shape[1])[None, :]).sum(axis=1).astype(np.uint16)
    assert np.array_equal(gm.unpack_kept(packed, kept.shape[1]), kept)
    model = torch_model(m, grad=False)
    view = make_view(campos)
    a = sc.decode_torch(model, view, torch.from_numpy(visible), kept=torch.from_numpy(kept))
    b = sc.decode_torch(model, view, torch.from_numpy(visible), kept=torch.from_numpy(packed.view(np.int16)))
    assert torch.equal(a.xyz, b.xyz) and torch.equal(a.offset_index, b.offset_index) and a.xyz.shape[0] == int(kept.sum())
    # a kept set that is NOT the sign of the logits: the mask decides
    flipped = kept.copy()
    flipped[np.nonzero(visible)[0][0]] = ~flipped[np.nonzero(visible)[0][0]]
    c = sc.decode_torch(model, view, torch.from_numpy(visible), kept=torch.from_numpy(flipped))
    ai, oj = np.nonzero(flipped)
    assert np.array_equal(c.anchor_index.numpy(), ai) and np.array_equal(c.offset_index.numpy(), oj)


# ------------------------------------------------------------------------------------------------------------ hand cases
def small(n=6, k=4, seed=2, bank=True):
    m = sm.random_model(n, k, seed=seed, bank=bank)
    visible = np.ones(n, dtype=bool)
    kept = np.ones((n, k), dtype=bool)
    rng = np.random.default_rng(seed)
    cot = {name: rng.normal(size=(n * k, c)).astype(np.float32) for name, c in gm.COT.items()}
    return m, visible, kept, cot


def edit(m, name, idx, fn):
    w = [t.copy() for t in m[name]]
    fn(w)
    return dict(m, **{name: tuple(w)})


def test_relu_at_zero_gets_no_gradient():
    m, visible, kept, cot = small()

    def zero_unit(w):
        w[0][5] = 0
        w[1][5] = 0
    m = edit(m, "mlp_cov", 5, zero_unit)
    for g in (gm.backward(m, CAMPOS, visible, cot, kept), gm.backward64(m, CAMPOS, visible, cot, kept)):
        dw1, db1, dw2, db2 = g["mlp_cov"]
        assert not dw1[5].any() and db1[5] == 0 and not dw2[:, 5].any()          # pre-activation 0: dpre = 0, h = 0
        assert dw1[4].any() and db2.any()
    got = decode_torch_grads(m, CAMPOS, visible, kept, cot, torch.float64)
    assert not got["cov_W1"][5].any() and got["cov_b1"][5] == 0


def test_zero_rotation_takes_the_clamp_rule():
    m, visible, kept, cot = small(bank=False)

    def zero_rot(w):
        for j in range(4):
            w[2][7 * j + 3:7 * j + 7] = 0
            w[3][7 * j + 3:7 * j + 7] = 0
    m = edit(m, "mlp_cov", None, zero_rot)
    cot = dict(rotations=cot["rotations"])
    g32 = gm.backward(m, CAMPOS, visible, cot, kept)
    g64 = gm.backward64(m, CAMPOS, visible, cot, kept)
    # n = 0: du = G / 1e-12, so db2 of the rotation rows = sum over anchors of G / 1e-12
    want = (cot["rotations"].astype(np.float64).reshape(6, 4, 4) / 1e-12).sum(axis=0)
    for j in range(4):
        assert np.allclose(g64["mlp_cov"][3][7 * j + 3:7 * j + 7], want[j], rtol=1e-12)
        assert np.allclose(g32["mlp_cov"][3][7 * j + 3:7 * j + 7], want[j], rtol=1e-5)
        assert not g32["mlp_cov"][3][7 * j:7 * j + 3].any()
    t = decode_torch_grads(m, CAMPOS, visible, kept, cot, torch.float64)
    assert np.allclose(t["cov_b2"], g64["mlp_cov"][3], rtol=1e-12)


def test_dropped_offsets_and_empty_anchors():
    m, visible, kept, cot = small()
    kept[:] = False
    kept[2, 1] = True                                      # anchor 2: a single kept offset; every other anchor: none
    cot = {name: c[:1] for name, c in cot.items()}
    for fn in (gm.backward, gm.backward64):
        g = fn(m, CAMPOS, visible, cot, kept)
        assert g["offset"][2, 1].any() and not g["offset"][2, [0, 2, 3]].any()
        for name in ("anchor", "anchor_feat", "offset", "scaling"):
            rest = np.delete(g[name], 2, axis=0)
            assert not rest.any(), name
    # a visible anchor without a kept offset contributes nothing, also to the weight sums: the same as leaving it out
    one = {name: (t[2:3] if name in ("anchor", "anchor_feat", "offset", "scaling", "rot") else t) for name, t in m.items()}
    alone = gm.backward(one, CAMPOS, np.ones(1, bool), cot, kept[2:3])
    full = gm.backward(m, CAMPOS, visible, cot, kept)
    for name in gm.MLPS:
        for a, b in zip(alone[name], full[name]):
            assert np.array_equal(a, b), name


def test_bank_transpose_against_a_dense_matrix():
    """x = T(w) f with the dense [32, 32] matrix T[c, 4 (c % 8)] += w0, T[c, 2 (c % 16)] += w1, T[c, c] += w2: dF = T^t dx."""
    m, visible, kept, cot = small(n=3, k=2, seed=4)
    g = gm.backward64(m, CAMPOS, visible, cot, kept)
    f64 = lambda t: np.asarray(t, dtype=np.float64)
    v = f64(m["anchor"]) - f64(CAMPOS)
    d = np.linalg.norm(v, axis=1, keepdims=True)
    vd = np.concatenate([v / d, d], axis=1)
    wb = [f64(t) for t in m["bank"]]
    o = np.maximum(vd @ wb[0].T + wb[1], 0) @ wb[2].T + wb[3]
    w = np.exp(o) / np.exp(o).sum(axis=1, keepdims=True)
    # dx[0:32] of anchor a from the plain (no bank) backward on the mixed features
    for a in range(3):
        T = np.zeros((32, 32))
        for c in range(32):
            T[c, 4 * (c % 8)] += w[a, 0]
            T[c, 2 * (c % 16)] += w[a, 1]
            T[c, c] += w[a, 2]
        mixed = dict(m, bank=None, anchor_feat=(T @ f64(m["anchor_feat"][a]))[None, :].repeat(3, axis=0))
        plain = gm.backward64(mixed, CAMPOS, visible, cot, kept)
        assert np.allclose(g["anchor_feat"][a], T.T @ plain["anchor_feat"][a], rtol=1e-10, atol=1e-13)
    g32 = gm.backward(m, CAMPOS, visible, cot, kept)
    assert np.abs(g32["anchor_feat"] - g["anchor_feat"]).max() <= 1e-5 * np.abs(g["anchor_feat"]).max()


def test_none_cotangent_is_zeros():
    m, visible, kept, cot = small()
    some = dict(colors=cot["colors"], scales=None)
    zeros = {name: (cot[name] if name == "colors" else np.zeros_like(c)) for name, c in cot.items()}
    for fn in (gm.backward, gm.backward64):
        a, b = fn(m, CAMPOS, visible, some, kept), fn(m, CAMPOS, visible, zeros, kept)
        for name, t in gm.leaves(a, True).items():
            assert np.array_equal(t, gm.leaves(b, True)[name]), name
    a = gm.backward(m, CAMPOS, visible, some, kept)
    assert not a["mlp_opacity"][2].any() and not a["mlp_cov"][2].any() and not a["offset"].any() and a["mlp_color"][2].any()


def test_weight_sum_tree():
    """Block b of 256 anchors belongs to chain b mod 256; a chain adds in ascending anchor order in float32, the chains are added
    in ascending order in float64."""
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    right = np.zeros((4, 0), np.float32)
    left = np.array([[big], [one], [one], [-big]], np.float32)
    same_chain = np.array([0, 1, 256 * 256, 256 * 256 + 1])            # blocks 0 and 256: chain 0, float32: (2^24 + 1 + 1) - 2^24 = 0
    assert gm.weight_sums(same_chain, left, right)[1][0] == 0.0
    two_chains = np.array([0, 256, 257, 65536])                        # chain 0: 2^24 - 2^24 = 0; chain 1: 1 + 1
    assert gm.weight_sums(two_chains, left, right)[1][0] == 2.0
    assert gm.longest_chain(513) == 256 and gm.longest_chain(65537) == 512 and gm.longest_chain(2 * 65536 + 1) == 768


# ------------------------------------------------------------------------------------------------- the Python boundary
def test_backward_keyword_is_checked():
    m, visible, kept, cot = small()
    model = torch_model(m)
    view = make_view(CAMPOS)
    with pytest.raises(ValueError, match="backward"):
        sc.decode(model, view, backward="cuda")
    with pytest.raises(ValueError, match="backward"):
        sc.render_scaffold(model, view, backward="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # the "hip" path refuses CPU tensors, like decode
        sc.decode(model, view, torch.from_numpy(visible), backward="hip")
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.decode(model, view, torch.from_numpy(visible), backward="hip")
    g = sc.decode(model, view, torch.from_numpy(visible))               # the default stays the torch path, on any device
    assert g.xyz.requires_grad
    assert sc.decode(model, view, torch.from_numpy(visible), backward="torch").xyz.shape == g.xyz.shape


def test_kept_argument_is_checked():
    m, visible, kept, cot = small()
    model = torch_model(m, grad=False)
    view = make_view(CAMPOS)
    mask = torch.from_numpy(visible)
    with pytest.raises(ValueError, match="kept"):
        sc.decode_torch(model, view, mask, kept=torch.ones(6, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="kept"):
        sc.decode_torch(model, view, mask, kept=torch.ones(5, dtype=torch.int16))
    with pytest.raises(TypeError, match="kept"):
        sc.decode_torch(model, view, mask, kept=torch.ones(6, 4))
    with pytest.raises(TypeError, match="kept"):
        sc.decode_torch(model, view, mask, kept=torch.ones(6, dtype=torch.int32))
    with pytest.raises(TypeError, match="kept"):
        sc.decode_torch(model, view, mask, kept=np.ones((6, 4), dtype=bool))
    with pytest.raises(ValueError, match="kept is on meta"):
        sc.decode_torch(model, view, mask, kept=torch.ones(6, 4, dtype=torch.bool, device="meta"))
