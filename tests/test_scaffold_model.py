"""CPU tests of the Scaffold-GS decode: the numpy model of tests/scaffold_model.py (what the HIP kernels reproduce bit for bit,
tests/test_gpu_scaffold.py) and gaustudio_amd.scaffold.decode_torch against the reference renderer's own float64 and float32
records (tests/golden/py_scaffold.npz, written by tests/golden/make_scaffold_fixture.py), and the Python boundary.

The bounds are computed, not tuned.  With u = 2^-24 and gamma_n = n u / (1 - n u), a dot product of n terms plus a bias,
summed in ANY order with or without fused multiply-adds, is within gamma_(n+1) (|W| |x| + |b|) of the exact one, and an error
dx of its inputs adds |W| dx; relu is 1-Lipschitz.  Input errors: a component of the unit view direction carries at most
gamma_8 (subtraction, three squares and sums, a root, a quotient), the distance gamma_6 of itself.  The feature bank's softmax
weights carry 2 r + gamma_4 with r = 2 e + u max|o - m| + EXP_REL, e the bound of the bank's logits; the mixed feature then
carries (sum of the three |feat| it mixes) (dw + gamma_3).  Activations: their Lipschitz constant times the bound of the
pre-activation plus the measured approximation error of the gs_exp-built function."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import scaffold_model as sm  # noqa: E402
from gaustudio_amd import scaffold as sc  # noqa: E402
from gaustudio_amd import GaussianRasterizationSettings  # noqa: E402

U = 2.0 ** -24
# approximation errors of the gs_exp-built activations against float64, measured by test_activation_errors below over dense
# sweeps (4 000 001 points); each constant is twice the measured maximum because the sweep is finite
SIGMOID_ABS = 2.1e-7      # measured 1.005e-7 on [-20, 20]
TANH_ABS = 2.6e-7         # measured 1.280e-7 on (0, 20]
EXP_REL = 2.6e-6          # measured 1.273e-6 relative on [-80, 0]


def gamma(n):
    return n * U / (1 - n * U)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "py_scaffold.npz"))


def weights(fx, p, name):
    return tuple(fx[f"{p}{name}_{n}"] for n in ("W1", "b1", "W2", "b2"))


def model_outputs(fx, p):
    bank = weights(fx, p, "bank") if p == "bank_" else None
    return sm.decode(fx[p + "anchor"], fx[p + "anchor_feat"], fx[p + "offset"], fx[p + "scaling"], weights(fx, p, "opacity"),
                     weights(fx, p, "cov"), weights(fx, p, "color"), fx[p + "campos"], fx[p + "visible"], bank)


def layer_bound(w, b, x, dx, n):
    """(exact W x + b, its error bound) in float64 for inputs x known to dx."""
    w, b = np.abs(w.astype(np.float64)), np.abs(b.astype(np.float64))
    return gamma(n + 1) * (np.abs(x) @ w.T + b) + dx @ w.T


def mlp_truth(wts, x, dx):
    """float64 output of the two-layer MLP and the bound of a float32 evaluation's error."""
    w1, b1, w2, b2 = (t.astype(np.float64) for t in wts)
    z1 = x @ w1.T + b1
    e1 = layer_bound(w1, b1, x, dx, w1.shape[1])
    h = np.maximum(z1, 0)
    # the computed hidden value may be as large as h + e1: the second layer's own rounding term is taken on that
    e2 = layer_bound(w2, b2, h + e1, e1, w2.shape[1])
    return h @ w2.T + b2, e2


def truth(fx, p):
    """float64 pre-activations of the visible anchors and their float32 error bounds: dict(logits, cov, color -> (value, bound))."""
    vis = fx[p + "visible"]
    a, f = fx[p + "anchor"][vis].astype(np.float64), fx[p + "anchor_feat"][vis].astype(np.float64)
    v = a - fx[p + "campos"].astype(np.float64)
    d = np.linalg.norm(v, axis=1, keepdims=True)
    vd = np.concatenate([v / d, d], axis=1)
    dvd = np.concatenate([np.full_like(v, gamma(8)), gamma(6) * d], axis=1)
    df = np.zeros_like(f)
    if p == "bank_":
        o, e = mlp_truth(weights(fx, p, "bank"), vd, dvd)
        m = o.max(axis=1, keepdims=True)
        w = np.exp(o - m)
        w = w / w.sum(axis=1, keepdims=True)
        r = 2 * e.max(axis=1, keepdims=True) + U * np.abs(o - m).max(axis=1, keepdims=True) + EXP_REL
        dw = 2 * r + gamma(4)
        c = np.arange(sm.FEAT)
        parts = (f[:, 4 * (c % 8)], f[:, 2 * (c % 16)], f)
        df = (np.abs(parts[0]) + np.abs(parts[1]) + np.abs(parts[2])) * (dw + gamma(3))
        f = parts[0] * w[:, 0:1] + parts[1] * w[:, 1:2] + parts[2] * w[:, 2:3]
    x, dx = np.concatenate([f, vd], axis=1), np.concatenate([df, dvd], axis=1)
    return {name: mlp_truth(weights(fx, p, name), x, dx) for name in ("opacity", "cov", "color")}


def output_bounds(fx, p):
    """Per kept Gaussian: the bounds of the five activated outputs, and the (anchor, offset) indices of the float64 mask."""
    t = truth(fx, p)
    k = fx[p + "offset"].shape[1]
    logits, e_log = t["opacity"]
    assert np.abs(logits - fx[p + "f64_logits"]).max() < 1e-12
    assert np.abs(logits).min() >= 1e-3, "the fixture's condition: no float64 logit within 1e-3 of 0"
    ai, oj = np.nonzero(logits > 0)
    cov, e_cov = (a.reshape(-1, k, 7)[ai, oj] for a in t["cov"])
    e_col = t["color"][1].reshape(-1, k, 3)[ai, oj]
    a = np.nonzero(fx[p + "visible"])[0][ai]
    scaling = fx[p + "scaling"][a].astype(np.float64)
    qn = np.linalg.norm(cov[:, 3:7], axis=1, keepdims=True)
    bounds = dict(
        opacity=(e_log[ai, oj] * 1.0 + TANH_ABS + gamma(2))[:, None], colors=e_col * 0.25 + SIGMOID_ABS + gamma(2),
        scales=scaling[:, 3:6] * (e_cov[:, 0:3] * 0.25 + SIGMOID_ABS + gamma(3)),
        rotations=2 * np.linalg.norm(e_cov[:, 3:7], axis=1, keepdims=True) / qn + gamma(8),
        xyz=gamma(2) * (np.abs(fx[p + "anchor"][a].astype(np.float64))
                        + np.abs(fx[p + "offset"][a, oj].astype(np.float64) * scaling[:, 0:3])))
    return bounds, a, oj, t


REF_NAME = dict(xyz="xyz", colors="color", opacity="opacity", scales="scales", rotations="rotations")


def test_activation_errors():
    """The constants above: twice the measured maximum over a dense sweep."""
    x = np.linspace(-20, 20, 4_000_001).astype(np.float32)
    x64 = x.astype(np.float64)
    e_sig = np.abs(sm.sigmoid(x).astype(np.float64) - 1 / (1 + np.exp(-x64))).max()
    xp = x[x > 0]
    e_tanh = np.abs(sm.tanh_pos(xp).astype(np.float64) - np.tanh(xp.astype(np.float64))).max()
    pp = np.linspace(-80, 0, 4_000_001).astype(np.float32)
    e_exp = np.abs(sm.gs_exp(pp).astype(np.float64) / np.exp(pp.astype(np.float64)) - 1).max()
    print(f"sigmoid {e_sig:.4e}  tanh {e_tanh:.4e}  gs_exp (relative) {e_exp:.4e}")
    assert e_sig <= SIGMOID_ABS / 2 * 1.001 and e_tanh <= TANH_ABS / 2 * 1.001 and e_exp <= EXP_REL / 2 * 1.001
    assert e_sig >= SIGMOID_ABS / 4 and e_tanh >= TANH_ABS / 4 and e_exp >= EXP_REL / 4, "the constants are no longer the measurement"


def test_fma_resolves_float64_ties():
    a = b = np.float32(1 + 2.0 ** -12)               # a b = 1 + 2^-11 + 2^-24: a float32 tie once a tiny c is rounded away
    lo, hi = np.float32(1 + 2.0 ** -11), np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert sm.fma(a, b, np.float32(2.0 ** -60)) == hi
    assert sm.fma(a, b, np.float32(-2.0 ** -60)) == lo
    assert sm.fma(a, b, np.float32(0)) == lo        # the exact tie goes to even


@pytest.mark.parametrize("p", ["plain_", "bank_"])
def test_model_against_float64_record(fx, p):
    bounds, a, oj, t = output_bounds(fx, p)
    out = model_outputs(fx, p)
    assert np.array_equal(out["anchor_index"], a) and np.array_equal(out["offset_index"], oj)
    k = fx[p + "offset"].shape[1]
    for name, got in (("opacity", out["logits"]), ("cov", out["cov_raw"].reshape(-1, 7 * k)), ("color", out["color_raw"].reshape(-1, 3 * k))):
        val, err = t[name]
        ratio = (np.abs(got.astype(np.float64) - val) / err).max()
        print(f"{p}{name}: max |model - float64| / bound = {ratio:.3f}")
        assert ratio <= 1.0
    for name, ref in REF_NAME.items():
        want = fx[p + "f64_" + ref]
        assert out[name].shape == want.shape
        ratio = (np.abs(out[name].astype(np.float64) - want) / bounds[name]).max()
        print(f"{p}{name}: max |model - float64| / bound = {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("p", ["plain_", "bank_"])
def test_reference_float32_record_within_the_same_bounds(fx, p):
    """The reference's own float32 run against its float64 run obeys the same bounds.  Measured ratio of error to bound: 0.002 to
    0.007 for the MLP outputs without the bank (the model's own: 0.010 to 0.013), 0.5 to 0.6 for xyz; with the bank the
    worst-case propagation through the softmax weights and both layers makes the bound some 1e4 times the observed error."""
    bounds, _, _, _ = output_bounds(fx, p)
    for name, ref in REF_NAME.items():
        got, want = fx[p + "f32_" + ref], fx[p + "f64_" + ref]
        assert got.shape == want.shape
        ratio = (np.abs(got.astype(np.float64) - want) / bounds[name]).max()
        print(f"{p}{name}: max |reference float32 - float64| / bound = {ratio:.3f}")
        assert ratio <= 1.0


def torch_model(fx, p, device="cpu"):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    w = lambda name: tuple(t(x) for x in weights(fx, p, name))
    return sc.ScaffoldModel(t(fx[p + "anchor"]), t(fx[p + "anchor_feat"]), t(fx[p + "offset"]), t(fx[p + "scaling"]), t(fx[p + "rot"]),
                            w("opacity"), w("cov"), w("color"), w("bank") if p == "bank_" else None)


def make_view(campos, width=64, height=48, device="cpu"):
    eye = torch.eye(4, dtype=torch.float32, device=device)
    return GaussianRasterizationSettings(height, width, 0.5, 0.4, torch.zeros(3, device=device), 1.0, eye, eye, 1,
                                         torch.as_tensor(campos, dtype=torch.float32, device=device), False, False)


@pytest.mark.parametrize("p", ["plain_", "bank_"])
def test_decode_torch_against_the_record(fx, p):
    bounds, a, oj, _ = output_bounds(fx, p)
    g = sc.decode_torch(torch_model(fx, p), make_view(fx[p + "campos"]), torch.from_numpy(fx[p + "visible"]))
    assert np.array_equal(g.anchor_index.numpy(), a) and np.array_equal(g.offset_index.numpy(), oj)
    assert g.radii is None and np.array_equal(g.visible.numpy(), fx[p + "visible"])
    for name, ref in REF_NAME.items():
        got, want = getattr(g, name).numpy(), fx[p + "f64_" + ref]
        assert got.shape == want.shape and got.dtype == np.float32
        assert (np.abs(got.astype(np.float64) - want) / bounds[name]).max() <= 1.0


def test_bank_index_pattern():
    """repeat tiles: channel c mixes feat[4 (c mod 8)], feat[2 (c mod 16)] and feat[c]."""
    feat = np.arange(32, dtype=np.float32)[None, :] + 100
    for col, pick in ((0, lambda c: 4 * (c % 8)), (1, lambda c: 2 * (c % 16)), (2, lambda c: c)):
        w = np.zeros((1, 3), dtype=np.float32)
        w[0, col] = 1
        got = sm.bank_mix(feat, w)[0]
        assert np.array_equal(got, np.array([100 + pick(c) for c in range(32)], dtype=np.float32))
    # the same through torch's own repeat, and through decode_torch's expression
    ft = torch.from_numpy(feat)
    assert torch.equal(ft[:, ::4].repeat(1, 4)[0], torch.tensor([100.0 + 4 * (c % 8) for c in range(32)]))
    assert torch.equal(ft.unsqueeze(-1)[:, ::2, :1].repeat([1, 2, 1])[0, :, 0], torch.tensor([100.0 + 2 * (c % 16) for c in range(32)]))
    assert sm.bank_mix(feat, np.array([[0.25, 0.5, 0.25]], dtype=np.float32))[0, 9] == np.float32((104 * 0.25 + 118 * 0.5) + 109 * 0.25)


def zero_model(n=3, k=4, b2=0.0):
    m = sm.random_model(n, k, seed=1)
    z = lambda w: tuple(np.zeros_like(t) for t in w)
    op = list(z(m["mlp_opacity"]))
    op[3] = np.full(k, b2, dtype=np.float32)
    m["mlp_opacity"] = tuple(op)
    return m


def test_logit_zero_rule():
    campos = np.zeros(3, dtype=np.float32) + 5
    vis = np.ones(3, dtype=bool)
    assert sm.decode_model(zero_model(b2=0.0), campos, vis)["xyz"].shape == (0, 3)              # logit exactly 0: dropped
    tiny = float(np.finfo(np.float32).tiny)
    out = sm.decode_model(zero_model(b2=tiny), campos, vis)                                     # smallest positive normal: kept
    assert out["xyz"].shape == (12, 3) and np.array_equal(out["offset_index"], np.tile(np.arange(4), 3))
    # gs_exp(0) is 1 + 2^-23 (its polynomial's constant term), so tanh of a logit below about 6e-8 comes out as -2^-24, not 0
    assert np.all(out["opacity"] == np.float32(-2.0 ** -24))
    assert sm.decode_model(zero_model(b2=-tiny), campos, vis)["xyz"].shape == (0, 3)
    for b2, m_want in ((0.0, 0), (tiny, 12)):
        m = zero_model(b2=b2)
        t = lambda a: torch.from_numpy(a)
        tm = sc.ScaffoldModel(t(m["anchor"]), t(m["anchor_feat"]), t(m["offset"]), t(m["scaling"]), t(m["rot"]),
                              *(tuple(t(x) for x in m[n]) for n in ("mlp_opacity", "mlp_cov", "mlp_color")))
        assert sc.decode_torch(tm, make_view(campos), None).xyz.shape[0] == m_want


# ------------------------------------------------------------------------------------------------- the Python boundary
def np_model(n=5, k=3, feat=32, bank=False, dtype=torch.float32):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dtype)
    lin = lambda n_in, n_out: (r(feat, n_in), r(feat), r(n_out, feat), r(n_out))
    return dict(anchor=r(n, 3), anchor_feat=r(n, feat), offset=r(n, k, 3), scaling=r(n, 6).abs(), rot=r(n, 4), mlp_opacity=lin(feat + 4, k),
                mlp_cov=lin(feat + 4, 7 * k), mlp_color=lin(feat + 4, 3 * k), mlp_feature_bank=lin(4, 3) if bank else None)


def test_feat_dim_other_than_32_is_rejected():
    with pytest.raises(ValueError, match="feat_dim"):
        sc.ScaffoldModel(**np_model(feat=16))
    a = np_model()
    a["mlp_cov"] = (torch.zeros(16, 36), torch.zeros(16), torch.zeros(21, 16), torch.zeros(21))
    with pytest.raises(ValueError, match="feat_dim"):
        sc.ScaffoldModel(**a)


@pytest.mark.parametrize("k", [0, 17])
def test_n_offsets_out_of_range(k):
    with pytest.raises(ValueError, match="n_offsets"):
        sc.ScaffoldModel(**np_model(k=max(k, 1)), n_offsets=k)
    if k:
        with pytest.raises(ValueError, match="n_offsets"):
            sc.ScaffoldModel(**np_model(k=k))


def test_dtype_and_shape_checks():
    with pytest.raises(TypeError, match="float32"):
        sc.ScaffoldModel(**np_model(dtype=torch.float64))
    a = np_model()
    a["scaling"] = a["scaling"][:, :3]
    with pytest.raises(ValueError, match="scaling"):
        sc.ScaffoldModel(**a)
    a = np_model()
    a["mlp_color"] = a["mlp_cov"]
    with pytest.raises(ValueError, match="mlp_color"):
        sc.ScaffoldModel(**a)
    m = sc.ScaffoldModel(**np_model())
    with pytest.raises(TypeError, match="bool"):
        sc.decode_torch(m, make_view([0, 0, 0]), torch.ones(5))
    with pytest.raises(ValueError, match="visible_mask"):
        sc.decode_torch(m, make_view([0, 0, 0]), torch.ones(4, dtype=torch.bool))


def test_decode_takes_rocm_tensors_only():
    m = sc.ScaffoldModel(**np_model(bank=True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.decode(m, make_view([0, 0, 5]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.visible_anchors(m, make_view([0, 0, 5]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.decode(m, make_view([0, 0, 5]), torch.ones(5, dtype=torch.bool))


def test_mismatched_devices():
    a = np_model()
    a["offset"] = a["offset"].to("meta")
    m = sc.ScaffoldModel(**a)
    with pytest.raises(ValueError, match="offset is on meta"):
        sc.decode_torch(m, make_view([0, 0, 5]), None)
    with pytest.raises(RuntimeError):
        sc.decode(m, make_view([0, 0, 5]))


def test_unsupported_render_arguments():
    m = sc.ScaffoldModel(**np_model())
    with pytest.raises(NotImplementedError, match="kernel_size"):
        sc.render_scaffold(m, make_view([0, 0, 5]), kernel_size=0.1)
    with pytest.raises(NotImplementedError, match="subpixel_offset"):
        sc.render_scaffold(m, make_view([0, 0, 5]), subpixel_offset=torch.zeros(48, 64, 2))


def sequentials(k=3, bank=True):
    n_in = 36
    return (nn.Sequential(nn.Linear(n_in, 32), nn.ReLU(True), nn.Linear(32, k), nn.Tanh()),
            nn.Sequential(nn.Linear(n_in, 32), nn.ReLU(True), nn.Linear(32, 7 * k)),
            nn.Sequential(nn.Linear(n_in, 32), nn.ReLU(True), nn.Linear(32, 3 * k), nn.Sigmoid()),
            nn.Sequential(nn.Linear(4, 32), nn.ReLU(True), nn.Linear(32, 3), nn.Softmax(dim=1)) if bank else None)


def test_from_modules_and_from_raw():
    a = np_model()
    attrs = {k: a[k] for k in ("anchor", "anchor_feat", "offset", "scaling", "rot")}
    op, cov, col, bank = sequentials()
    m = sc.ScaffoldModel.from_modules(op, cov, col, bank, **attrs)
    assert m.n_offsets == 3 and m.use_feat_bank and m.mlp_cov[2] is cov[2].weight
    # decode_torch of the container equals the reference's arrangement of the same modules
    with torch.no_grad():
        g = sc.decode_torch(m, make_view([0.0, 0.0, 5.0]), None)
        v = attrs["anchor"] - torch.tensor([0.0, 0.0, 5.0])
        d = v.norm(dim=1, keepdim=True)
        w = bank(torch.cat([v / d, d], dim=1))
        f = attrs["anchor_feat"]
        f = f[:, ::4].repeat(1, 4) * w[:, :1] + f[:, ::2].repeat(1, 2) * w[:, 1:2] + f * w[:, 2:]
        opac = op(torch.cat([f, v / d, d], dim=1)).reshape(-1, 1)
        assert torch.allclose(g.opacity, opac[opac[:, 0] > 0], atol=1e-6)
    with pytest.raises(TypeError, match="mlp_opacity"):
        sc.ScaffoldModel.from_modules(cov, cov, col, None, **attrs)                      # no Tanh
    with pytest.raises(ValueError, match="mlp_cov"):
        sc.ScaffoldModel.from_modules(op, sequentials(k=4)[1], col, None, **attrs)
    with pytest.raises(ValueError, match="feat_dim"):
        sc.ScaffoldModel.from_modules(nn.Sequential(nn.Linear(36, 16), nn.ReLU(), nn.Linear(16, 3), nn.Tanh()), cov, col, None, **attrs)
    raw = sc.ScaffoldModel.from_raw(a["anchor"], a["anchor_feat"], a["offset"], a["scaling"].log(), a["rot"] * 3, a["mlp_opacity"],
                                    a["mlp_cov"], a["mlp_color"])
    assert torch.allclose(raw.scaling, a["scaling"]) and torch.allclose(raw.rot.norm(dim=1), torch.ones(5))
    assert raw.to("cpu").n_offsets == 3


def test_exported_from_the_package():
    import gaustudio_amd
    for name in ("ScaffoldModel", "ScaffoldGaussians", "decode", "decode_torch", "render_scaffold", "visible_anchors"):
        assert getattr(gaustudio_amd, name) is getattr(sc, name)
