"""GPU tests of the HIP backward of gaustudio_amd.scaffold.decode (csrc/gsr_scaffold.hip: scaffold_bwd_anchor, scaffold_bwd_wsum,
scaffold_bwd_final).  Every comparison with the numpy model of tests/scaffold_grad_model.py is BIT-EXACT,
the weight tensors included (the model restates the reduction tree); the weight tensors also obey the bound that holds for
any realisation of that tree, |got - sum64| <= ulp + D 2^-24 sum|terms|."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import scaffold_grad_model as gm  # noqa: E402
import scaffold_model as sm  # noqa: E402
from gaustudio_amd import GaussianRasterizationSettings, scenes  # noqa: E402
from gaustudio_amd import scaffold as sc  # noqa: E402

pytestmark = pytest.mark.gpu

CAMPOS = np.array([0.2, -0.1, 3.0], dtype=np.float32)
OUTS = ("xyz", "colors", "opacity", "scales", "rotations")
ATTRS = ("anchor", "anchor_feat", "offset", "scaling")
# approximation errors of the gs_exp-built activations, measured by tests/test_scaffold_model.py::test_activation_errors
ACT_ERR = dict(sigmoid=2.1e-7, tanh=2.6e-7, exp_rel=2.6e-6)
EREF_FACTOR = 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def to_torch(m, dev, grad=True):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad)
    w = lambda ws: None if ws is None else tuple(t(x) for x in ws)
    model = sc.ScaffoldModel(t(m["anchor"]), t(m["anchor_feat"]), t(m["offset"]), t(m["scaling"]),
                             torch.from_numpy(m["rot"]).to(dev), w(m["mlp_opacity"]), w(m["mlp_cov"]), w(m["mlp_color"]), w(m["bank"]),
                             n_offsets=m["offset"].shape[1])
    return model


def make_view(dev, campos=CAMPOS, width=64, height=48, cam=None):
    cam = cam or scenes.make_camera(width, height)
    campos = cam.campos if campos is None else torch.from_numpy(campos)
    return GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0,
                                         cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 1, campos.to(dev), False, False)


def leaves_of(model):
    """name -> tensor in the naming of scaffold_grad_model.leaves."""
    res = {a: getattr(model, a) for a in ATTRS}
    for name, w in (("opacity", model.mlp_opacity), ("cov", model.mlp_cov), ("color", model.mlp_color), ("bank", model.mlp_feature_bank)):
        if w is not None:
            res.update({f"{name}_{n}": t for n, t in zip(("W1", "b1", "W2", "b2"), w)})
    return res


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cotangents(m_rows, seed):
    rng = np.random.default_rng(seed)
    return {name: rng.normal(size=(m_rows, c)).astype(np.float32) for name, c in gm.COT.items()}


def hip_grads(model, view, visible, cot_fn, dev):
    """decode(backward="hip") and its gradients for the cotangents cot_fn(M) -> dict of numpy arrays (a missing name: None)."""
    mask = None if visible is None else torch.from_numpy(visible).to(dev)
    g = sc.decode(model, view, mask, backward="hip")
    cot = cot_fn(g.xyz.shape[0])
    names = [n for n in OUTS if cot.get(n) is not None]
    lv = leaves_of(model)
    grads = torch.autograd.grad([getattr(g, n) for n in names], list(lv.values()),
                                [torch.from_numpy(cot[n]).to(dev) for n in names], allow_unused=True)
    return g, cot, {k: (None if t is None else t.cpu().numpy()) for k, t in zip(lv, grads)}


def assert_grads(got, want, m, n, what=""):
    """Bit for bit against the model; the weight sums also within the bound of the tree.  D = the float32 additions of the
    longest chain: ceil(blocks / SB_CHAINS) blocks of 256 anchors (scaffold_grad_model.longest_chain; csrc: SB_CHAINS = 256
    chains, 256-anchor blocks, block b in chain b mod 256); the float64 stage adds one rounding, the `ulp` term."""
    bank = m["bank"] is not None
    wl = gm.leaves(want, bank)
    assert set(got) == set(wl)
    for name in ATTRS:
        assert got[name].shape == wl[name].shape and got[name].dtype == np.float32
        assert np.array_equal(bits(got[name]), bits(wl[name])), f"{what}d {name} differs from the model"
    D = gm.longest_chain(n)
    for mlp in gm.MLPS[:3] + (("bank",) if bank else ()):
        short = mlp.replace("mlp_", "")
        for (left, right), (wn, bn) in zip(want["terms"][mlp], (("W1", "b1"), ("W2", "b2"))):
            s64, sabs = gm.exact_sums((left, right))
            g = np.concatenate([got[f"{short}_{wn}"], got[f"{short}_{bn}"][:, None]], axis=1)
            ulp = np.spacing(np.maximum(np.abs(s64.astype(np.float32)), np.abs(g))).astype(np.float64)
            err = np.abs(g.astype(np.float64) - s64)
            assert (err <= ulp + D * 2.0 ** -24 * sabs).all(), f"{what}{short}_{wn}/{bn}: beyond the bound of the tree"
        for nm in ("W1", "b1", "W2", "b2"):
            a, b = got[f"{short}_{nm}"], wl[f"{short}_{nm}"]
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), f"{what}d {short}_{nm} differs from the model"


def check(m, visible, dev, seed=0, campos=CAMPOS, cot_fn=None):
    n = m["anchor"].shape[0]
    model = to_torch(m, dev)
    g, cot, got = hip_grads(model, make_view(dev, campos), visible, cot_fn or (lambda mr: cotangents(mr, seed)), dev)
    kept = np.zeros(m["offset"].shape[:2], dtype=bool)
    kept[g.anchor_index.cpu().numpy(), g.offset_index.cpu().numpy()] = True
    mk, _ = gm.kept_bits(m, campos, visible)
    assert np.array_equal(kept, mk)
    want = gm.backward(m, campos, visible, cot, kept, want_terms=True)
    assert_grads(got, want, m, n)
    return g, got


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("k", [1, 3, 10, 16])
def test_against_model(dev, k, bank):
    """N = 513: two full 256-anchor blocks and a one-anchor tail; the offset loop's tails and the row padding (k, 7k, 3k to
    multiples of 4); at k = 16 with the bank the row space needs two slices of scaffold_bwd_wsum."""
    n = 513
    m = sm.random_model(n, k, seed=100 + k, bank=bank)
    visible = np.random.default_rng(k).uniform(size=n) < 0.4
    visible[-1] = True
    g, _ = check(m, visible, dev, seed=k)
    assert g.xyz.shape[0] > 0


@pytest.mark.parametrize("n,k", [(1, 1), (257, 5)])
def test_small_sizes(dev, n, k):
    for seed in range(8):                                   # N = 1, k = 1: the first seed whose single logit is kept
        m = sm.random_model(n, k, seed=n + seed, bank=True)
        if gm.kept_bits(m, CAMPOS, np.ones(n, bool))[0].any():
            break
    g, _ = check(m, np.ones(n, dtype=bool), dev)
    assert g.xyz.shape[0] > 0


def test_blank_block_and_empty_mask(dev):
    n, k = 513, 4
    m = sm.random_model(n, k, seed=7, bank=True)
    visible = np.random.default_rng(7).uniform(size=n) < 0.4
    visible[256:512] = False                                 # a whole block without a visible anchor
    visible[512] = True
    _, got = check(m, visible, dev)
    assert not got["anchor_feat"][256:512].any() and not got["offset"][~visible].any()
    g, got = check(m, np.zeros(n, dtype=bool), dev)          # M = 0: no launch, zeros
    assert g.xyz.shape[0] == 0
    for name, a in got.items():
        assert a is not None and not a.any(), name


def test_chain_tail(dev):
    """N = 2 * 65536 + 1: chain 0 owns blocks 0, 256 and 512 (three chunks, the accumulators pass through the partials buffer
    twice) and block 512 is one anchor.  Visible: all of block 0, all of block 256, the tail anchor, block 300 (a chain with a
    single busy block in the second chunk) and some 2000 scattered anchors; the model walks the visible anchors only."""
    n, k = 2 * 65536 + 1, 3
    m = sm.random_model(n, k, seed=9, bank=True)
    visible = np.random.default_rng(9).uniform(size=n) < 2000 / n
    visible[0:256] = True
    visible[256 * 256:257 * 256] = True
    visible[300 * 256:301 * 256] = True
    visible[n - 1] = True
    assert visible.sum() <= 3000 and gm.longest_chain(n) == 3 * 256
    check(m, visible, dev)


def test_forward_is_the_no_grad_forward(dev):
    n = 3000
    m = sm.random_model(n, 10, seed=21, bank=True)
    view = make_view(dev, None, 320, 240, cam=scenes.make_camera(320, 240, T=(0.0, 0.0, 4.0)))
    model = to_torch(m, dev)
    with torch.no_grad():
        want = sc.decode(model, view, backward="hip")
    got = sc.decode(model, view, backward="hip")
    assert got.xyz.requires_grad and got.opacity.requires_grad and not want.xyz.requires_grad and want.xyz.shape[0] > 0
    for f in sc.ScaffoldGaussians._fields:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.detach(), b), f
        if f not in OUTS:
            assert not a.requires_grad
    mask = want.visible
    got = sc.decode(model, view, mask, backward="hip")
    assert got.radii is None and torch.equal(got.colors.detach(), want.colors)
    plain = to_torch(m, dev, grad=False)                     # nothing requires grad: the keyword changes nothing
    assert not sc.decode(plain, view, backward="hip").xyz.requires_grad


class Model64(sc.ScaffoldModel):
    """decode_torch in float64: the container without its float32 check."""

    def check(self):
        return self


def torch_grads(m, campos, visible, kept, cot, dtype, device):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(device).requires_grad_(True)
    w = lambda ws: None if ws is None else tuple(t(x) for x in ws)
    cls = sc.ScaffoldModel if dtype == torch.float32 else Model64
    model = cls(t(m["anchor"]), t(m["anchor_feat"]), t(m["offset"]), t(m["scaling"]), torch.from_numpy(m["rot"]).to(dtype).to(device),
                w(m["mlp_opacity"]), w(m["mlp_cov"]), w(m["mlp_color"]), w(m["bank"]), n_offsets=m["offset"].shape[1])
    eye = torch.eye(4, device=device)
    view = GaussianRasterizationSettings(48, 64, 0.5, 0.4, torch.zeros(3, device=device), 1.0, eye, eye, 1,
                                         torch.from_numpy(campos).to(device), False, False)
    g = sc.decode_torch(model, view, torch.from_numpy(visible).to(device), kept=torch.from_numpy(kept).to(device))
    lv = leaves_of(model)
    grads = torch.autograd.grad([getattr(g, n) for n in OUTS], list(lv.values()),
                                [torch.from_numpy(cot[n]).to(dtype).to(device) for n in OUTS])
    return {k: t.detach().cpu().numpy() for k, t in zip(lv, grads)}


def test_against_torch_on_the_device(dev):
    """decode(backward="hip") against autograd of decode_torch(kept = the HIP mask) on the same GPU, within 4 E + B_exp: E =
    |decode_torch float32 - decode_torch float64| on the CPU for the same inputs (torch's own float32 error, never the code
    under test), B_exp the first-order share of the polynomial exp (scaffold_grad_model.backward64(act_err=...))."""
    n, k = 2000, 10
    m = sm.random_model(n, k, seed=77, bank=True)
    visible = np.random.default_rng(77).uniform(size=n) < 0.4
    model = to_torch(m, dev)
    g, cot, got = hip_grads(model, make_view(dev), visible, lambda mr: cotangents(mr, 3), dev)
    kept = np.zeros((n, k), dtype=bool)
    kept[g.anchor_index.cpu().numpy(), g.offset_index.cpu().numpy()] = True
    on_gpu = torch_grads(m, CAMPOS, visible, kept, cot, torch.float32, dev)
    cpu32 = torch_grads(m, CAMPOS, visible, kept, cot, torch.float32, "cpu")
    cpu64 = torch_grads(m, CAMPOS, visible, kept, cot, torch.float64, "cpu")
    b_exp = gm.leaves(gm.backward64(m, CAMPOS, visible, cot, kept, act_err=ACT_ERR), True)
    for name in got:
        e = np.abs(cpu32[name].astype(np.float64) - cpu64[name]).max()
        err = np.abs(got[name].astype(np.float64) - on_gpu[name].astype(np.float64))
        bound = EREF_FACTOR * e + b_exp[name]
        print(f"{name}: max |hip - torch| = {err.max():.3e}, E = {e:.3e}, max err / bound = {(err / bound).max():.3f}")
        assert (err <= bound).all(), name


def test_cotangent_handling(dev):
    n, k = 513, 5
    m = sm.random_model(n, k, seed=13, bank=True)
    visible = np.random.default_rng(13).uniform(size=n) < 0.5
    view = make_view(dev)
    # a loss on colors only: None for the other four cotangents
    _, got = check(m, visible, dev, cot_fn=lambda mr: dict(colors=cotangents(mr, 1)["colors"]))
    for name in ("opacity_W1", "opacity_b1", "opacity_W2", "opacity_b2", "cov_W1", "cov_b1", "cov_W2", "cov_b2", "offset", "scaling"):
        assert not got[name].any(), name
    assert got["color_W2"].any() and got["anchor_feat"].any() and got["bank_W1"].any()
    # a non-contiguous cotangent: sum() hands backward an expanded scalar
    model = to_torch(m, dev)
    g = sc.decode(model, view, torch.from_numpy(visible).to(dev), backward="hip")
    (g.scales.sum() + g.rotations[:, 1].sum()).backward()
    mr = g.xyz.shape[0]
    rot = np.zeros((mr, 4), np.float32)
    rot[:, 1] = 1
    want = gm.backward(m, CAMPOS, visible, dict(scales=np.ones((mr, 3), np.float32), rotations=rot), want_terms=True)
    assert_grads({k_: t.grad.cpu().numpy() for k_, t in leaves_of(model).items()}, want, m, n, "expand: ")
    # only anchor_feat requires grad
    model = to_torch(m, dev, grad=False)
    model.anchor_feat.requires_grad_(True)
    g = sc.decode(model, view, torch.from_numpy(visible).to(dev), backward="hip")
    (g.scales.sum() + g.rotations[:, 1].sum()).backward()
    assert np.array_equal(bits(model.anchor_feat.grad.cpu().numpy()), bits(want["anchor_feat"]))
    assert all(t.grad is None for name, t in leaves_of(model).items() if name != "anchor_feat")


def render_setup(n, seed, dev):
    m = sm.random_model(n, 10, seed=seed, bank=True)
    m["anchor"] = (m["anchor"] * np.float32(0.7)).astype(np.float32)
    view = make_view(dev, None, 64, 48, cam=scenes.make_camera(64, 48, T=(0.0, 0.0, 5.0)))
    return m, view


def test_end_to_end_through_the_rasterizer(dev):
    n = 700
    m, view = render_setup(n, 31, dev)
    model = to_torch(m, dev)
    out = sc.render_scaffold(model, view, backward="hip")
    g = out["gaussians"]
    for name in OUTS:
        getattr(g, name).retain_grad()
    target = torch.linspace(0, 1, 3 * 48 * 64, device=dev).reshape(3, 48, 64)
    (out["render"] - target).abs().mean().backward()
    cot = {name: getattr(g, name).grad.cpu().numpy() for name in OUTS}
    assert all(np.abs(c).max() > 0 for c in cot.values())
    visible = g.visible.cpu().numpy()
    campos = view.campos.cpu().numpy()
    want = gm.backward(m, campos, visible, cot, want_terms=True)
    assert_grads({k: t.grad.cpu().numpy() for k, t in leaves_of(model).items()}, want, m, n, "render: ")


def test_two_runs_a_side_stream_and_retain_graph(dev):
    n = 3000
    m = sm.random_model(n, 10, seed=21, bank=True)
    visible = np.random.default_rng(2).uniform(size=n) < 0.6
    view = make_view(dev)

    def run():
        _, _, got = hip_grads(to_torch(m, dev), view, visible, lambda mr: cotangents(mr, 4), dev)
        return got

    first = run()
    again = run()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    for name, a in first.items():
        assert np.array_equal(bits(a), bits(again[name])) and np.array_equal(bits(a), bits(third[name])), name
    model = to_torch(m, dev)
    g = sc.decode(model, view, torch.from_numpy(visible).to(dev), backward="hip")
    loss = (g.colors * g.opacity).sum() + g.scales.sum()
    lv = list(leaves_of(model).values())
    a = torch.autograd.grad(loss, lv, retain_graph=True)
    b = torch.autograd.grad(loss, lv, retain_graph=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_adam_lowers_an_image_loss(dev):
    n = 2000
    m, view = render_setup(n, 5, dev)
    with torch.no_grad():
        target = sc.render_scaffold(to_torch(m, dev, grad=False), view)["render"]
    rng = np.random.default_rng(0)
    pert = dict(m, anchor_feat=(m["anchor_feat"] + rng.normal(size=m["anchor_feat"].shape).astype(np.float32) * np.float32(0.5)),
                mlp_color=tuple((t + rng.normal(size=t.shape).astype(np.float32) * np.float32(0.1)) for t in m["mlp_color"]))
    model = to_torch(pert, dev, grad=False)
    params = [model.anchor_feat] + list(model.mlp_color)
    for p in params:
        p.requires_grad_(True)
    opt = torch.optim.Adam(params, lr=1e-2)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = (sc.render_scaffold(model, view, backward="hip")["render"] - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"loss {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert losses[-1] < losses[0]
