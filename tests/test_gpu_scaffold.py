"""GPU tests of gaustudio_amd.scaffold (csrc/gsr_scaffold.hip).  Every comparison with the numpy model of
tests/scaffold_model.py is BIT-EXACT; the visible filter is compared with the operator's own forward, element for element."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import scaffold_model as sm  # noqa: E402
from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, scenes  # noqa: E402
from gaustudio_amd import scaffold as sc  # noqa: E402

pytestmark = pytest.mark.gpu

SCAN_TILE = 1024          # csrc/gsr_sort.h: the exclusive scan works in 1024-element tiles
FIELDS = ("xyz", "colors", "opacity", "scales", "rotations", "anchor_index", "offset_index")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def to_torch(m, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    w = lambda ws: None if ws is None else tuple(t(x) for x in ws)
    return sc.ScaffoldModel(t(m["anchor"]), t(m["anchor_feat"]), t(m["offset"]), t(m["scaling"]), t(m["rot"]), w(m["mlp_opacity"]),
                            w(m["mlp_cov"]), w(m["mlp_color"]), w(m["bank"]), n_offsets=m["offset"].shape[1])


def make_view(dev, width=64, height=48, scale_modifier=1.0, cam=None):
    cam = cam or scenes.make_camera(width, height)
    return GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), scale_modifier,
                                         cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 1, cam.campos.to(dev), False, False)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(g, ref, what=""):
    """ScaffoldGaussians against the model's dict (or another ScaffoldGaussians), bit for bit."""
    for f in FIELDS:
        got = getattr(g, f).cpu().numpy()
        want = ref[f] if isinstance(ref, dict) else getattr(ref, f).cpu().numpy()
        assert got.shape == want.shape, f"{what}{f}: shape {got.shape} != {want.shape}"
        assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want)), f"{what}{f} differs"


def check_against_model(m, dev, visible, campos=None):
    view = make_view(dev)
    if campos is not None:
        view = view._replace(campos=torch.from_numpy(campos).to(dev))
    g = sc.decode(to_torch(m, dev), view, torch.from_numpy(visible).to(dev))
    ref = sm.decode_model(m, view.campos.cpu().numpy(), visible)
    assert_same(g, ref)
    assert g.radii is None and np.array_equal(g.visible.cpu().numpy(), visible)
    return g


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("k", [1, 3, 10, 16])
def test_decode_against_model(dev, k, bank):
    """Lane, wave and workgroup tails (64-lane waves, 256-thread groups) and the offset loop's tail."""
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
        m = sm.random_model(n, k, seed=n + k, bank=bank)
        visible = np.random.default_rng(n).uniform(size=n) < 0.7
        g = check_against_model(m, dev, visible, campos=np.array([0.2, -0.1, 3.0], dtype=np.float32))
        if n == 0:
            assert g.xyz.shape == (0, 3) and g.opacity.shape == (0, 1) and g.anchor_index.shape == (0,)


def with_opacity_bias(m, b2):
    """The model with an opacity MLP of zero weights and the given last bias [k] or [n-independent scalar]: logit j = b2[j]."""
    op = [np.zeros_like(t) for t in m["mlp_opacity"]]
    op[3] = np.broadcast_to(np.asarray(b2, dtype=np.float32), op[3].shape).copy()
    return dict(m, mlp_opacity=tuple(op))


def test_scan_edges(dev):
    k = 4
    for n in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1):
        m = sm.random_model(n, k, seed=n)
        check_against_model(m, dev, np.ones(n, dtype=bool))
    n = SCAN_TILE + 37
    m = sm.random_model(n, k, seed=3, bank=True)
    allv = np.ones(n, dtype=bool)
    g = check_against_model(with_opacity_bias(m, 1.0), dev, allv)                                   # every offset kept
    assert g.xyz.shape[0] == n * k
    g = check_against_model(with_opacity_bias(m, -1.0), dev, allv)                                  # none kept
    assert g.xyz.shape[0] == 0
    g = check_against_model(m, dev, np.zeros(n, dtype=bool))                                        # nothing visible
    assert g.xyz.shape[0] == 0
    last = np.zeros(n, dtype=bool)
    last[-1] = True
    g = check_against_model(with_opacity_bias(m, [-1, -1, 1, -1]), dev, last)                       # one Gaussian, in the last anchor
    assert g.xyz.shape[0] == 1 and int(g.anchor_index[0]) == n - 1 and int(g.offset_index[0]) == 2
    runs = np.zeros(n, dtype=bool)                                                                 # runs of count-0 anchors between kept ones
    runs[[0, 5, 6, 300, SCAN_TILE - 1, SCAN_TILE, n - 2]] = True
    g = check_against_model(m, dev, runs)
    assert set(g.anchor_index.cpu().tolist()) <= set(np.nonzero(runs)[0].tolist())


def test_logit_edges(dev):
    n, k = 70, 4
    m = sm.random_model(n, k, seed=8)
    allv = np.ones(n, dtype=bool)
    tiny = float(np.finfo(np.float32).tiny)
    denorm = float(np.nextafter(np.float32(0), np.float32(1)))
    g = check_against_model(with_opacity_bias(m, [0.0, tiny, -0.0, denorm]), dev, allv)            # 0 and -0 dropped, the smallest kept
    assert g.xyz.shape[0] == 2 * n and set(g.offset_index.cpu().tolist()) == {1, 3}
    g = check_against_model(with_opacity_bias(m, [50.0, 40.0, 39.9, 1e30]), dev, allv)             # -2 x at and beyond the -80 clamp
    assert g.xyz.shape[0] == 4 * n and float(g.opacity.min()) == 1.0
    nanrow = dict(m, anchor_feat=m["anchor_feat"].copy())
    nanrow["anchor_feat"][[3, 64]] = np.nan                                                        # NaN logits: nan > 0 is false
    g = check_against_model(nanrow, dev, allv)
    assert not ({3, 64} & set(g.anchor_index.cpu().tolist()))
    assert bool(torch.isfinite(g.colors).all())


def filter_scene(n, seed, dev):
    rng = np.random.default_rng(seed)
    m = sm.random_model(n, 3, seed=seed)
    a = m["anchor"]
    a[:, 0:2] = rng.uniform(-4, 4, size=(n, 2))
    a[:, 2] = rng.uniform(-2, 12, size=n)                       # a share behind the camera
    a[0] = (0.0, 0.0, 0.2)                                      # exactly on the near plane: culled (z <= 0.2)
    a[1] = (0.0, 0.0, np.nextafter(np.float32(0.2), np.float32(1)))
    a[2] = (1000.0, 0.0, 5.0)                                   # far off-screen: a zero-area tile rect
    a[3] = (0.0, -1000.0, 5.0)
    a[4] = (0.0, 0.0, -3.0)
    m["scaling"][5] = 0.0                                       # degenerate scales: the 0.3 low-pass alone
    a[5] = (0.1, 0.1, 4.0)
    m["scaling"][6, 0:3] = (1e-30, 5.0, 0.0)
    a[6] = (-0.5, 0.2, 6.0)
    m["scaling"][7, 0:3] = 1e4                                  # huge
    a[7] = (0.0, 0.0, 3.0)
    m["rot"][8] = 0.0                                           # a zero quaternion
    a[8] = (0.2, 0.0, 3.0)
    return m


@pytest.mark.parametrize("size", [(16, 16), (17, 31), (640, 480)])
@pytest.mark.parametrize("scale_modifier", [1.0, 2.5])
def test_filter_against_the_operator(dev, size, scale_modifier):
    n = 1500
    m = filter_scene(n, size[0], dev)
    model = to_torch(m, dev)
    view = make_view(dev, size[0], size[1], scale_modifier)
    mask, radii = sc.visible_anchors(model, view)
    with torch.no_grad():
        out = GaussianRasterizer(view)(means3D=model.anchor, means2D=torch.zeros_like(model.anchor),
                                       opacities=torch.ones(n, 1, device=dev), colors_precomp=torch.rand(n, 3, device=dev),
                                       scales=model.scaling[:, :3].contiguous(), rotations=model.rot)
    assert radii.dtype == torch.int32 and torch.equal(radii, out[1])
    assert mask.dtype == torch.bool and torch.equal(mask, out[1] > 0)
    assert not bool(mask[0]) and not bool(mask[2]) and not bool(mask[3]) and not bool(mask[4])
    assert 0 < int(mask.sum()) < n
    # decode with the camera filter = decode with that mask given
    g_cam, g_mask = sc.decode(model, view), sc.decode(model, view, mask)
    assert_same(g_cam, g_mask)
    assert torch.equal(g_cam.radii, radii) and torch.equal(g_cam.visible, mask) and g_mask.radii is None


def test_two_runs_and_a_side_stream(dev):
    n = 3000
    model = to_torch(sm.random_model(n, 10, seed=21, bank=True), dev)
    view = make_view(dev, 320, 240, cam=scenes.make_camera(320, 240, T=(0.0, 0.0, 4.0)))
    first = sc.decode(model, view)
    assert first.xyz.shape[0] > 0
    assert_same(sc.decode(model, view), first)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        again = sc.decode(model, view)
    side.synchronize()
    assert_same(again, first)
    assert torch.equal(again.radii, first.radii)


def test_mid_size_against_model(dev):
    n, k = 100_000, 10
    m = sm.random_model(n, k, seed=5, bank=True)
    visible = np.random.default_rng(6).uniform(size=n) < 0.4
    g = check_against_model(m, dev, visible)
    assert g.xyz.shape[0] > n


def test_render_scaffold_equals_the_operator(dev):
    n = 4000
    m = sm.random_model(n, 10, seed=31)
    m["anchor"] = (m["anchor"] * np.float32(0.7)).astype(np.float32)
    model = to_torch(m, dev)
    view = make_view(dev, 200, 120, cam=scenes.make_camera(200, 120, T=(0.0, 0.0, 5.0)))
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    with torch.no_grad():
        out = sc.render_scaffold(model, view, bg=bg)
        g = sc.decode(model, view)
        want = GaussianRasterizer(view._replace(bg=bg))(means3D=g.xyz, means2D=torch.zeros_like(g.xyz), opacities=g.opacity,
                                                        colors_precomp=g.colors, scales=g.scales, rotations=g.rotations)
    assert_same(out["gaussians"], g)
    for name, w in zip(("render", "radii", "depth", "median_depth", "opacity"), want):
        assert torch.equal(out[name], w), name
    assert torch.equal(out["visibility_filter"], want[1] > 0) and out["viewspace_points"].shape == g.xyz.shape
    assert out["render"].shape == (3, 120, 200) and float(out["opacity"].max()) > 0.1


def test_decode_under_grad_takes_the_torch_path(dev):
    m = sm.random_model(500, 5, seed=41, bank=True)
    model = to_torch(m, dev)
    leaves = [model.anchor_feat] + list(model.mlp_opacity) + list(model.mlp_cov) + list(model.mlp_color) + list(model.mlp_feature_bank)
    for t in leaves:
        t.requires_grad_(True)
    view = make_view(dev, cam=scenes.make_camera(64, 48, T=(0.0, 0.0, 4.0)))
    g = sc.decode(model, view)
    assert g.opacity.requires_grad and g.radii is not None and g.xyz.shape[0] > 0
    (g.opacity.sum() + g.colors.sum() + g.scales.sum() + (g.rotations * torch.arange(4.0, device=dev)).sum()).backward()
    for t in leaves:
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0
    with torch.no_grad():
        hip = sc.decode(model, view)
    assert not hip.opacity.requires_grad and hip.xyz.shape[0] > 0      # (the two paths are not compared: their logits differ in the last bits)
