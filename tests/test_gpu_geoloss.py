"""GPU tests of gaustudio_amd.surfel_losses (csrc/gsr_geoloss.hip) against the float32 model tests/geoloss_model.py.

Every comparison with the model is EXACT (same_bits: NaN in the same places, the bytes of everything else): loss, both parts,
every map of surfel_maps with and without a viewmatrix, and all seven planes of the gradient.  The library is built without
contraction and with correctly rounded divide and sqrt, and the model restates every operation and the float64 partial tree,
so there is nothing to tolerate.  Shapes sit on the edges of the stencil (3) and of the workgroup's tile (16 x 64).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import geoloss_model as gm  # noqa: E402
import geoloss_model_parity as parity  # noqa: E402
from gaustudio_amd import scenes, surfel_losses  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
TH, TW = surfel_losses.TILE_H, surfel_losses.TILE_W
MAPS = tuple(gm.MAP_PLANES)
VIEW = scenes.look_at_camera(64, 48, (1.0, -2.0, -3.0), (0.0, 0.2, 0.4)).viewmatrix

SHAPES = [(1, 1), (2, 5), (3, 3), (5, 4), (TH, TW), (TH - 1, TW - 1), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 2)]
assert SHAPES[-1] == (33, 130)       # three tile rows and columns: the backward's halo-2 gather crosses tile corners both ways


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def noisy(shape, seed):
    """An allmap with no structure: depth in [1, 3), alpha in (0.2, 1], normals in [-1, 1), median in [1, 3)."""
    H, W = shape
    rng = np.random.default_rng([seed, H, W])
    a = np.zeros((7, H, W))
    alpha = 1.0 - 0.8 * rng.random((H, W))
    a[0], a[1] = (1.0 + 2.0 * rng.random((H, W))) * alpha, alpha
    a[2:5] = 2.0 * rng.random((3, H, W)) - 1.0
    a[5] = 1.0 + 2.0 * rng.random((H, W))
    a[6] = rng.random((H, W))
    return a.astype(F32), parity.intrinsics_of(H, W)


def run_hip(a, intr, ln=0.05, ld=0.0, rho=0.0, grad_loss=1.0, maps=True):
    """Forward and backward through autograd, the maps without and with a viewmatrix; everything back on the host."""
    ai = gpu(a).requires_grad_(True)
    loss, nl, dl = surfel_losses.surfel_geometric_loss_with_parts(ai, intr, ln, ld, rho)
    (loss * grad_loss if grad_loss != 1.0 else loss).backward()
    out = dict(loss=host(loss), normal_loss=host(nl), dist_loss=host(dl), grad=host(ai.grad))
    if maps:
        out.update({k: host(v) for k, v in surfel_losses.surfel_maps(ai, intr, None, rho).items()})
        out.update({"world_" + k: host(v) for k, v in surfel_losses.surfel_maps(ai, intr, VIEW, rho).items()})
    return out


def check(a, intr, ln=0.05, ld=0.0, rho=0.0, grad_loss=1.0):
    got = run_hip(a, intr, ln, ld, rho, grad_loss)
    want = gm.loss_and_grad(a, intr, ln, ld, rho, grad_loss)
    world = gm.forward(a, intr, ln, ld, rho, viewmatrix=VIEW.numpy())
    want.update({"world_" + k: world[k] for k in MAPS})
    for k in ("loss", "normal_loss", "dist_loss", "grad") + MAPS + tuple("world_" + k for k in MAPS):
        assert got[k].dtype == F32 and got[k].shape == np.shape(want[k]), k
        assert gm.same_bits(got[k], want[k]), f"{k} differs from the model: max |d| = {np.nanmax(np.abs(got[k] - want[k]))}"
    return got, want


# --------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_exact(hw):
    a, intr = noisy(hw, 1)
    check(a, intr, 0.05, 3.0, 0.25)


def test_many_partials_exact():
    """17 x 18 tiles: 306 workgroup partials, more than one pass of the final kernel's 256 lanes plus a ragged tail of 50."""
    shape = (17 * TH, 18 * TW)
    assert shape == (272, 1152) and 17 * 18 > 256
    a, intr = noisy(shape, 2)
    check(a, intr, 0.05, 3.0, 0.5)


# --------------------------------------------------------------------------------------------------------- values
VSHAPE = (2 * TH + 1, 2 * TW + 2)


@pytest.mark.parametrize("rho", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("name", parity.SCENES)
def test_smooth_scenes_exact(name, rho):
    a, intr = parity.scene(name, VSHAPE)
    got, _ = check(a, intr, 0.05, 100.0, rho)
    if rho == 0.0:
        assert np.all(got["grad"][5] == 0)
    if rho == 1.0:
        assert np.all(got["grad"][0] == 0) and np.all(got["grad"][1] == 0)


@pytest.mark.parametrize("ln,ld", [(0.0, 3.0), (0.7, 0.0), (0.0, 0.0)])
def test_lambda_zero_terms(ln, ld):
    a, intr = noisy(VSHAPE, 3)
    got, _ = check(a, intr, ln, ld)
    if ln == 0.0:
        assert got["normal_loss"] == 0 and np.all(got["grad"][:6] == 0)
    if ld == 0.0:
        assert got["dist_loss"] == 0 and np.all(got["grad"][6] == 0)


def test_zero_alpha_regions_straddle_tile_edges():
    a, intr = parity.scene("sphere_cap", VSHAPE)
    hole = np.zeros(VSHAPE, bool)
    hole[TH - 2:TH + 3, TW - 3:TW + 2] = True          # across the corner of four tiles
    hole[2 * TH - 1:, 5:9] = True                      # across a tile row's edge and onto the image border
    hole[0, 0] = True
    a[1][hole] = 0.0                                   # a0 / 0 = +inf
    a[0][TH, TW] = 0.0                                 # 0 / 0 = NaN
    a[0][TH - 1, TW - 1] = -a[0][TH - 1, TW - 1]       # -inf
    for rho in (0.0, 0.5):
        got, _ = check(a, intr, 0.05, 10.0, rho)
        assert np.all(got["rendered_depth"][0][hole] == 0)
        assert np.all(got["grad"][0][hole] == 0) and np.all(got["grad"][1][hole] == 0)
        for k, v in got.items():
            assert np.isfinite(v).all(), k


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_median(bad):
    a, intr = parity.scene("tilted_plane", VSHAPE)
    for y, x in ((TH, TW - 1), (0, 3), (TH - 1, 2 * TW)):
        a[5][y, x] = bad
    for rho in (0.5, 1.0):
        got, _ = check(a, intr, 0.05, 0.0, rho)
        assert got["rendered_median_depth"][0][TH, TW - 1] == 0 and got["grad"][5][TH, TW - 1] == 0
        assert np.isfinite(got["loss"]) and np.isfinite(got["grad"]).all()


def test_nan_normal_reaches_the_loss():
    a, intr = parity.scene("tilted_plane", VSHAPE)
    a[3][0, 5] = np.nan                                # a border pixel: N * 0 is still NaN
    a[2][TH, TW] = np.nan                              # an interior one, on a tile corner
    got, _ = check(a, intr, 0.05, 2.0)
    assert np.isnan(got["loss"]) and np.isnan(got["normal_loss"]) and np.isfinite(got["dist_loss"])
    assert np.isnan(got["normal_error"][0, 5]) and np.isnan(got["normal_error"][TH, TW]) and np.isnan(got["normal_error"]).sum() == 2


def test_all_zero_depth():
    a = np.zeros((7,) + VSHAPE, F32)
    a[1], a[2:5] = 0.5, 0.3
    got, _ = check(a, parity.intrinsics_of(*VSHAPE))
    assert np.all(got["surf_normal"] == 0) and np.all(got["grad"] == 0) and got["normal_loss"] == F32(0.05)


def test_parts_and_entry_points_agree():
    a, intr = noisy(VSHAPE, 4)
    x = gpu(a)
    loss, nl, dl = surfel_losses.surfel_geometric_loss_with_parts(x, intr, 0.1, 2.0, 0.5)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and not loss.requires_grad
    assert torch.equal(surfel_losses.surfel_geometric_loss(x, intr, 0.1, 2.0, 0.5), loss)
    # intrinsics as a CPU tensor and as a device tensor (read back) give the same launch
    for t in (torch.tensor(intr, dtype=torch.float64), torch.tensor(intr, dtype=torch.float64).cuda()):
        assert torch.equal(surfel_losses.surfel_geometric_loss(x, t, 0.1, 2.0, 0.5), loss)
    m = surfel_losses.surfel_maps(x, intr, None, 0.5)
    assert m["rendered_depth"].shape == (1,) + VSHAPE and m["surf_normal"].shape == (3,) + VSHAPE and m["normal_error"].shape == VSHAPE
    # the maps of the published renderer, in torch
    q = x[0].cpu() / x[1].cpu()                                    # (on the host: an IEEE divide)
    assert torch.equal(m["rendered_depth"][0].cpu(), torch.where(torch.isfinite(q), q, torch.zeros_like(q)))
    assert torch.equal(m["rendered_median_depth"][0], x[5])
    assert torch.equal(m["rendered_normal"], x[2:5])
    mw = surfel_losses.surfel_maps(x, intr, VIEW.cuda(), 0.5)
    want = (x[2:5].permute(1, 2, 0).double() @ VIEW[:3, :3].T.double().cuda()).permute(2, 0, 1)
    assert (mw["rendered_normal"].double() - want).abs().max() < 1e-6


# ------------------------------------------------------------------------------------------------------- autograd
def test_scaled_and_reused_loss():
    a, intr = noisy(VSHAPE, 5)
    check(a, intr, 0.05, 3.0, 0.5, grad_loss=3.0)                  # (3 loss).backward(): the upstream gradient is read on the device
    ai = gpu(a).requires_grad_(True)
    loss = surfel_losses.surfel_geometric_loss(ai, intr, 0.05, 3.0, 0.5)
    (loss + 0.5 * loss).backward()                                 # the loss twice in one graph: upstream 1 + 0.5
    assert gm.same_bits(host(ai.grad), gm.backward(a, intr, 0.05, 3.0, 0.5, grad_loss=1.5))


def test_no_grad_allocates_only_the_partials():
    shape = (4 * TH, 4 * TW)
    a, intr = noisy(shape, 6)
    x = gpu(a).requires_grad_(True)
    loss_g = surfel_losses.surfel_geometric_loss(x, intr)
    assert loss_g.requires_grad
    blocks = 16
    torch.cuda.synchronize()
    with torch.no_grad():
        surfel_losses.surfel_geometric_loss(x, intr)               # (warm: the library and the allocator's pools)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        (loss_n, _, _), st = surfel_losses.surfel_geometric_loss_with_state(x, intr)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    assert st.maps is None and not loss_n.requires_grad and torch.equal(loss_n, loss_g)
    # out [3] and 2 float64 partials per workgroup, each rounded up to the allocator's 512-byte granule: nothing of H x W
    assert peak <= 512 + 512 * ((16 * blocks + 511) // 512), peak
    assert peak < 4 * shape[0] * shape[1]


def test_non_contiguous_allmap():
    a, intr = noisy((40, 70), 7)
    base = gpu(np.ascontiguousarray(a.transpose(1, 2, 0))).requires_grad_(True)       # [H, W, 7]
    view = base.permute(2, 0, 1)
    assert not view.is_contiguous()
    loss = surfel_losses.surfel_geometric_loss(view, intr, 0.05, 3.0, 0.5)
    loss.backward()
    want = gm.loss_and_grad(a, intr, 0.05, 3.0, 0.5)
    assert gm.same_bits(host(loss), want["loss"])
    assert gm.same_bits(host(base.grad), want["grad"].transpose(1, 2, 0))


# ------------------------------------------------------------------------------------------------ with the operator
def _surfel_setup(sc, dev):
    from gaustudio_amd import GaussianRasterizationSettings
    cam = sc.cam
    rs = GaussianRasterizationSettings(sc.H, sc.W, cam.tanfovx, cam.tanfovy, sc.bg.to(dev), 1.0, cam.viewmatrix.to(dev),
                                       cam.projmatrix.to(dev), sc.D, cam.campos.to(dev), False, False)
    return rs


def _surfel_render(sc, rs, dev):
    from gaustudio_amd.surfel import GaussianRasterizer
    lv = {k: v.to(dev).requires_grad_(True) for k, v in sc.leaves.items()}
    color, radii, allmap = GaussianRasterizer(rs)(means3D=lv["means3D"], means2D=torch.zeros_like(lv["means3D"], requires_grad=True),
                                                 opacities=lv["opacities"], shs=lv.get("shs"), colors_precomp=lv.get("colors_precomp"),
                                                 scales=lv["scales"], rotations=lv["rotations"])
    return lv, radii, allmap


def test_allmap_from_the_surfel_operator():
    """allmap as an autograd output of the operator: the leaves' gradients equal what the operator's backward gives when handed
    the model's dL/dallmap directly."""
    import surfel_scenes as ss
    dev = torch.device("cuda", 0)
    sc = ss.ragged(31, 47)
    rs = _surfel_setup(sc, dev)
    intr = surfel_losses.intrinsics_from_settings(rs)
    la, _, allmap_a = _surfel_render(sc, rs, dev)
    assert allmap_a.shape == (7, 47, 31) and allmap_a.requires_grad
    surfel_losses.surfel_geometric_loss(allmap_a, intr, 0.05, 100.0, 0.5).backward()
    lb, _, allmap_b = _surfel_render(sc, rs, dev)
    assert torch.equal(allmap_a, allmap_b)
    want = gm.loss_and_grad(host(allmap_b), intr, 0.05, 100.0, 0.5)
    allmap_b.backward(gpu(want["grad"]))
    for k in la:
        assert (la[k].grad is None) == (lb[k].grad is None), k
        if la[k].grad is not None:
            assert torch.isfinite(la[k].grad).all() and torch.equal(la[k].grad, lb[k].grad), k
    assert la["means3D"].grad.abs().sum() > 0 and la["rotations"].grad.abs().sum() > 0


def test_end_to_end_against_the_torch_restatement():
    """means3D / opacities (and the other leaves) through operator + this loss against operator + the torch float32 restatement
    on the device, per surfel, within the tolerance tests/test_surfel_scenes.py derives for float32 against float64."""
    import surfel_checks as ck
    import surfel_scenes as ss
    from test_gpu_surfel_edges import PER_SURFEL_TOL
    from test_surfel_scenes import _ragged
    dev = torch.device("cuda", 0)
    sc, out = _ragged(129, 65)                                      # (the float64 model's radii, rects and event pixels)
    rs = _surfel_setup(sc, dev)
    intr = surfel_losses.intrinsics_from_settings(rs)
    args = (0.05, 100.0, 0.5)
    la, radii, allmap_a = _surfel_render(sc, rs, dev)
    surfel_losses.surfel_geometric_loss(allmap_a, intr, *args).backward()
    lb, _, allmap_b = _surfel_render(sc, rs, dev)
    r = parity.restatement(allmap_b, intr, *args, dtype=torch.float32, device=dev)
    assert torch.isfinite(r["grad"]).all()
    allmap_b.backward(r["grad"])
    names = ("means3D", "opacities", "scales", "rotations")
    g, ref = {k: la[k].grad for k in names}, {k: lb[k].grad for k in names}
    worst, where, share = ck.per_surfel_error(g, ref, out)
    print(f"per-surfel max {worst:.3g} at {where}, excluded {share:.2%}")
    assert share <= 0.25 and int((radii > 0).sum()) > 100
    assert all(float(ref[k].abs().sum()) > 0 for k in names)
    assert worst <= PER_SURFEL_TOL, f"per-surfel gradient error {worst:.3g} at {where}"


# ------------------------------------------------------------------------------------------- determinism and device
def test_two_runs_identical_and_stream_independent():
    shape = (5 * TH + 1, 3 * TW + 1)
    a, intr = noisy(shape, 8)
    x, y = run_hip(a, intr, 0.05, 3.0, 0.5), run_hip(a, intr, 0.05, 3.0, 0.5)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        z = run_hip(a, intr, 0.05, 3.0, 0.5)
    s.synchronize()
    for k in x:
        assert gm.same_bits(x[k], y[k]) and gm.same_bits(x[k], z[k]), k


def test_cpu_tensor_raises():
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        surfel_losses.surfel_geometric_loss(torch.rand(7, 8, 8), torch.tensor([10.0, 10.0, 4.0, 4.0]).cuda())


def test_c_abi_rejects_bad_arguments():
    """A negative status (-2), not a fault: bad sizes, depth_ratio, lambdas or intrinsics -- no kernel is launched."""
    import ctypes
    from gaustudio_amd._abi import call
    x = torch.rand(7, 4, 4, device="cuda")
    out = torch.empty(3, device="cuda")
    f = ctypes.c_float
    good = (10.0, 10.0, 1.5, 1.5, 0.0, 0.05, 0.0)
    cases = [(h, w) + good for h, w in ((0, 4), (4, 0), (-1, 4), (2 ** 15, 2 ** 14))]
    cases += [(4, 4) + good[:i] + (v,) + good[i + 1:] for i, v in ((0, 0.0), (1, 0.0), (0, float("nan")), (2, float("inf")),
                                                                   (4, -0.1), (4, 1.5), (4, float("nan")), (5, -1.0),
                                                                   (5, float("inf")), (6, float("nan")))]
    for h, w, *sc in cases:
        sc = [f(v) for v in sc]
        with pytest.raises(ValueError):
            call("gsr_surfel_geoloss_fwd", x.device, x, h, w, *sc, None, None, out, workspace=True, errors=surfel_losses._ERRORS)
        with pytest.raises(ValueError):
            call("gsr_surfel_geoloss_bwd", x.device, x, h, w, *sc, out, x, errors=surfel_losses._ERRORS)


# -------------------------------------------------------------------------------------------------------- example
def test_example_runs_and_its_loss_decreases():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_surfel_synthetic.py"), "40"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr                  # (the script asserts that the total went down)
    assert "total loss" in r.stdout and "->" in r.stdout
