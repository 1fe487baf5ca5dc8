"""CPU tests of the surfel geometric loss's definition (tests/geoloss_model.py) and of the Python boundary of
gaustudio_amd.surfel_losses.

The float32 model -- the kernels' arithmetic to the bit -- is held against the float64 restatement of the published formula
(geoloss_model_parity.restatement: torch, autograd).  Its allowed error is measured, not invented: on each scene it may be at
most 2x the error of torch's own float32 evaluation of the same restatement on |loss - loss64|, max |normal_error - its float64|
and, per gradient group, max |grad - grad64| / max |grad64| (the factor tests/test_loss_model.py gives).  Both float32
evaluations form the same differences of neighbouring points in the same order, so the errors are nearly equal;
`python tests/geoloss_model_parity.py` writes both sides' figures to profiles/geometric_loss_parity.json.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import geoloss_model as gm  # noqa: E402
import geoloss_model_parity as parity  # noqa: E402
from gaustudio_amd import scenes, surfel_losses  # noqa: E402

F32 = np.float32
INTR = (40.0, 42.0, 3.2, 2.7)


# ------------------------------------------------------------------------------------- float32 model against float64
@pytest.fixture(scope="module")
def report():
    return parity.measure()


@pytest.mark.parametrize("name", [f"{s}-{h}x{w}-rho{r}" for s in parity.SCENES for h, w in parity.SHAPES for r in parity.RHOS])
def test_model_error_within_twice_torch_float32(report, name):
    r = report[name]
    print(name, r)
    assert r["min_c"] > parity.C_FLOOR                 # no pixel near the clamp of the normalisation: none is excluded
    for k in ("loss", "normal_error", "grad_depth_over_scale", "grad_normal_over_scale"):
        assert r["model"][k] <= 2.0 * r["torch_float32"][k], f"{name}: {k} model {r['model'][k]:.3e} torch {r['torch_float32'][k]:.3e}"


def test_parity_scenes_are_what_they_claim():
    for s in parity.SCENES:
        a, _ = parity.scene(s, parity.SHAPES[0])
        assert a.dtype == F32 and a[1].min() > 0.2 and a[1].max() <= 1.0 and np.isfinite(a).all()
        assert a[0].min() > 0 and np.abs(np.linalg.norm(a[2:5], axis=0) - 1).max() < 0.3


# ------------------------------------------------------------------------------------------------------- hand cases
def plane_allmap(H, W, depth=2.0, alpha=1.0):
    a = np.zeros((7, H, W), F32)
    a[0], a[1], a[4], a[5] = depth * alpha, alpha, -1.0, depth
    return a


@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_fronto_parallel_plane(alpha):
    H, W, lam = 9, 12, 0.05
    a = plane_allmap(H, W, 2.0, alpha)
    m = gm.loss_and_grad(a, INTR, lam)
    inner = m["surf_normal"][:, 1:-1, 1:-1]
    assert np.all(inner[0] == 0) and np.all(inner[1] == 0) and np.all(inner[2] == F32(-alpha))
    border = np.ones((H, W), bool)
    border[1:-1, 1:-1] = False
    assert np.all(m["surf_normal"][:, border] == 0) and np.all(m["normal_error"][border] == 1)
    assert np.all(m["normal_error"][~border] == F32(1 - alpha))
    if alpha == 1.0:
        nb = int(border.sum())
        assert nb == H * W - (H - 2) * (W - 2)
        assert m["normal_loss"] == F32(np.float64(F32(lam)) * (nb / (H * W)))
        assert m["loss"] == m["normal_loss"] and m["dist_loss"] == 0


@pytest.mark.parametrize("shape", [(1, 1), (2, 5), (5, 2), (1, 9)])
def test_no_interior_pixel(shape):
    rng = np.random.default_rng(3)
    a = rng.random((7,) + shape, dtype=F32) + F32(0.5)
    lam = 0.3
    m = gm.loss_and_grad(a, INTR, lam, 0.0)
    assert m["normal_loss"] == F32(lam) and m["loss"] == F32(lam)
    assert np.all(m["grad"][:6] == 0) and np.all(m["grad"][6] == 0)
    m = gm.loss_and_grad(a, INTR, lam, 2.0)
    assert np.all(m["grad"][:6] == 0) and np.all(m["grad"][6] == F32(2.0 / (shape[0] * shape[1])))


def test_zero_alpha_pixels_are_finite():
    a, intr = parity.scene("sphere_cap", (20, 30))
    hole = np.zeros((20, 30), bool)
    hole[5:9, 10:14] = True
    hole[0, 0] = hole[19, 29] = True
    a[1][hole] = 0.0                                   # a0 / 0 = +inf
    a[0][6, 11] = 0.0                                  # 0 / 0 = NaN
    a[0][7, 12] = -a[0][7, 12]                         # -inf
    for rho in (0.0, 0.5):
        m = gm.loss_and_grad(a, intr, 0.05, 10.0, rho)
        assert np.all(m["rendered_depth"][0][hole] == 0)
        if rho == 0.0:
            assert np.all(m["surf_depth"][0][hole] == 0)
        assert np.all(m["grad"][0][hole] == 0) and np.all(m["grad"][1][hole] == 0)
        for k in ("loss", "normal_loss", "dist_loss", "maps", "grad"):
            assert np.isfinite(m[k]).all(), k
        # the restatement pins the same zeros, and away from them the two agree
        r = parity.restatement(a, intr, 0.05, 10.0, rho)
        g64 = r["grad"].numpy()
        assert np.all(g64[0][hole] == 0) and np.all(g64[1][hole] == 0) and np.isfinite(g64).all()
        assert float(m["loss"]) == pytest.approx(float(r["loss"]), rel=1e-5)
        assert np.abs(m["grad"] - g64).max() <= 1e-3 * np.abs(g64).max()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_median(bad):
    a, intr = parity.scene("tilted_plane", (12, 17))
    a[5][4, 6] = bad
    a[5][0, 3] = bad
    for rho in (0.5, 1.0):
        m = gm.loss_and_grad(a, intr, 0.05, 0.0, rho)
        assert m["rendered_median_depth"][0][4, 6] == 0 and m["grad"][5][4, 6] == 0 and m["grad"][5][0, 3] == 0
        assert np.isfinite(m["loss"]) and np.isfinite(m["grad"]).all() and np.isfinite(m["maps"]).all()
        r = parity.restatement(a, intr, 0.05, 0.0, rho)
        assert float(m["loss"]) == pytest.approx(float(r["loss"]), rel=1e-5)
        assert np.abs(m["grad"] - r["grad"].numpy()).max() <= 1e-3 * np.abs(r["grad"].numpy()).max()
    m0 = gm.loss_and_grad(a, intr, 0.05, 0.0, 0.0)        # rho = 0: the median is not looked at
    assert np.all(m0["grad"][5] == 0) and np.isfinite(m0["loss"])


def test_depth_ratio_ends():
    a, intr = parity.scene("sphere_cap", (14, 19))
    m0, m5, m1 = (gm.loss_and_grad(a, intr, 0.05, 0.0, r) for r in (0.0, 0.5, 1.0))
    assert np.array_equal(m0["surf_depth"], m0["rendered_depth"]) and np.array_equal(m1["surf_depth"], m1["rendered_median_depth"])
    assert np.all(m0["grad"][5] == 0) and np.all(m1["grad"][0] == 0) and np.all(m1["grad"][1] == 0)
    assert np.abs(m5["grad"][0]).max() > 0 and np.abs(m5["grad"][5]).max() > 0
    assert np.array_equal(m5["surf_depth"], F32(0.5) * m5["rendered_depth"] + F32(0.5) * m5["rendered_median_depth"])


def test_lambda_zero_terms():
    a, intr = parity.scene("tilted_plane", (14, 19))
    m = gm.loss_and_grad(a, intr, 0.0, 3.0)
    assert m["normal_loss"] == 0 and m["loss"] == m["dist_loss"] and np.all(m["grad"][:6] == 0)
    assert np.all(m["grad"][6] == F32(3.0 / (14 * 19)))
    m = gm.loss_and_grad(a, intr, 0.7, 0.0)
    assert m["dist_loss"] == 0 and m["loss"] == m["normal_loss"] and np.all(m["grad"][6] == 0)
    assert np.abs(m["grad"][:6]).max() > 0
    both = gm.forward(a, intr, 0.7, 3.0)
    assert both["normal_loss"] == m["normal_loss"]                 # the parts do not depend on the other lambda


def test_all_zero_depth():
    """c = 0 through a = b = 0: the clamped branch, n = 0 / eps = 0, and dL/dc = g / eps is finite and meets da/dd = 0."""
    a = np.zeros((7, 6, 7), F32)
    a[1] = 0.5
    a[2:5] = 0.3
    m = gm.loss_and_grad(a, INTR, 0.05, 0.0)
    assert np.all(m["surf_normal"] == 0) and np.all(m["normal_error"] == 1) and m["normal_loss"] == F32(0.05)
    assert np.all(m["grad"] == 0) and np.isfinite(m["grad"]).all()


def test_nan_normal_reaches_the_loss():
    a, intr = parity.scene("tilted_plane", (12, 17))
    a[3][0, 5] = np.nan                                # a border pixel: N * 0 is still NaN, as in torch
    m = gm.forward(a, intr)
    assert np.isnan(m["loss"]) and np.isnan(m["normal_loss"]) and m["dist_loss"] == 0
    assert np.isnan(float(parity.restatement(a, intr)["loss"]))


def test_viewmatrix_turns_both_normals():
    a, intr = parity.scene("sphere_cap", (10, 13))
    cam = scenes.look_at_camera(13, 10, (1.0, -2.0, -3.0), (0.0, 0.2, 0.4))
    V = cam.viewmatrix.numpy()
    m, mw = gm.forward(a, intr), gm.forward(a, intr, viewmatrix=V)
    want = np.einsum("ihw,ji->jhw", m["rendered_normal"].astype(np.float64), V[:3, :3].astype(np.float64))   # v @ V[:3,:3].T
    assert np.abs(mw["rendered_normal"] - want).max() < 1e-6
    want = np.einsum("ihw,ji->jhw", m["surf_normal"].astype(np.float64), V[:3, :3].astype(np.float64))
    assert np.abs(mw["surf_normal"] - want).max() < 1e-6
    assert np.array_equal(mw["normal_error"], m["normal_error"]) and mw["loss"] == m["loss"]


# ------------------------------------------------------------------------------------------------- finite differences
def test_finite_differences_of_the_restatement():
    """Central differences of the float64 restatement on a 6 x 7 map against its autograd gradient, and the model beside it."""
    a, intr = parity.scene("sphere_cap", (6, 7))
    args = (0.05, 2.0, 0.5)
    a64 = a.astype(np.float64)
    r = parity.restatement(a64, intr, *args)
    g = r["grad"].numpy()
    h = 1e-6
    fd = np.zeros_like(a64)
    for idx in np.ndindex(a64.shape):
        p, q = a64.copy(), a64.copy()
        p[idx] += h
        q[idx] -= h
        # alpha is a constant in the factor n * alpha: the restatement detaches it, so the difference quotient must too
        fd[idx] = (_loss_alpha_fixed(p, a64, intr, *args) - _loss_alpha_fixed(q, a64, intr, *args)) / (2 * h)
    assert np.abs(fd - g).max() <= 1e-6 * np.abs(g).max() + 1e-9
    m = gm.backward(a, intr, *args)
    assert np.abs(m - g).max() <= 1e-4 * np.abs(g).max()


def _loss_alpha_fixed(a, a_ref, intr, ln, ld, rho):
    """The restatement's loss with the detached alpha factor taken from a_ref."""
    r = parity.restatement(a, intr, ln, ld, rho)
    n = r["surf_normal"].numpy() / np.where(a[1] != 0, a[1], 1.0) * a_ref[1]
    err = 1.0 - (a[2:5] * n).sum(0)
    return ln * err.mean() + ld * a[6].mean()


# ------------------------------------------------------------------------------------------------ intrinsics_from_settings
def _settings(cam):
    from gaustudio_amd import GaussianRasterizationSettings
    return GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0, cam.viewmatrix,
                                         cam.projmatrix, 3, cam.campos, False, False)


@pytest.mark.parametrize("W,H", [(64, 48), (53, 37)])
def test_intrinsics_against_make_camera(W, H):
    cam = scenes.make_camera(W, H)
    fx, fy, cx, cy = surfel_losses.intrinsics_from_settings(_settings(cam))
    assert fx == pytest.approx(W / (2 * cam.tanfovx), rel=1e-6) and fy == pytest.approx(H / (2 * cam.tanfovy), rel=1e-6)
    assert cx == pytest.approx((W - 1) / 2, abs=1e-5) and cy == pytest.approx((H - 1) / 2, abs=1e-5)


def test_intrinsics_against_the_operators_projection():
    """A point built from (pixel, depth) with the derived intrinsics, taken to world space and projected with the operator's
    own formula h.x = c.x W / 2 + c.w (W - 1) / 2, lands on that pixel."""
    W, H = 61, 45
    cam = scenes.look_at_camera(W, H, (0.5, -1.0, -4.0), (0.1, 0.0, 0.5))
    fx, fy, cx, cy = surfel_losses.intrinsics_from_settings(_settings(cam))
    view, full = cam.viewmatrix.double(), cam.projmatrix.double()
    rng = np.random.default_rng(0)
    for _ in range(20):
        x, y, d = rng.uniform(0, W - 1), rng.uniform(0, H - 1), rng.uniform(0.5, 20.0)
        p_cam = torch.tensor([d * (x - cx) / fx, d * (y - cy) / fy, d, 1.0], dtype=torch.float64)
        p_world = p_cam @ torch.inverse(view)
        c = p_world @ full
        hx = c[0] * W / 2 + c[3] * (W - 1) / 2
        hy = c[1] * H / 2 + c[3] * (H - 1) / 2
        assert float(hx / c[3]) == pytest.approx(x, abs=1e-4) and float(hy / c[3]) == pytest.approx(y, abs=1e-4)
        assert float(c[3]) == pytest.approx(d, rel=1e-5)


# ------------------------------------------------------------------------------------------------- Python boundary
def test_boundary_errors_need_no_device():
    a = torch.rand(7, 8, 9)
    intr = (10.0, 10.0, 4.0, 3.5)
    fns = (surfel_losses.surfel_geometric_loss, surfel_losses.surfel_geometric_loss_with_parts)
    for f in fns + (surfel_losses.surfel_maps,):
        with pytest.raises(TypeError):
            f(a.numpy(), intr)                                      # 1. types
        with pytest.raises(TypeError):
            f(a, None)
        with pytest.raises(TypeError):
            f(a, ("10", 10.0, 4.0, 3.5))
        with pytest.raises(TypeError):
            f(a, intr, depth_ratio="0")
        with pytest.raises(ValueError):
            f(a[:6], intr)                                          # 2. shape
        with pytest.raises(ValueError):
            f(a[None], intr)
        with pytest.raises(ValueError):
            f(a, intr[:3])
        with pytest.raises(TypeError):
            f(a.double(), intr)                                     # 3. dtype
        with pytest.raises(ValueError):
            f(a[:, :0], intr)                                       # 4. empty
        for rho in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="depth_ratio"):
                f(a, intr, depth_ratio=rho)                         # 5.
        for bad in ((0.0, 10.0, 4.0, 3.5), (10.0, 0.0, 4.0, 3.5), (float("nan"), 10.0, 4.0, 3.5), (10.0, float("inf"), 4.0, 3.5),
                    torch.tensor([10.0, 1e-60, 4.0, 3.5], dtype=torch.float64)):
            with pytest.raises(ValueError, match="intrinsics"):
                f(a, bad)                                           # 7.
        with pytest.raises(RuntimeError, match="ROCm devices only"):
            f(a, intr)                                              # 8. CPU tensors: on_rocm
        with pytest.raises(RuntimeError, match="ROCm devices only"):
            f(a, torch.tensor(intr))
    for f in fns:
        with pytest.raises(TypeError):
            f(a, intr, "0.05")
        with pytest.raises(TypeError):
            f(a, intr, 0.05, None)
        for lam in (-0.1, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="lambda_normal"):
                f(a, intr, lam)                                     # 6.
            with pytest.raises(ValueError, match="lambda_dist"):
                f(a, intr, 0.05, lam)
        with pytest.raises(ValueError, match="depth_ratio"):        # the order: depth_ratio before the lambdas before fx
            f(a, (0.0, 1.0, 0.0, 0.0), -1.0, 0.0, 2.0)
        with pytest.raises(ValueError, match="lambda_normal"):
            f(a, (0.0, 1.0, 0.0, 0.0), -1.0, 0.0, 0.5)
    with pytest.raises(TypeError):
        surfel_losses.surfel_maps(a, intr, viewmatrix=np.eye(4))
    with pytest.raises(ValueError):
        surfel_losses.surfel_maps(a, intr, viewmatrix=torch.eye(3))


def test_huge_allmap_is_refused_without_memory():
    a = torch.empty(7, 1, 1).expand(7, 2 ** 15, 2 ** 14)            # 7 * 2^29 >= 2^31 elements, no storage behind them
    with pytest.raises(ValueError, match="2\\^31"):
        surfel_losses.surfel_geometric_loss(a, (10.0, 10.0, 4.0, 3.5))


def test_exported_from_the_package():
    import gaustudio_amd
    for n in ("surfel_geometric_loss", "surfel_geometric_loss_with_parts", "surfel_maps", "intrinsics_from_settings"):
        assert getattr(gaustudio_amd, n) is getattr(surfel_losses, n)
    assert (surfel_losses.TILE_H, surfel_losses.TILE_W) == (gm.TH, gm.TW)
    assert math.isclose(float(gm.EPS), 1e-12, rel_tol=1e-6)
