"""GPU tests of gaustudio_amd.losses (csrc/gsr_loss.hip) against the float32 model tests/loss_model.py.

Every comparison with the model is EXACT (loss_model.same_bits: NaN in the same places, the bytes of everything else): loss,
l1, ssim, ssim_map, the three saved maps and the gradient.  The library is built without contraction and with correctly
rounded divides, and the model restates every operation and the float64 partial tree, so there is nothing to tolerate.
Shapes sit on the edges of the window (11) and of the workgroup's tile (losses.TILE_H x losses.TILE_W).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import loss_model as lm  # noqa: E402
import loss_model_parity as parity  # noqa: E402
from gaustudio_amd import losses  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
TH, TW = losses.TILE_H, losses.TILE_W

SHAPES = [(1, 1), (1, 11), (5, 3), (10, 10), (11, 11), (TH - 1, TW + 1), (TH, TW), (TH + 1, TW - 1), (2 * TH + 1, TW + 5),
          (1, 4 * TW + 3), (4 * TH + 3, 1)]
LEADS = [(), (3,), (2, 3)]


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def run_hip(x, y, lam=0.2, grad_loss=1.0):
    """Forward with state and backward through autograd; everything back on the host."""
    xi = gpu(x).requires_grad_(True)
    yt = gpu(y)
    (loss, l1, ssim), st = losses.photometric_loss_with_state(xi, yt, lam)
    (loss * grad_loss if grad_loss != 1.0 else loss).backward()
    smap = losses.ssim_map(xi, yt)
    return dict(loss=host(loss), l1=host(l1), ssim=host(ssim), ssim_map=host(smap), maps=host(st.maps), grad=host(xi.grad))


def check(x, y, lam=0.2, grad_loss=1.0):
    got = run_hip(x, y, lam, grad_loss)
    want = lm.loss_and_grad(x, y, lam, grad_loss)
    for k in ("loss", "l1", "ssim", "ssim_map", "maps", "grad"):
        assert got[k].dtype == F32
        assert lm.same_bits(got[k], want[k]), f"{k} differs from the model: max |d| = {np.nanmax(np.abs(got[k] - want[k]))}"
    return got, want


def uniform(shape, seed, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return ((hi - lo) * rng.random(shape, dtype=F32) + F32(lo)).astype(F32)


# --------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("lead", LEADS, ids=lambda l: "x".join(map(str, l)) or "plane")
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_exact(hw, lead):
    shape = tuple(lead) + tuple(hw)
    check(uniform(shape, 1), uniform(shape, 2))


def test_many_partials_exact():
    """10 x 10 tiles (the last row and column one pixel deep) on 3 planes: 300 workgroup partials, more than one pass of the
    final kernel's 256 lanes plus a ragged tail of 44."""
    shape = (3, 9 * TH + 1, 9 * TW + 1)
    assert 3 * 10 * 10 > 256
    check(uniform(shape, 3), uniform(shape, 4))


# --------------------------------------------------------------------------------------------------------- values
VSHAPE = (3, 2 * TH + 1, TW + 5)


def _values(name):
    x, y = uniform(VSHAPE, 5), uniform(VSHAPE, 6)
    if name == "unclamped":
        return uniform(VSHAPE, 7, -0.5, 1.5), uniform(VSHAPE, 8, -0.5, 1.5)
    if name == "constant":
        return (np.broadcast_to(np.array([0.25, 0.5, 1.0], F32)[:, None, None], VSHAPE).copy(),
                np.broadcast_to(np.array([0.75, 0.5, 0.0], F32)[:, None, None], VSHAPE).copy())
    if name == "checkerboard_ties":
        yy, xx = np.mgrid[0:VSHAPE[1], 0:VSHAPE[2]]
        return x, np.where((yy + xx) % 2 == 0, x, y)
    if name == "flat_halves":
        return parity.scene("flat_halves", VSHAPE[1:])
    return x, y


@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("name", ["uniform", "unclamped", "constant", "checkerboard_ties", "flat_halves"])
def test_values_exact(name, lam):
    x, y = _values(name)
    got, _ = check(x, y, lam)
    if name == "checkerboard_ties" and lam == 0.0:
        assert np.all(got["grad"][x == y] == 0)                    # sign(0) = 0
    if lam == 0.0:
        assert got["loss"] == got["l1"]


def test_identical_images():
    x = uniform(VSHAPE, 9)
    got, _ = check(x, x.copy())
    assert got["loss"] == 0 and got["l1"] == 0 and got["ssim"] == 1 and np.all(got["ssim_map"] == 1)


def test_one_nan_pixel():
    x, y = uniform(VSHAPE, 10), uniform(VSHAPE, 11)
    p, r, c = 1, 3, VSHAPE[2] - 2                                  # near two borders: the neighbourhood is clipped
    x[p, r, c] = np.nan
    got, _ = check(x, y)
    want = np.zeros(VSHAPE, bool)
    want[p, max(r - 5, 0):r + 6, max(c - 5, 0):c + 6] = True
    assert np.array_equal(np.isnan(got["ssim_map"]), want)
    assert np.isnan(got["loss"]) and np.isnan(got["l1"]) and np.isnan(got["ssim"])


def test_parts_are_the_same_bits():
    x, y = gpu(uniform(VSHAPE, 12)), gpu(uniform(VSHAPE, 13))
    loss, l1, ssim = losses.photometric_loss_with_parts(x, y, 0.35)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    assert torch.equal(losses.l1_loss(x, y), l1) and torch.equal(losses.ssim(x, y), ssim)
    assert torch.equal(losses.photometric_loss(x, y, 0.35), loss)


# ------------------------------------------------------------------------------------------------------- autograd
def test_scaled_and_reused_loss():
    x, y = uniform(VSHAPE, 14), uniform(VSHAPE, 15)
    check(x, y, 0.2, grad_loss=2.5)                                # (2.5 loss).backward()
    xi = gpu(x).requires_grad_(True)
    loss = losses.photometric_loss(xi, gpu(y))
    (loss + 0.5 * loss).backward()                                 # the loss twice in one graph: upstream 1 + 0.5
    m = lm.forward(x, y)
    assert lm.same_bits(host(xi.grad), lm.backward(x, y, m["maps"], 0.2, grad_loss=1.5))


def test_no_grad_allocates_no_maps():
    x, y = gpu(uniform(VSHAPE, 16)), gpu(uniform(VSHAPE, 17))
    xr = x.clone().requires_grad_(True)
    (loss_g, _, _), st_g = losses.photometric_loss_with_state(xr, y)
    assert st_g.maps is not None and st_g.maps.shape == (3,) + VSHAPE and loss_g.requires_grad
    with torch.no_grad():
        (loss_n, _, _), st_n = losses.photometric_loss_with_state(xr, y)
    assert st_n.maps is None and st_n.ssim_map is None and not loss_n.requires_grad
    (loss_d, _, _), st_d = losses.photometric_loss_with_state(x, y)       # nothing requires a gradient
    assert st_d.maps is None
    assert torch.equal(loss_g, loss_n) and torch.equal(loss_g, loss_d)


def test_non_contiguous_image():
    x, y = uniform((3, 40, 70), 18), uniform((3, 70, 40), 19)
    xt = gpu(x).requires_grad_(True)
    view = xt.transpose(1, 2)
    assert not view.is_contiguous()
    loss = losses.photometric_loss(view, gpu(y))
    loss.backward()
    xc = np.ascontiguousarray(x.transpose(0, 2, 1))
    want = lm.loss_and_grad(xc, y)
    assert lm.same_bits(host(loss), want["loss"])
    assert lm.same_bits(host(xt.grad), want["grad"].transpose(0, 2, 1))


def test_backward_through_the_rasterizer():
    """means3D.grad etc. equal what the rasterizer's backward gives when handed the model's dL/dimage directly."""
    from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, scenes
    dev = torch.device("cuda", 0)
    cam = scenes.make_camera(48, 40)
    sc = scenes.make_scene(600, cam, seed=3, sigma_px_median=2.5)
    rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0,
                                       cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 3, cam.campos.to(dev), False, False)
    target = gpu(uniform((3, 40, 48), 20))
    names = ("means3D", "scales", "rotations", "opacities", "shs")

    def render():
        leaves = {k: getattr(sc, k).to(dev).requires_grad_(True) for k in names}
        color = GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=torch.zeros_like(leaves["means3D"], requires_grad=True),
                                       opacities=leaves["opacities"], shs=leaves["shs"], scales=leaves["scales"],
                                       rotations=leaves["rotations"])[0]
        return leaves, color

    la, color_a = render()
    assert color_a.shape == (3, 40, 48)
    losses.photometric_loss(color_a, target).backward()
    lb, color_b = render()
    assert torch.equal(color_a, color_b)
    g = lm.loss_and_grad(host(color_b), host(target))["grad"]
    color_b.backward(gpu(g))
    for k in names:
        assert la[k].grad is not None and la[k].grad.abs().sum() > 0
        assert torch.equal(la[k].grad, lb[k].grad), k


# ------------------------------------------------------------------------------------------- determinism and device
def test_two_runs_identical_and_stream_independent():
    shape = (3, 9 * TH + 1, 3 * TW + 1)
    x, y = uniform(shape, 21), uniform(shape, 22)
    a, b = run_hip(x, y), run_hip(x, y)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c = run_hip(x, y)
    s.synchronize()
    for k in a:
        assert lm.same_bits(a[k], b[k]) and lm.same_bits(a[k], c[k]), k


def test_cpu_tensor_raises():
    x, y = torch.rand(3, 8, 8), torch.rand(3, 8, 8)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        losses.photometric_loss(x.cuda(), y)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        losses.photometric_loss(x, y.cuda())


def test_mismatched_devices_raise():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second device")
    x, y = torch.rand(3, 8, 8, device="cuda:0"), torch.rand(3, 8, 8, device="cuda:1")
    with pytest.raises(ValueError):
        losses.photometric_loss(x, y)


def test_c_abi_rejects_bad_sizes():
    """A negative status, not a fault: H or W < 1, a plane or element count beyond int32 -- no kernel is launched."""
    import ctypes
    from gaustudio_amd._abi import call
    x = torch.rand(1, 4, 4, device="cuda")
    out = torch.empty(3, device="cuda")
    for planes, h, w in ((1, 0, 4), (1, 4, 0), (1, -1, 4), (0, 4, 4), (2 ** 31, 1, 1), (2 ** 16, 2 ** 8, 2 ** 8)):
        with pytest.raises(ValueError):
            call("gsr_photometric_fwd", x.device, x, x, ctypes.c_longlong(planes), h, w, ctypes.c_float(0.2), None, None, out,
                 workspace=True, errors=losses._ERRORS)
        with pytest.raises(ValueError):
            call("gsr_photometric_bwd", x.device, x, x, x, ctypes.c_longlong(planes), h, w, ctypes.c_float(0.2), out, x,
                 errors=losses._ERRORS)


# -------------------------------------------------------------------------------------------------------- example
def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fit_photometric_synthetic.py"), "20"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "->" in r.stdout
