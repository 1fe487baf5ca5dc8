"""CPU tests of the photometric loss's definition (tests/loss_model.py) and of the Python boundary of gaustudio_amd.losses.

The float32 model -- the kernels' arithmetic to the bit -- is held against the float64 restatement of the published formula.
Its allowed error is measured, not invented: on each scene it may be at most 2x the error of torch's own float32 evaluation of
the same conv2d formula (what everyone trains with today) on |loss - loss64|, max |ssim_map - ssim_map64| and
max |grad - grad64| / max |grad64|.  The two float32 evaluations differ in summation order (11 + 11 separable taps against
121), so the errors are of one order, not equal; `python tests/loss_model_parity.py` writes both sides' figures to
profiles/photometric_loss_parity.json.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loss_model as lm  # noqa: E402
import loss_model_parity as parity  # noqa: E402
from gaustudio_amd import losses  # noqa: E402

F32 = np.float32


# ------------------------------------------------------------------------------------- float32 model against float64
@pytest.fixture(scope="module")
def report():
    return parity.measure()


@pytest.mark.parametrize("name", [f"{s}-{h}x{w}" for s in parity.SCENES for h, w in parity.SHAPES])
def test_model_error_within_twice_torch_float32(report, name):
    r = report[name]
    print(name, r)
    for k in ("loss", "ssim_map", "grad_over_scale"):
        assert r["model"][k] <= 2.0 * r["torch_float32"][k], f"{name}: {k} model {r['model'][k]:.3e} torch {r['torch_float32'][k]:.3e}"


@pytest.mark.parametrize("shape", parity.SHAPES)
def test_identical_images(shape):
    """The float64 gradient is ~1e-18 here, a ratio means nothing: exact statements instead."""
    x = parity.scene("noise", shape)[0]
    m = lm.loss_and_grad(x, x.copy())
    assert np.all(m["ssim_map"] == F32(1))
    assert m["loss"] == 0 and m["l1"] == 0 and m["ssim"] == 1
    assert np.all(lm.backward(x, x, m["maps"], lambda_dssim=0.0) == 0)          # the L1 gradient alone
    assert np.abs(m["grad"]).max() <= 1e-6


# ------------------------------------------------------------------------------------------------------- hand cases
def test_one_pixel_closed_form():
    """1 x 1: only the centre tap of either pass sees the pixel, the window reduces to c = g[5]^2."""
    a, b, lam = 0.7, 0.4, 0.2
    m = lm.loss_and_grad(np.full((1, 1), a, F32), np.full((1, 1), b, F32), lam)
    g5 = lm.WINDOW[5]
    assert m["ssim_map"].shape == (1, 1)
    # the float32 chain itself: g5 * (g5 * a), the other ten taps add +0
    mu1, mu2 = g5 * (g5 * F32(a)), g5 * (g5 * F32(b))
    e11, e22, e12 = g5 * (g5 * (F32(a) * F32(a))), g5 * (g5 * (F32(b) * F32(b))), g5 * (g5 * (F32(a) * F32(b)))
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    S32 = ((F32(2) * (mu1 * mu2) + lm.C1) * (F32(2) * s12 + lm.C2)) / (((mu1 * mu1 + mu2 * mu2) + lm.C1) * ((s1 + s2) + lm.C2))
    assert m["ssim_map"][0, 0] == S32 and m["ssim"] == S32
    assert m["l1"] == abs(F32(a) - F32(b))
    # the closed form in float64, a and b as the float32 values the model was given
    a, b, c = float(F32(a)), float(F32(b)), float(g5) ** 2
    C1, C2 = 1e-4, 9e-4
    m1, m2 = c * a, c * b
    v1, v2, v12 = c * a * a - m1 * m1, c * b * b - m2 * m2, c * a * b - m1 * m2
    A1, A2, B1, B2 = 2 * m1 * m2 + C1, 2 * v12 + C2, m1 * m1 + m2 * m2 + C1, v1 + v2 + C2
    S = A1 * A2 / (B1 * B2)
    dA = 2 * m2 * A2 / (B1 * B2) - 2 * m1 * A1 * A2 / (B1 * B1 * B2)
    dB = -A1 * A2 / (B1 * B2 * B2)
    dD = 2 * A1 / (B1 * B2)
    dS_da = c * (dA - 2 * m1 * dB - m2 * dD) + 2 * a * c * dB + b * c * dD
    loss = (1 - float(F32(lam))) * abs(a - b) + float(F32(lam)) * (1 - S)
    grad = (1 - float(F32(lam))) * 1.0 - float(F32(lam)) * dS_da
    assert float(m["ssim"]) == pytest.approx(S, rel=1e-5)
    assert float(m["loss"]) == pytest.approx(loss, rel=1e-5)
    assert float(m["grad"][0, 0]) == pytest.approx(grad, rel=1e-4)


def test_constant_images_closed_form():
    """Away from the borders a constant image has mu = value (the window sums to 1) and zero variance:
    ssim_map = (2ab + C1) / (a^2 + b^2 + C1).  Tolerance: s = E[x^2] - mu^2 cancels two numbers of size a^2 that carry a few
    float32 roundings each (eleven taps twice, the square, the difference: under 16 half-ulps), and that error stands against
    C2 = 9e-4 alone in s1 + s2 + C2 and 2 s12 + C2: |dS| <= S * 2 * 16 * 2^-24 (a^2 + b^2) / C2."""
    a, b = 0.6, 0.4
    m = lm.forward(np.full((2, 30, 40), a, F32), np.full((2, 30, 40), b, F32))
    S = (2 * a * b + 1e-4) / (a * a + b * b + 1e-4)
    tol = S * 2 * 16 * 2.0 ** -24 * (a * a + b * b) / 9e-4
    inner = m["ssim_map"][:, 5:-5, 5:-5]
    assert np.abs(inner - S).max() <= tol
    assert float(m["l1"]) == pytest.approx(abs(a - b), rel=1e-6)


def test_lambda_ends():
    x, y = parity.scene("noise", (37, 53))
    l0, l1 = lm.forward(x, y, 0.0), lm.forward(x, y, 1.0)
    assert l0["loss"] == l0["l1"]                                  # (1 - 0) l1 + 0 (1 - ssim), exactly
    assert float(l1["loss"]) == pytest.approx(1.0 - float(l1["ssim"]), abs=2.0 ** -23)
    assert l0["l1"] == l1["l1"] and l0["ssim"] == l1["ssim"]       # the parts do not depend on lambda


def test_sign_zero_pixels_get_no_l1_gradient():
    x, y = parity.scene("noise", (37, 53))
    tie = np.zeros(x.shape, bool)
    tie[:, ::2, ::3] = True
    y = np.where(tie, x, y)
    m = lm.forward(x, y, 0.0)
    g = lm.backward(x, y, m["maps"], 0.0, grad_loss=2.5)
    assert np.all(g[tie] == 0)
    w = F32(1.0 / x.size)
    assert np.array_equal(g[~tie], (F32(2.5) * (w * np.sign(x - y)))[~tie])


# ---------------------------------------------------------------------------------------------------------- window
def test_window_table():
    g = np.array([math.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)])
    g /= g.sum()
    assert np.array_equal(lm.WINDOW, g.astype(F32))                # float64, rounded once
    assert np.array_equal(lm.WINDOW, lm.WINDOW[::-1])
    assert abs(lm.WINDOW.astype(np.float64).sum() - 1.0) <= 2.0 ** -23
    assert (losses.TILE_H, losses.TILE_W) == (lm.TH, lm.TW)


def test_tile_partials_cover_every_pixel_once():
    """Integers sum exactly in any order: the tree must return the plain sum."""
    v = np.arange(3 * 37 * 150, dtype=F32).reshape(3, 37, 150) % 7
    p = lm.tile_partials(v)
    assert len(p) == 3 * 3 * 3 and lm.final_sum(p) == v.astype(np.float64).sum()
    assert lm.final_sum(np.ones(700)) == 700


# ------------------------------------------------------------------------------------------------- Python boundary
def test_boundary_errors_need_no_device():
    x, y = torch.rand(3, 8, 9), torch.rand(3, 8, 9)
    fns = (losses.photometric_loss, losses.photometric_loss_with_parts, losses.l1_loss, losses.ssim, losses.ssim_map)
    for f in fns:
        with pytest.raises(TypeError):
            f(x.numpy(), y)
        with pytest.raises(TypeError):
            f(x, None)
        with pytest.raises(ValueError):
            f(x, y[:, :, :8])
        with pytest.raises(ValueError):
            f(x[0, 0], y[0, 0])                                     # fewer than two dimensions
        with pytest.raises(TypeError):
            f(x.double(), y.double())
        with pytest.raises(TypeError):
            f(x, y.half())
        with pytest.raises(ValueError):
            f(x[:, :0], y[:, :0])                                   # empty
        with pytest.raises(NotImplementedError):
            f(x, y.clone().requires_grad_(True))
        with pytest.raises(RuntimeError, match="ROCm devices only"):
            f(x, y)                                                 # CPU tensors: on_rocm
    for lam in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            losses.photometric_loss(x, y, lam)
        with pytest.raises(ValueError):
            losses.photometric_loss_with_parts(x, y, lam)
    with pytest.raises(TypeError):
        losses.photometric_loss(x, y, "0.2")


def test_exported_from_the_package():
    import gaustudio_amd
    for n in ("photometric_loss", "photometric_loss_with_parts", "l1_loss", "ssim", "ssim_map"):
        assert getattr(gaustudio_amd, n) is getattr(losses, n)
