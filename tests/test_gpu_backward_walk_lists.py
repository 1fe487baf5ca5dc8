"""-m gpu: composite_bwd's per-quarter walk lists, their contributor threshold and its two walk loops.

A quarter's list holds 16-bit entries: the staged instance's batch index times 16, which a walk step uses as the LDS offset of
the record as it is; the sentinel is entry 128 * 16.  `contributor < last_contributor` is one compare of the entry with a per-lane
threshold 16 * (top - 1 - last_contributor) that moves by a batch per round.  A wave whose pixels have a background term
(background . dL_dpixel != 0 somewhere in its 8x8 pixels) walks a loop with that term, every other wave a loop without it.  Phase 2
starts its row sums from the first pixel's value (no 0 + x), which can change the sign of a zero sum and must not change a bit of
what is returned.

The scenes are the smallest that reach each of these (one tile, 16x16, and a ragged 20x27 image), with the distinct-field
anisotropic splats of tests/test_gpu_backward_record_layout.py, so that a record fetched from a neighbouring slot is off by a
factor; their properties are asserted on the CPU oracle's forward before the GPU runs.  Checks: those of
tests/test_gpu_backward.py::_check (the summation bound against the oracle, the bit-exact per-Gaussian stage, the banded backward
equal to the one call) and of the round tests' colour-only check."""
import numpy as np
import pytest
import torch

import gaustudio_amd
from gaustudio_amd import scenes

import test_gpu_backward
from test_gpu_backward import GRAD_KEYS, _check
from test_gpu_backward_record_layout import _powers, _scaled_output_grads, _splats
from test_gpu_backward_rounds import _check_colour_only, _tile_stats
from util import assert_bits_equal, hip_backward_raw, hip_forward, oracle_forward, scene_kwargs, to_np

pytestmark = pytest.mark.gpu

IMAGES = {"1tile": (16, 16), "ragged": (20, 27)}
LENGTHS = (1, 2, 127, 128, 129, 257)   # batch index 0, index 127 (the last before the sentinel), a round boundary, three rounds
BATCH = 128                            # instances staged per round (GSR_BWQ_BATCH)
BG = torch.tensor([0.3, 0.55, 0.8])
SMALL_BLOCKS = ((0, 0), (1, 0), (0, 1), (2, 2), (3, 1))   # the 4x4 blocks (of tile 0) that get one-block splats: five of sixteen


def _part_zero_grads(cam, seed=1):
    """_scaled_output_grads with the colour gradient zero for x < 8: the waves of the left 8x8 regions have no background term
    (background . dL_dpixel == 0 in all 64 pixels) and walk the loop without it, their neighbours in the same workgroup the other."""
    g = list(_scaled_output_grads(cam, seed))
    g[0] = g[0].clone()
    g[0][:, :, :8] = 0.0
    return tuple(g)


GRADS = {"dense": _scaled_output_grads, "part_zero": _part_zero_grads}


@pytest.fixture
def upstream(monkeypatch):
    """_check and _check_colour_only draw their upstream gradients from scenes.make_output_grads."""
    def use(kind):
        monkeypatch.setattr(scenes, "make_output_grads", GRADS[kind] if isinstance(kind, str) else kind)
    use("dense")
    return use


@pytest.fixture
def device_background(monkeypatch):
    """_check hands one `bg` to the oracle (host) and to the library; here the library's copy is moved to the device, which takes
    the other branch of GsBg (a device pointer instead of three host values)."""
    def fwd(sc, cam, D, kw, scale_modifier=1.0, bg=None, *a, **k):
        return hip_forward(sc, cam, D, kw, scale_modifier, None if bg is None else bg.cuda(), *a, **k)

    def bwd(hs, sc, cam, D, kw, grads, scale_modifier=1.0, bg=None, *a, **k):
        return hip_backward_raw(hs, sc, cam, D, kw, grads, scale_modifier, None if bg is None else bg.cuda(), *a, **k)

    def use():
        monkeypatch.setattr(test_gpu_backward, "hip_forward", fwd)
        monkeypatch.setattr(test_gpu_backward, "hip_backward_raw", bwd)
    return use


def _colour_only_with_background(oracle, sc, cam, D, kw, seed, bg, bg_lib):
    """_check_colour_only with a background: the CONLY instantiation bit-equal to explicit zero planes, the summation bound and
    the bit-exact per-Gaussian stage against an oracle that was given the zeros."""
    full = scenes.make_output_grads(cam, seed=seed)
    os_ = oracle_forward(oracle, sc, cam, D, kw, 1.0, bg)
    ob = oracle.backward(os_, full[0].numpy(), *[np.zeros_like(g.numpy()) for g in full[1:]])
    hs = hip_forward(sc, cam, D, kw, 1.0, bg_lib)
    hb = hip_backward_raw(hs, sc, cam, D, kw, [full[0], None, None, None], 1.0, bg_lib)
    hz = hip_backward_raw(hs, sc, cam, D, kw, [full[0]] + [torch.zeros_like(g) for g in full[1:]], 1.0, bg_lib)
    for k in GRAD_KEYS + ("acc",):
        assert torch.equal(hb[k], hz[k]), k
    err = np.abs(to_np(hb["acc"]).astype(np.float64) - ob["acc"])
    assert (err <= 4e-5 * ob["accabs"] + 1e-30).all()
    fin = oracle.finish_backward(os_, to_np(hb["acc"]))
    for k in GRAD_KEYS:
        assert_bits_equal(to_np(hb[k]).reshape(fin[k].shape), fin[k], k)


def _run_both_losses(oracle, sc, cam, D, kw, seed, background, device_background):
    """The full loss and the colour-only loss, with no background, or a non-zero one passed as host values or as a device tensor."""
    if background == "zero":
        _check(oracle, sc, cam, D, kw, seed=seed)
        _check_colour_only(oracle, sc, cam, D, kw, seed=seed)
        return
    if background == "device":
        device_background()
    _check(oracle, sc, cam, D, kw, bg=BG, seed=seed)
    _colour_only_with_background(oracle, sc, cam, D, kw, seed, BG, BG.cuda() if background == "device" else BG)


# ---- entry encoding: every batch index, unequal quarters ----

def _unequal_lists(cam, n, seed):
    """n splats in depth order: two of three cover the whole image (sigmas 60 and 35 px, opacity 0.015 .. 0.025: 0.975^257 = 1.5e-3,
    nobody's walk ends early), every third one -- never the last -- is a splat of sigmas 1.0 and 0.45 px at the centre of one of
    five 4x4 blocks of tile 0, which reaches alpha >= 1/255 in that block only (with the rasterizer's 0.3 px^2 dilation 0.03 exp(-2.5^2 / 2.6) = 2.7e-3)."""
    g = torch.Generator().manual_seed(seed)
    small = (torch.arange(n) % 3 == 1) & (torch.arange(n) < n - 1)
    if n == 2:
        small = torch.tensor([True, False])
    blk = torch.tensor(SMALL_BLOCKS)[torch.arange(n) % len(SMALL_BLOCKS)]
    px = torch.where(small, 4.0 * blk[:, 0] + 1.5, torch.rand(n, generator=g) * (cam.width - 3) + 1.0)
    py = torch.where(small, 4.0 * blk[:, 1] + 1.5, torch.rand(n, generator=g) * (cam.height - 3) + 1.0)
    angle = torch.rand(n, generator=g) * 0.35 + 0.25
    opacity = torch.where(small, torch.full((n,), 0.03), torch.rand(n, generator=g) * 0.01 + 0.015)
    sig_u = torch.where(small, torch.full((n,), 1.0), torch.full((n,), 60.0))
    sig_v = torch.where(small, torch.full((n,), 0.45), torch.full((n,), 35.0))
    return _splats(cam, n, px, py, sig_u, sig_v, angle, opacity, 3.0, 9.0, seed + 1), small.numpy()


def _assert_unequal_lists(os_, cam, n, small):
    length, bmax = _tile_stats(os_, cam)
    assert length[0] == n and bmax[0] == n and (bmax == length).all(), (n, length, bmax)   # tile 0 walks all n, every tile its whole list
    p = _powers(os_, cam)
    hit = (p <= 0) & (os_["conic_opacity"][:, 3].astype(np.float64)[:, None, None] * np.exp(p) >= 1.0 / 255.0)
    per_block = np.array([[hit[:, by:by + 4, bx:bx + 4].any(axis=(1, 2)) for bx in range(0, 16, 4)] for by in range(0, 16, 4)])
    blocks_hit = per_block.reshape(16, n).sum(axis=0)
    assert (blocks_hit[small] == 1).all() and (blocks_hit[~small] == 16).all(), blocks_hit      # one block only / the whole tile
    counts = per_block.reshape(16, n).sum(axis=1)
    if small.any():
        assert counts.min() == n - small.sum() and counts.max() > counts.min(), counts             # quarters of unequal length
    co, rgb = os_["conic_opacity"].astype(np.float64), os_["rgb"].astype(np.float64)
    assert (np.abs(co[:, 0] - co[:, 2]) > 0.2 * np.maximum(co[:, 0], co[:, 2])).all() and (np.abs(co[:, 1]) > 0).all()   # a != c, b != 0
    assert (rgb[:, 1] - rgb[:, 0] > 0.05).all() and (rgb[:, 2] - rgb[:, 1] > 0.05).all()
    assert len(np.unique(os_["depths"])) == n and not os_["clamped"].any()


@pytest.mark.parametrize("background", ["zero", "host", "device"])
@pytest.mark.parametrize("fast_exp", [True, False], ids=["fast_exp", "exact"])
@pytest.mark.parametrize("image", sorted(IMAGES))
def test_every_batch_index_reaches_its_record_in_unequal_quarter_lists(oracle, upstream, device_background, image, fast_exp, background):
    cam = scenes.make_camera(*IMAGES[image])
    upstream("part_zero" if background != "zero" else "dense")
    for n in LENGTHS:
        sc, small = _unequal_lists(cam, n, seed=n)
        kw = scene_kwargs(sc, True, False)
        _assert_unequal_lists(oracle_forward(oracle, sc, cam, 2, kw), cam, n, small)
        with gaustudio_amd.options(fast_exp=fast_exp):
            _run_both_losses(oracle, sc, cam, 2, kw, n % 5, background, device_background)


# ---- the contributor threshold ----

N_THRESHOLD = 300                      # rounds of tile 0: top = 300, 172, 44
TOP = N_THRESHOLD - BATCH              # the round the targets are placed around: list positions 44 .. 171
# last_contributor wanted at the centre pixel of a pair of opaque splats, the list position of the pair's second splat, and that pixel
# (4 px apart: a pair reaches alpha >= 1/255 within 3.3 px only, so the pairs of neighbouring targets may interleave).  Relative to
# the round with top = 172: before it (top - 1 - lc >= 127: every entry dead), all dead by one (lc = top - 128), only its last entry
# alive (lc = top - 127), inside, only its first entry dead (lc = top - 1), all alive (lc = top)
TARGETS = ((10, 10, (1, 1)), (TOP - BATCH, TOP - BATCH + 1, (5, 1)), (TOP - BATCH + 1, TOP - BATCH + 2, (9, 1)), (100, 100, (13, 1)),
           (TOP - 1, TOP, (1, 5)), (TOP, TOP + 1, (5, 5)))


def _threshold_scene(cam, seed):
    """300 splats in depth order.  The faint ones (opacity 0.012, sigmas 4 and 2.8 px, centres in [2, 8]^2: 0.988^300 = 0.027, no walk
    ends by them, and they leave the far corner of the tile untouched) and, for every target lc, two opaque ones (opacity 1, sigma 1 px)
    centred on one pixel, the first at list position lc - 1: alpha is capped at 0.99 there, the first one is taken (last_contributor
    = lc), the second one ends the walk (T 0.01^2 < 1e-4; nothing between the two reaches the pixel).  A pixel next to the centre
    sees alpha 0.6 twice and walks on."""
    n = N_THRESHOLD
    g = torch.Generator().manual_seed(seed)
    px = torch.rand(n, generator=g) * 6.0 + 2.0
    py = torch.rand(n, generator=g) * 6.0 + 2.0
    sig_u, sig_v = torch.full((n,), 4.0), torch.full((n,), 2.8)
    opacity = torch.full((n,), 0.012)
    angle = torch.rand(n, generator=g) * 0.35 + 0.25
    opaque = torch.zeros(n, dtype=torch.bool)
    for lc, second, (cx, cy) in TARGETS:
        for pos in (lc - 1, second):
            assert not opaque[pos]
            opaque[pos] = True
            px[pos], py[pos], sig_u[pos], sig_v[pos], opacity[pos], angle[pos] = float(cx), float(cy), 1.0, 1.0, 1.0, 0.0
    return _splats(cam, n, px, py, sig_u, sig_v, angle, opacity, 3.0, 9.0, seed + 1)


def _assert_threshold_cases(os_, cam):
    """The five positions of a lane's threshold relative to a round, and last_contributor differing inside one 4x4 block."""
    length, bmax = _tile_stats(os_, cam)
    assert length[0] == N_THRESHOLD and bmax[0] == N_THRESHOLD, (length, bmax)
    nc = os_["n_contrib"][:16, :16].astype(np.int64)
    for lc, _, (cx, cy) in TARGETS:
        assert nc[cy, cx] == lc, (lc, (cx, cy), nc[cy, cx])
        assert len(np.unique(nc[cy & ~3:(cy & ~3) + 4, cx & ~3:(cx & ~3) + 4])) >= 2      # differs from pixel to pixel inside the quarter
    top = TOP
    assert ((nc > 0) & (top - 1 - nc >= BATCH - 1)).any()             # before the round: every entry dead for that lane
    assert ((nc > top - BATCH + 1) & (nc < top - 1)).any()            # inside it
    assert (nc == top - 1).any() and (nc == top).any()                # at its first entry: dead / alive
    assert (nc == top - BATCH + 1).any() and (nc == top - BATCH).any()   # at its last entry: alive / dead
    assert (nc > top).any() and (nc == N_THRESHOLD).any()             # beyond it: negative threshold, every entry passes
    assert (nc == 0).any()                                            # a pixel no splat reaches (and, ragged, those outside the image)


@pytest.mark.parametrize("background", ["zero", "host", "device"])
@pytest.mark.parametrize("fast_exp", [True, False], ids=["fast_exp", "exact"])
@pytest.mark.parametrize("image", sorted(IMAGES))
def test_last_contributor_at_every_position_relative_to_a_round(oracle, upstream, device_background, image, fast_exp, background):
    cam = scenes.make_camera(*IMAGES[image])
    sc = _threshold_scene(cam, seed=7)
    kw = scene_kwargs(sc, True, False)
    _assert_threshold_cases(oracle_forward(oracle, sc, cam, 2, kw), cam)
    for kind in ("dense", "part_zero") if background != "zero" else ("dense",):
        upstream(kind)
        with gaustudio_amd.options(fast_exp=fast_exp):
            _run_both_losses(oracle, sc, cam, 2, kw, 3, background, device_background)


# ---- zero sums of either sign ----

def _zero_row_grads(zero):
    """Every upstream gradient identically `zero` (+0.0 or -0.0) on pixel row 1 of every 4x4 block (y % 4 == 1), and on the whole block
    at (4, 8); of both signs elsewhere."""
    def make(cam, seed=1):
        out = []
        for t in _scaled_output_grads(cam, seed):
            t = t - 0.5 * t.mean()
            assert (t > 0).any() and (t < 0).any()
            t[:, 1::4, :] = zero
            t[:, 8:12, 4:8] = zero
            out.append(t)
        return tuple(out)
    return make


@pytest.mark.parametrize("zero", [0.0, -0.0], ids=["plus0", "minus0"])
@pytest.mark.parametrize("fast_exp", [True, False], ids=["fast_exp", "exact"])
def test_a_row_of_zero_gradients_returns_the_zeros_of_the_oracle(oracle, upstream, fast_exp, zero):
    """A row of -0.0 gradients makes every q of that row -0: the row sums that start from the first pixel's value are -0 where
    sums that start from +0 are +0.  Nothing of that may show: the sums equal the oracle's within the bound, every gradient has the
    bits of the oracle's per-Gaussian stage, and a zero sum has the sign of the oracle's zero."""
    upstream(_zero_row_grads(zero))
    for image, n in (("1tile", 5), ("1tile", 129), ("ragged", 40)):
        cam = scenes.make_camera(*IMAGES[image])
        sc, small = _unequal_lists(cam, n, seed=n)
        kw = scene_kwargs(sc, True, False)
        os_ = oracle_forward(oracle, sc, cam, 2, kw)
        _assert_unequal_lists(os_, cam, n, small)
        grads = scenes.make_output_grads(cam, seed=2)
        assert all(np.signbit(g.numpy()[:, 1::4, :]).all() == np.signbit(zero) and not g.numpy()[:, 1::4, :].any() for g in grads)
        with gaustudio_amd.options(fast_exp=fast_exp):
            _check(oracle, sc, cam, 2, kw, seed=2)
            _check_colour_only(oracle, sc, cam, 2, kw, seed=2)
            hs = hip_forward(sc, cam, 2, kw)
            hb = hip_backward_raw(hs, sc, cam, 2, kw, grads)
        ob = oracle.backward(os_, *[g.numpy() for g in grads])
        acc, ref = to_np(hb["acc"]), ob["acc"].astype(np.float32)
        both_zero = (acc == 0) & (ref == 0)
        assert (np.signbit(acc[both_zero]) == np.signbit(ref[both_zero])).all()
        fin = oracle.finish_backward(os_, acc)
        for k in GRAD_KEYS:
            a, b = to_np(hb[k]).reshape(fin[k].shape), fin[k]
            assert (np.signbit(a) == np.signbit(b)).all(), k
