"""-m gpu: composite_bwd's staged records, field by field.

The backward regroups the 16-B parts of a record in LDS -- (px, py, -a/2, -b), (-c/2, opacity, depth, r), (g, b, pcut, -) -- so
that a walk step reads 16 + 16 + 8 bytes.  The round tests (tests/test_gpu_backward_rounds.py) use isotropic splats, with which
swapped conic terms or a colour taken from the wrong word pass unnoticed.  Here every field of a record differs from every
other: anisotropic rotated Gaussians (a != c, b != 0), r, g, b pairwise different, distinct depths and opacities, and upstream
gradients with a different scale (and a non-zero mean) per output and per colour channel -- all checked on the CPU oracle
before the GPU runs.  Checks: those of tests/test_gpu_backward.py::_check and of the round tests' colour-only check (the
summation bound against the oracle, the bit-exact per-Gaussian stage, the banded backward equal to the one call)."""
import numpy as np
import pytest
import torch

import gaustudio_amd
from gaustudio_amd import scenes

from test_gpu_backward import _check
from test_gpu_backward_rounds import _check_colour_only, _tile_stats
from util import oracle_forward, scene_kwargs

pytestmark = pytest.mark.gpu

IMAGES = {"1tile": (16, 16), "ragged": (20, 27)}
LENGTHS = (1, 2, 127, 128, 129, 257)   # first slot, last slot before the sentinel, a round boundary, three rounds
SH_C0 = 0.28209479177387814
COLOUR_SCALE = (1.0, 0.37, 2.3)        # upstream gradient scales: colour channels, then depth, median depth, opacity
DEPTH_SCALE, MEDIAN_SCALE, OPACITY_SCALE = 0.21, 0.13, 0.45


def _scaled_output_grads(cam, seed=1):
    """scenes.make_output_grads with a different scale and mean per output and per colour channel: a gradient that reaches
    the wrong accumulator, or a colour multiplied with another channel's gradient, is off by a factor, not by noise."""
    g = torch.Generator().manual_seed(1000 + seed)
    H, W = cam.height, cam.width
    cs = torch.tensor(COLOUR_SCALE)[:, None, None]
    return ((torch.randn(3, H, W, generator=g) + 0.5) * cs, (torch.randn(1, H, W, generator=g) + 0.5) * DEPTH_SCALE,
            (torch.randn(3, H, W, generator=g) + 0.5) * MEDIAN_SCALE, (torch.randn(1, H, W, generator=g) + 0.5) * OPACITY_SCALE)


@pytest.fixture(autouse=True)
def _distinct_upstream_gradients(monkeypatch):
    """_check and _check_colour_only draw their upstream gradients from scenes.make_output_grads."""
    monkeypatch.setattr(scenes, "make_output_grads", _scaled_output_grads)


def _splats(cam, n, px, py, sig_u, sig_v, angle, opacity, z_lo, z_hi, seed):
    """n Gaussians at pixel centres (px, py), flat in z, with sigmas (sig_u, sig_v) pixels along axes turned by `angle` about
    the viewing direction; depths distinct and ascending with the index (the list order of every tile); r, g, b of a splat in
    three disjoint bands."""
    g = torch.Generator().manual_seed(seed)
    z = torch.linspace(z_lo, z_hi, n + 2)[1:-1].double() if n > 1 else torch.tensor([0.5 * (z_lo + z_hi)]).double()
    px, py = px.double(), py.double()
    x = ((2 * px + 1) / cam.width - 1) * cam.tanfovx * z       # inverse of the rasterizer's ndc -> pixel map
    y = ((2 * py + 1) / cam.height - 1) * cam.tanfovy * z
    to_world = z * 2 * cam.tanfovx / cam.width
    scales = torch.stack([sig_u.double() * to_world, sig_v.double() * to_world, 1e-3 * to_world], 1)
    rot = torch.zeros(n, 4)
    rot[:, 0] = torch.cos(angle / 2)
    rot[:, 3] = torch.sin(angle / 2)
    shs = torch.randn(n, 16, 3, generator=g) * 0.02
    rgb = torch.rand(n, 3, generator=g) * 0.2 + torch.tensor([0.1, 0.4, 0.7])
    shs[:, 0, :] = (rgb - 0.5) / SH_C0
    return scenes.Scene(torch.stack([x, y, z], 1).float().contiguous(), scales.float().contiguous(), rot.contiguous(),
                        opacity.reshape(n, 1).float().contiguous(), shs.float().contiguous())


def _distinct_fields(cam, n, seed=0):
    """Every splat covers the whole image at alpha >= 1/255, and the transmittance stays above 1e-4 behind 257 of them
    (0.975^257 = 1.5e-3): every tile walks its whole list.  Sigmas 60 and 35 px, turned by 0.25 .. 0.6 rad (at pi/4 a would equal c)."""
    g = torch.Generator().manual_seed(seed)
    px = torch.rand(n, generator=g) * (cam.width - 3) + 1.0
    py = torch.rand(n, generator=g) * (cam.height - 3) + 1.0
    angle = torch.rand(n, generator=g) * 0.35 + 0.25
    opacity = torch.rand(n, generator=g) * 0.01 + 0.015
    return _splats(cam, n, px, py, torch.full((n,), 60.0), torch.full((n,), 35.0), angle, opacity, 3.0, 9.0, seed + 1)


def _assert_distinct(os_, cam, n):
    length, bmax = _tile_stats(os_, cam)
    assert (length == n).all() and (bmax == n).all(), (n, length, bmax)      # the intended walk: the whole list, in every tile
    co, rgb, d = os_["conic_opacity"].astype(np.float64), os_["rgb"].astype(np.float64), os_["depths"].astype(np.float64)
    assert (np.abs(co[:, 0] - co[:, 2]) > 0.2 * np.maximum(co[:, 0], co[:, 2])).all()      # a != c
    assert (np.abs(co[:, 1]) > 0.05 * np.sqrt(co[:, 0] * co[:, 2])).all()                  # b != 0
    assert (rgb[:, 1] - rgb[:, 0] > 0.05).all() and (rgb[:, 2] - rgb[:, 1] > 0.05).all()   # r < g < b, apart
    assert not os_["clamped"].any()
    assert len(np.unique(d)) == n and len(np.unique(co[:, 3])) == n                        # distinct depths and opacities


def _powers(os_, cam):
    """power[i, y, x] of Gaussian i at every pixel, in double from the oracle's projected centres and conics."""
    m, co = os_["means2D"].astype(np.float64), os_["conic_opacity"].astype(np.float64)
    ys, xs = np.mgrid[0:cam.height, 0:cam.width].astype(np.float64)
    dx, dy = m[:, 0, None, None] - xs[None], m[:, 1, None, None] - ys[None]
    return -0.5 * (co[:, 0, None, None] * dx * dx + co[:, 2, None, None] * dy * dy) - co[:, 1, None, None] * dx * dy


@pytest.mark.parametrize("fast_exp", [True, False], ids=["fast_exp", "exact"])
@pytest.mark.parametrize("image", sorted(IMAGES))
def test_every_field_of_a_record_reaches_its_place(oracle, image, fast_exp):
    cam = scenes.make_camera(*IMAGES[image])
    for n in LENGTHS:
        sc = _distinct_fields(cam, n, seed=n)
        kw = scene_kwargs(sc, True, False)
        _assert_distinct(oracle_forward(oracle, sc, cam, 2, kw), cam, n)
        with gaustudio_amd.options(fast_exp=fast_exp):
            _check(oracle, sc, cam, 2, kw, seed=n % 5)


@pytest.mark.parametrize("fast_exp", [True, False], ids=["fast_exp", "exact"])
@pytest.mark.parametrize("image", sorted(IMAGES))
def test_every_field_with_a_colour_only_loss(oracle, image, fast_exp):
    """Depth, median-depth and opacity gradients absent: the CONLY instantiation, which reads the staged words in other shapes."""
    cam = scenes.make_camera(*IMAGES[image])
    for n in LENGTHS:
        sc = _distinct_fields(cam, n, seed=n)
        kw = scene_kwargs(sc, True, False)
        _assert_distinct(oracle_forward(oracle, sc, cam, 2, kw), cam, n)
        with gaustudio_amd.options(fast_exp=fast_exp):
            _check_colour_only(oracle, sc, cam, 2, kw, seed=n % 5)


def _unequal_quarters(cam, n, ox, oy, seed):
    """n splats of sigma 1 px and opacity 0.03 (alpha >= 1/255 within 2.3 px of the centre; 0.97^200 = 2e-3) with centres in
    [0.5, 2.0] x [0.5, 1.9] of the 8x8 region at (ox, oy): all of them reach its first 4x4 block, a fraction the second or
    the third, none the fourth."""
    g = torch.Generator().manual_seed(seed)
    px = ox + 0.5 + 1.5 * torch.rand(n, generator=g)
    py = oy + 0.5 + 1.4 * torch.rand(n, generator=g)
    one = torch.ones(n)
    return _splats(cam, n, px, py, one, one, torch.zeros(n), torch.full((n,), 0.03), 3.0, 9.0, seed + 1)


def _block_hits(os_, cam, ox, oy):
    """How many Gaussians have a pixel with power <= 0 and alpha >= 1/255 in each 4x4 block of the 8x8 region at (ox, oy)."""
    p = _powers(os_, cam)
    hit = (p <= 0) & (os_["conic_opacity"][:, 3].astype(np.float64)[:, None, None] * np.exp(p) >= 1.0 / 255.0)
    return [int(hit[:, oy + by:oy + by + 4, ox + bx:ox + bx + 4].any(axis=(1, 2)).sum()) for by in (0, 4) for bx in (0, 4)]


@pytest.mark.parametrize("fast_exp", [True, False], ids=["fast_exp", "exact"])
def test_short_quarters_walk_all_zero_sentinels(oracle, fast_exp):
    """The four quarters of a wave walk in step: the short lists are padded with the sentinel slot, whose record must be all
    zeros in every staged array a step reads (alpha = 0, w = 0, q = 0) -- anything else lands in the sums."""
    cam = scenes.make_camera(16, 16)
    for n, (ox, oy) in ((120, (0, 0)), (200, (8, 8))):
        sc = _unequal_quarters(cam, n, ox, oy, seed=n)
        kw = scene_kwargs(sc, True, False)
        hits = _block_hits(oracle_forward(oracle, sc, cam, 1, kw), cam, ox, oy)
        assert hits[0] == n and hits[3] == 0 and 0 < hits[1] < n // 2 and 0 < hits[2] < n // 2, hits
        with gaustudio_amd.options(fast_exp=fast_exp):
            _check(oracle, sc, cam, 1, kw, seed=3)
            _check_colour_only(oracle, sc, cam, 1, kw, seed=3)


def _footprint_edges(cam, n, seed):
    """Splats of sigma 1.5 .. 3 px and opacity 0.1 .. 0.6 spread over the image: the edge of the footprint (power = pcut, 2 to
    3.2 sigma from the centre) runs through the tile."""
    g = torch.Generator().manual_seed(seed)
    px = torch.rand(n, generator=g) * (cam.width - 1)
    py = torch.rand(n, generator=g) * (cam.height - 1)
    sig_u = 1.5 + 1.5 * torch.rand(n, generator=g)
    sig_v = sig_u * (0.5 + 0.3 * torch.rand(n, generator=g))
    angle = torch.rand(n, generator=g) * 0.35 + 0.25
    opacity = 0.1 + 0.5 * torch.rand(n, generator=g)
    return _splats(cam, n, px, py, sig_u, sig_v, angle, opacity, 3.0, 9.0, seed + 1)


@pytest.mark.parametrize("image", sorted(IMAGES))
def test_pcut_of_the_exact_mode(oracle, image):
    """The exact instantiations test power >= pcut, the one word of the record the fast_exp ones do not read.  (A pair below pcut
    also fails the alpha test, so a pcut that is too low goes unnoticed by construction; one that is too high -- a colour, a
    zero -- kills live pairs.)"""
    cam = scenes.make_camera(*IMAGES[image])
    n = 40
    sc = _footprint_edges(cam, n, seed=11)
    kw = scene_kwargs(sc, True, False)
    os_ = oracle_forward(oracle, sc, cam, 2, kw)
    p = _powers(os_, cam)
    pcut = np.maximum(-np.log(255.0 * os_["conic_opacity"][:, 3].astype(np.float64)) - 0.001, -80.0)[:, None, None]
    below, above = p < pcut - 1e-3, (p >= pcut + 1e-3) & (p <= 0)
    both = 0
    for by in range(0, cam.height, 4):
        for bx in range(0, cam.width, 4):
            both += int((below[:, by:by + 4, bx:bx + 4].any(axis=(1, 2)) & above[:, by:by + 4, bx:bx + 4].any(axis=(1, 2))).sum())
    assert both >= n, both      # (Gaussian, 4x4 block) pairs with pixels on both sides of pcut
    assert int(os_["n_contrib"].max()) >= n // 4
    with gaustudio_amd.options(fast_exp=False):
        _check(oracle, sc, cam, 2, kw, seed=2)
        _check_colour_only(oracle, sc, cam, 2, kw, seed=2)


@pytest.mark.parametrize("fast_exp", [True, False], ids=["fast_exp", "exact"])
def test_every_field_without_block_masks_from_the_forward(oracle, fast_exp):
    """cull off: the forward leaves no block masks and the backward runs gs_quarter_mask<2> on the staged arrays -- the conic,
    the centre and pcut, from three different places."""
    cam = scenes.make_camera(*IMAGES["ragged"])
    with gaustudio_amd.options(fast_exp=fast_exp, cull=False):
        n = 129
        sc = _distinct_fields(cam, n, seed=n)
        kw = scene_kwargs(sc, True, False)
        _assert_distinct(oracle_forward(oracle, sc, cam, 2, kw), cam, n)
        _check(oracle, sc, cam, 2, kw, seed=4)
        for sc, D in ((_footprint_edges(cam, 40, seed=11), 2), (_unequal_quarters(cam, 120, 8, 8, seed=120), 1)):   # masks that differ by block
            _check(oracle, sc, cam, D, scene_kwargs(sc, True, False), seed=4)
