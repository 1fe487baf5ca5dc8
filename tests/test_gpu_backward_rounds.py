"""-m gpu: composite_bwd's staging rounds at their boundaries.

The backward stages 128 list entries per round (two halves of 64), requests a round's records one walk ahead and the
ids two walks ahead -- every lane loads, a lane beyond the walk's end from list position 0 -- and writes exact-zero rows
for the list entries behind the tile's last contributor.  The scenes here are the smallest that reach each of those
paths: one tile (16x16), 2x2 tiles (32x32) and a ragged 20x27 image in which EVERY Gaussian is in EVERY tile's list, so that
the list length is P and the walk's start is chosen by the opacities (all checked on the CPU oracle before the GPU runs).
Checks: those of tests/test_gpu_backward.py::_check -- the summation bound against the oracle (a row the kernel did not write
keeps the scratch's poison and fails it), the bit-exact per-Gaussian stage, the banded backward equal to the one call."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gaustudio_amd
from gaustudio_amd import scenes

from test_gpu_backward import GRAD_KEYS, _check
from util import assert_bits_equal, hip_backward_raw, hip_forward, oracle_forward, scene_kwargs, to_np

pytestmark = pytest.mark.gpu

IMAGES = {"1tile": (16, 16), "2x2": (32, 32), "ragged": (20, 27)}
UNSATURATED = (1, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257, 300)   # round, half-round and partial-round boundaries
DEAD_TAILS = (1, 127, 128, 129, 255, 256, 257, 600)                            # 256 threads: one, two and three trips of the zero-rows loop
FRONT = 8                                                                      # more opaque splats than any pixel walks


def _splats(cam, n, sigma_px, opacity, z_lo, z_hi, seed):
    """n isotropic Gaussians with centres inside the image, distinct depths ascending with the index (the list order of every tile)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.linspace(z_lo, z_hi, n + 2)[1:-1].double() if n > 1 else torch.tensor([0.5 * (z_lo + z_hi)]).double()
    px = torch.rand(n, generator=g).double() * (cam.width - 3) + 1.0
    py = torch.rand(n, generator=g).double() * (cam.height - 3) + 1.0
    x = ((2 * px + 1) / cam.width - 1) * cam.tanfovx * z       # inverse of the rasterizer's ndc -> pixel map
    y = ((2 * py + 1) / cam.height - 1) * cam.tanfovy * z
    sigma = sigma_px * z * 2 * cam.tanfovx / cam.width
    rot = torch.zeros(n, 4); rot[:, 0] = 1.0
    shs = torch.randn(n, 16, 3, generator=g) * 0.1
    shs[:, 0, :] = (torch.rand(n, 3, generator=g) * 2 - 1) / 0.28209479177387814
    return scenes.Scene(torch.stack([x, y, z], 1).float().contiguous(), sigma[:, None].expand(n, 3).float().contiguous(),
                        rot.contiguous(), torch.full((n, 1), float(opacity)), shs.float().contiguous())


def _cat(a, b):
    return scenes.Scene(*[torch.cat([u, v]).contiguous() for u, v in zip(a, b)])


def _unsaturated(cam, n, seed=0):
    """Every splat covers the whole image at alpha >= 1/255 and the transmittance stays above 1e-4 behind n <= 300 of them
    (0.98^300 = 2.3e-3): every tile walks its whole list."""
    return _splats(cam, n, sigma_px=40.0, opacity=0.02, z_lo=3.0, z_hi=9.0, seed=seed)


def _tile_stats(os_, cam):
    """Per tile: list length and the last contributor's maximum (the position the backward's walk starts at)."""
    gx, gy = (cam.width + 15) // 16, (cam.height + 15) // 16
    nc = os_["n_contrib"]
    r = os_["ranges"].astype(np.int64)
    bmax = np.array([[int(nc[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16].max()) for tx in range(gx)] for ty in range(gy)]).reshape(-1)
    return r[:, 1] - r[:, 0], bmax


def _saturated(oracle, cam, dead, seed=0):
    """Splats of opacity 0.8, each over the whole image, end every pixel's walk after a few entries (0.2^6 < 1e-4): nf are walked
    (probed on the oracle with FRONT of them), the next one ends the walk and is the first dead entry, and `dead` - 1 faint ones behind
    it make the dead tail.  Returns the scene, nf and the oracle's per-tile counts."""
    front = lambda k: _splats(cam, k, sigma_px=200.0, opacity=0.8, z_lo=2.0, z_hi=3.0, seed=seed + 100)
    probe = front(FRONT)
    _, b = _tile_stats(oracle_forward(oracle, probe, cam, 1, scene_kwargs(probe, True, False)), cam)
    nf = int(b.max())
    assert 0 < nf < FRONT
    sc = front(nf + 1)
    if dead > 1:
        sc = _cat(sc, _splats(cam, dead - 1, sigma_px=40.0, opacity=0.02, z_lo=4.0, z_hi=9.0, seed=seed))
    os_ = oracle_forward(oracle, sc, cam, 1, scene_kwargs(sc, True, False))
    return sc, nf, _tile_stats(os_, cam)


@pytest.mark.parametrize("fast_exp", [True, False], ids=["fast_exp", "exact"])
@pytest.mark.parametrize("image", sorted(IMAGES))
def test_unsaturated_lists_at_the_round_boundaries(oracle, image, fast_exp):
    cam = scenes.make_camera(*IMAGES[image])
    for n in UNSATURATED:
        sc = _unsaturated(cam, n, seed=n)
        kw = scene_kwargs(sc, True, False)
        length, bmax = _tile_stats(oracle_forward(oracle, sc, cam, 2, kw), cam)
        assert (length == n).all() and (bmax == n).all(), (image, n, length, bmax)   # the intended walk: the whole list, in every tile
        with gaustudio_amd.options(fast_exp=fast_exp):
            _check(oracle, sc, cam, 2, kw, seed=n % 5)


@pytest.mark.parametrize("fast_exp", [True, False], ids=["fast_exp", "exact"])
@pytest.mark.parametrize("image", ["1tile", "2x2"])
def test_saturated_tiles_write_zero_rows_for_the_dead_tail(oracle, image, fast_exp):
    cam = scenes.make_camera(*IMAGES[image])
    ran = 0
    for tail in DEAD_TAILS:
        sc, nf, (length, bmax) = _saturated(oracle, cam, tail, seed=tail)
        # only a case in which the oracle's own counts are the intended ones: every front splat is walked in every tile and nothing
        # behind them, so that the dead entries of every tile are exactly the `tail` faint ones
        if not ((length == nf + tail).all() and (bmax == nf).all()):
            continue
        ran += 1
        kw = scene_kwargs(sc, True, False)
        with gaustudio_amd.options(fast_exp=fast_exp):
            _check(oracle, sc, cam, 1, kw, seed=tail % 5)
            hs = hip_forward(sc, cam, 1, kw)
            hb = hip_backward_raw(hs, sc, cam, 1, kw, scenes.make_output_grads(cam, seed=2))
        acc = to_np(hb["acc"])
        assert np.isfinite(acc).all() and not acc[nf:].any(), (image, tail)       # written, and exactly zero
        assert acc[:nf].any()
    assert ran == len(DEAD_TAILS), f"only {ran} of {len(DEAD_TAILS)} scenes have the intended counts on the oracle"


def _check_colour_only(oracle, sc, cam, D, kw, seed):
    """The CONLY instantiation (three upstream gradients absent): bit-equal to explicit zero planes, and the two checks of _check
    against an oracle that was given the zeros."""
    full = scenes.make_output_grads(cam, seed=seed)
    os_ = oracle_forward(oracle, sc, cam, D, kw)
    ob = oracle.backward(os_, full[0].numpy(), *[np.zeros_like(g.numpy()) for g in full[1:]])
    hs = hip_forward(sc, cam, D, kw)
    hb = hip_backward_raw(hs, sc, cam, D, kw, [full[0], None, None, None])
    hz = hip_backward_raw(hs, sc, cam, D, kw, [full[0]] + [torch.zeros_like(g) for g in full[1:]])
    for k in GRAD_KEYS + ("acc",):
        assert torch.equal(hb[k], hz[k]), k
    err = np.abs(to_np(hb["acc"]).astype(np.float64) - ob["acc"])
    assert (err <= 4e-5 * ob["accabs"] + 1e-30).all()
    fin = oracle.finish_backward(os_, to_np(hb["acc"]))
    for k in GRAD_KEYS:
        assert_bits_equal(to_np(hb[k]).reshape(fin[k].shape), fin[k], k)


@pytest.mark.parametrize("fast_exp", [True, False], ids=["fast_exp", "exact"])
def test_colour_only_loss_at_the_round_boundaries(oracle, fast_exp):
    for image, lengths, tails in (("1tile", (1, 64, 65, 128, 129, 257, 300), (1, 257)), ("ragged", (63, 127, 193, 256), (600,))):
        cam = scenes.make_camera(*IMAGES[image])
        with gaustudio_amd.options(fast_exp=fast_exp):
            for n in lengths:
                sc = _unsaturated(cam, n, seed=n)
                _check_colour_only(oracle, sc, cam, 2, scene_kwargs(sc, True, False), seed=3)
            for tail in tails:
                sc, _, _ = _saturated(oracle, cam, tail, seed=tail)
                _check_colour_only(oracle, sc, cam, 1, scene_kwargs(sc, True, False), seed=3)


@pytest.mark.parametrize("fast_exp", [True, False], ids=["fast_exp", "exact"])
def test_forward_without_the_cull_leaves_no_block_masks(oracle, fast_exp):
    """cull off: the forward writes no per-entry block masks (has_qmask == 0), the backward computes gs_quarter_mask itself and must
    not read the masks' memory for anything it uses."""
    for image, lengths, tails in (("1tile", (1, 65, 128, 257), (129,)), ("2x2", (64, 129, 300), (1, 600))):
        cam = scenes.make_camera(*IMAGES[image])
        with gaustudio_amd.options(fast_exp=fast_exp, cull=False):
            for n in lengths:
                sc = _unsaturated(cam, n, seed=n)
                _check(oracle, sc, cam, 2, scene_kwargs(sc, True, False), seed=2)
            for tail in tails:
                sc, _, _ = _saturated(oracle, cam, tail, seed=tail)
                _check(oracle, sc, cam, 1, scene_kwargs(sc, True, False), seed=2)


@pytest.mark.parametrize("n", [1025, 1100, 1152])
def test_one_long_list_takes_the_row_flag_kernel_through_every_round(oracle, n):
    """More than 1024 entries in the image's only tile: the row-flag regime (no zero rows), nine rounds, the last one a single entry,
    a partial one or a full one.  (tests/test_gpu_backward.py's long-list scenes are random: their walks start anywhere.)"""
    cam = scenes.make_camera(16, 16)
    sc = _splats(cam, n, sigma_px=40.0, opacity=0.006, z_lo=3.0, z_hi=9.0, seed=n)     # 0.994^1152 = 1e-3: unsaturated
    kw = scene_kwargs(sc, True, False)
    length, bmax = _tile_stats(oracle_forward(oracle, sc, cam, 1, kw), cam)
    assert (length == n).all() and (bmax == n).all()
    _check(oracle, sc, cam, 1, kw, seed=4)


def test_every_lane_loads_inside_the_buffers_under_a_non_caching_allocator():
    """The staging loads are not masked: a lane beyond the walk's end reads the tile's list position 0 and the record it names.  Run
    (tests/guard_backward_rounds.py) where every opaque buffer is its own allocation, on a frame with empty tiles, on frames with
    one to three binned instances, without the forward's block masks and with a dead tail: same checks as above."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTORCH_NO_CUDA_MEMORY_CACHING="1")
    r = subprocess.run([sys.executable, os.path.join(here, "guard_backward_rounds.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count("ok ") == 6, (r.stdout[-1500:], r.stderr[-3000:])
