"""GPU edge tests of gaustudio_amd.postprocess (csrc/gsr_post.hip) against the float32 model tests/post_model.py, on the
inputs of tests/post_cases.py.

Points, normals and the fused epilogue are compared BIT FOR BIT (post_model.same_bits: NaN positions and the bytes of
everything else; the sign and payload of a NaN are the producer's).  The library is built without contraction and with
correctly rounded divide / sqrt, and the model restates every operation, so there is nothing to tolerate.

The masked bilateral filter: new_mask exactly, pixels outside the valid region byte for byte, filtered values under

    |hip - bilateral64| <= 4 E + range (2 delta + T 2^-23)

Derivation.  The kernel and post_model.bilateral32 perform the same float32 operations except the two __expf per tap, where
the model has np.exp.  bilateral64 is the same formula in float64.
  * E = max |bilateral32 - bilateral64| on that input, computed here: the float32 rounding of everything but the exps, as it
    accumulates in one particular evaluation; the kernel's differs in the weights, so it gets the same budget again with a
    factor for not being the same realisation (4 E in all).
  * a relative error delta on each weight moves the weighted mean sum(v w) / sum(w) of values v in [0, 1] by at most 2 delta
    (numerator and denominator each move by at most delta of sum(w)); the mean is scaled by `range` on the way out.
  * delta = 2^-22 + 2^-24 log2(e) max|arg|: __expf(x) is exp2(x log2(e)).  The hardware exp2 is good to 1 ulp, 2^-23
    relative, and a weight is the product of two of them: 2^-22.  The product x log2(e) is rounded, an absolute
    2^-24 log2(e) |x| on the exponent and (times ln 2 < 1) that much relative on the result.  max|arg| runs over the
    arguments of the taps whose weight is at least 2^-24 of the centre's weight 1: a smaller weight cannot move a float32
    mean of values in [0, 1], whatever its relative error.
  * T 2^-23: one rounding of the running sums per tap on either side.
The observed err / bound is printed per case; it is expected well under 1.  Measured on an MI355X (E, bound, err / bound):
    narrow-9x2-d5 4.5e-7 1.3e-5 0.036    narrow-3x3-d7 5.5e-7 1.8e-5 0.030    narrow-6x1-d3 3.7e-7 6.7e-6 0.056
    narrow-1x6-d3 4.7e-7 8.2e-6 0.057    narrow-2x2-d7 1.4e-7 1.7e-5 0.008    narrow-70x4-d9 9.9e-7 3.0e-5 0.040
    narrow-5x20-d11 1.4e-6 4.1e-5 0.034  d0-ss0.5 7.9e-7 1.3e-5 0.059         d0-ss1.0 7.1e-7 1.7e-5 0.048
    d0-ss2.1 9.6e-7 2.4e-5 0.047         d0-default-sigma (radius 112, 39381 taps) 3.1e-5 1.7e-2 0.0019
    extremes-pos-* 8.3e-7 1.1e-5..1.3e-5 0.061..0.077     extremes-neg-* 7.0e-7 1.0e-5..1.3e-5 0.050..0.063
    extremes-mixed-* 8.1e-7 1.1e-5..1.3e-5 0.058..0.072   nan-inside 7.5e-7 1.3e-5 0.060   all-valid 7.9e-7 1.2e-5 0.064
    sigma-color-0.05 8.8e-7 2.0e-5 0.042   sigma <= 0 (as 1) 7.9e-7 1.2e-5 0.072   one / two survivors, all-invalid: 0 0 0
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import post_cases as pc  # noqa: E402
import post_model as pm  # noqa: E402
from gaustudio_amd import postprocess as pp  # noqa: E402
from gaustudio_amd._abi import call  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def invalid(n):
    return (n == -1).all(-1)


def kw_of(K, E):
    return dict(extrinsics=torch.from_numpy(E), coordinate="world") if E is not None else dict(coordinate="camera")


# ------------------------------------------------------------------------------------------------ points, normals, epilogue
@pytest.mark.parametrize("H,W", pc.SIZES)
def test_points_and_normals_equal_the_model_bit_for_bit(H, W):
    for cam in pc.CAMERAS:
        K, E = pc.camera(cam, H, W)
        depth = pc.depth_map(H, W, cam)
        d, Kt, kw = gpu(depth), torch.from_numpy(K), kw_of(K, E)
        assert pm.same_bits(host(pp.depth_to_points(d, Kt, **kw)), pm.points(depth, K, E)), (cam, "points")
        zc = pm.points(depth, K)[..., 2]
        for lo, hi in pc.BOUNDS:
            for k in pc.KS + [pc.far_k(H, W)]:
                got = host(pp.depth_to_normals(d, Kt, k=k, d_min=lo, d_max=hi, **kw))
                want = pm.normals(depth, K, E, k, lo, hi)
                assert pm.same_bits(got, want), (cam, k, lo)
                if k == pc.far_k(H, W):
                    assert invalid(got).all()
            # k = 1: all five taps are the pixel itself, so its flag is the validity of its own camera z
            own = invalid(host(pp.depth_to_normals(d, Kt, k=1, d_min=lo, d_max=hi, **kw)))
            with np.errstate(invalid="ignore"):
                assert np.array_equal(own, ~((zc > F32(lo)) & (zc < F32(hi)))), (cam, lo)
                raw_ok = (depth > F32(lo)) & (depth < F32(hi))
            if cam == "skew" and lo == 0.5 and H * W >= 400:
                # raw depth and camera z on opposite sides of a bound, in both directions: the flag follows z
                with np.errstate(invalid="ignore"):
                    z_ok = (zc > F32(lo)) & (zc < F32(hi))
                for opposite in (raw_ok & (zc < F32(lo)), (depth > F32(hi)) & np.isfinite(depth) & z_ok):
                    assert opposite.sum() >= 10
                    assert np.array_equal(own[opposite], ~z_ok[opposite]) and np.array_equal(own[opposite], raw_ok[opposite])
            if cam != "skew" and W >= 8:
                # camera z == depth here; the row of depths on the bounds: d_min, above it, d_max, below it (twice: both BOUNDS)
                assert np.array_equal(zc[H // 2, :8], pc.bound_values())
                at = 0 if lo == pc.BOUNDS[0][0] else 4
                assert own[H // 2, at:at + 4].tolist() == [True, False, True, False]
        if cam == "shear" and H * W >= 400:
            n = host(pp.depth_to_normals(d, Kt, **kw))
            ln = np.linalg.norm(n[~invalid(n)].astype(np.float64), axis=-1)
            assert len(ln) > 50 and (np.abs(ln - 1) > 1e-3).all()          # A^-1 n of a non-rigid A, not renormalised


@pytest.mark.parametrize("H,W", pc.SIZES)
def test_fused_epilogue_equals_the_model_bit_for_bit(H, W):
    opac = pc.opacity_map(H, W, 0.5)
    o = gpu(opac)
    with np.errstate(invalid="ignore"):
        assert (opac == F32(0.5)).any() or H * W < 4
    for cam in pc.CAMERAS:
        K, E = pc.camera(cam, H, W)
        depth = pc.depth_map(H, W, cam)
        d, Kt, kw = gpu(depth), torch.from_numpy(K), kw_of(K, E)
        for lo, hi in pc.BOUNDS:
            for k in (1, 3, 5):
                want_p, want_n = pm.epilogue(depth, opac, 0.5, K, E, k, lo, hi)
                p, n = pp.depth_epilogue(d, Kt, opacity=o, min_opacity=0.5, k=k, d_min=lo, d_max=hi, **kw)
                assert pm.same_bits(host(p), want_p) and pm.same_bits(host(n), want_n), (cam, k, lo)
        # points only, normals only, no opacity
        want_p, want_n = pm.epilogue(depth, opac, 0.5, K, E, 3)
        p, n = pp.depth_epilogue(d, Kt, opacity=o, want_normals=False, **kw)
        assert n is None and pm.same_bits(host(p), want_p), cam
        p, n = pp.depth_epilogue(d, Kt, opacity=o, want_points=False, **kw)
        assert p is None and pm.same_bits(host(n), want_n), cam
        want_p, want_n = pm.epilogue(depth, None, 0.5, K, E, 5, 0.5, 2.5)
        p, n = pp.depth_epilogue(d, Kt, opacity=None, k=5, d_min=0.5, d_max=2.5, **kw)
        assert pm.same_bits(host(p), want_p) and pm.same_bits(host(n), want_n), cam
    with pytest.raises(RuntimeError):
        pp.depth_epilogue(d, Kt, k=7, **kw)


def test_singular_cameras_and_k0_raise_and_write_nothing():
    H, W = 9, 65
    K, E = pc.camera("rigid", H, W)
    Ks = K.copy(); Ks[1] = 2 * Ks[0]                 # proportional rows: the determinant is exactly 0
    Es = E.copy(); Es[2, :3] = 0                     # a zero row
    d = gpu(pc.depth_map(H, W, "rigid"))
    host9 = lambda a: (ctypes.c_float * a.size)(*[float(v) for v in a.reshape(-1)])
    f = ctypes.c_float
    for Kb, Eb in ((Ks, None), (Ks, E), (K, Es)):
        kb, eb = host9(Kb), (None if Eb is None else host9(Eb))
        out = torch.full((H, W, 3), 7.25, device="cuda")
        out2 = torch.full((H, W, 3), 7.25, device="cuda")
        with pytest.raises(RuntimeError):
            call("gsr_depth_to_points", d.device, d, W, H, kb, eb, out)
        with pytest.raises(RuntimeError):
            call("gsr_depth_to_normals", d.device, d, W, H, kb, 3, f(1e-3), f(1e5), eb, out)
        with pytest.raises(RuntimeError):
            call("gsr_depth_to_normals", d.device, d, W, H, kb, 7, f(1e-3), f(1e5), eb, out)
        with pytest.raises(RuntimeError):
            call("gsr_depth_epilogue", d.device, d, None, f(0.5), W, H, kb, 3, f(1e-3), f(1e5), eb, out, out2)
        torch.cuda.synchronize()
        assert bool((out == 7.25).all()) and bool((out2 == 7.25).all())
    Kt, Kst = torch.from_numpy(K), torch.from_numpy(Ks)
    with pytest.raises(RuntimeError):
        pp.depth_to_points(d, Kst)
    with pytest.raises(RuntimeError):
        pp.depth_to_normals(d, Kt, torch.from_numpy(Es), coordinate="world")
    with pytest.raises(RuntimeError):
        pp.depth_epilogue(d, Kt, torch.from_numpy(Es))
    for k in (0, -3):
        with pytest.raises(RuntimeError):
            pp.depth_to_normals(d, Kt, k=k)
        with pytest.raises(RuntimeError):
            pp.depth_epilogue(d, Kt, torch.from_numpy(E), k=k)
    # a singular extrinsic is not looked at in camera coordinates
    assert pm.same_bits(host(pp.depth_to_points(d, Kt, torch.from_numpy(Es), "camera")), pm.points(host(d), K))


def test_non_contiguous_depth_and_float64_cameras_give_the_same_bits():
    H, W = 17, 129
    K, E = pc.camera("shear", H, W)
    depth = pc.depth_map(H, W, "shear")
    d = gpu(depth)
    dT = gpu(np.ascontiguousarray(depth.T)).t()                   # [H, W] view with strides (1, H)
    assert not dT.is_contiguous() and torch.equal(dT.isnan(), d.isnan())
    Kt, Et = torch.from_numpy(K), torch.from_numpy(E)
    for Kx, Ex, dx in ((Kt.double(), Et.double(), d), (Kt, Et, dT), (Kt.t().contiguous().t(), Et.t().contiguous().t(), d)):
        assert pm.same_bits(host(pp.depth_to_points(dx, Kx, Ex, "world")), pm.points(depth, K, E))
        assert pm.same_bits(host(pp.depth_to_normals(dx, Kx, Ex, k=5, coordinate="world")), pm.normals(depth, K, E, 5))
        p, n = pp.depth_epilogue(dx, Kx, Ex, k=3)
        want_p, want_n = pm.epilogue(depth, None, 0.5, K, E, 3)
        assert pm.same_bits(host(p), want_p) and pm.same_bits(host(n), want_n)


# ---------------------------------------------------------------------------------------------------------- bilateral filter
def check_bilateral(cid, depth, mask, d, sc, ss, mask_t=None):
    """Runs the kernel and compares with the model; returns (filtered, new_mask) as numpy."""
    ref64, new_mask, E, bound, info = pm.bilateral_bound(depth, mask, d, sc, ss)
    got_t, got_mask_t = pp.masked_bilateral_filter(gpu(depth), gpu(mask) if mask_t is None else mask_t, d, sc, ss)
    got, got_mask = host(got_t), host(got_mask_t)
    assert got.dtype == F32 and np.array_equal(got_mask != 0, new_mask), cid
    region = new_mask & ~np.isnan(depth) if bound > 0 else np.zeros_like(new_mask)
    assert got[~region].tobytes() == depth[~region].tobytes(), cid          # invalid and NaN pixels: the input, byte for byte
    err = float(np.abs(got[region].astype(np.float64) - ref64[region]).max(initial=0.0))
    print(f"{cid}: radius {info['radius']} taps {info['taps']} range {info['range']:.4g} E {E:.3g} bound {bound:.3g} "
          f"err {err:.3g} err/bound {err / bound if bound else 0.0:.3g}")
    assert np.isfinite(got[region]).all() and err <= bound, cid
    return got, got_mask


@pytest.mark.parametrize("case", pc.bilateral_cases(), ids=lambda c: c[0])
def test_bilateral_against_the_model(case):
    cid, depth, mask, d, sc, ss = case
    got, got_mask = check_bilateral(*case)
    assert got_mask.dtype == np.bool_
    if cid in ("one-survivor", "two-equal-survivors", "all-invalid"):      # range 0 or nothing valid: the input comes back
        assert got.tobytes() == depth.tobytes()
        assert got_mask.sum() == dict([("one-survivor", 1), ("two-equal-survivors", 2), ("all-invalid", 0)])[cid]
    elif cid == "all-valid":
        assert got_mask.all()
    else:
        assert (got != depth)[got_mask].any()                               # the filter did run
    if cid == "nan-inside":
        (y, x), = np.argwhere(np.isnan(depth))
        clean = depth.copy(); clean[y, x] = 3.0
        _, clean_mask = pp.masked_bilateral_filter(gpu(clean), gpu(mask), d, sc, ss)
        assert got_mask[y, x] and np.array_equal(host(clean_mask), got_mask)      # new_mask does not look at the depth
        assert np.isnan(got[y, x]) and np.isnan(got).sum() == 1


def test_bilateral_arguments():
    _, depth, mask, d, sc, ss = next(c for c in pc.bilateral_cases() if c[0] == "sigma-color-0.05")
    dt, mt = gpu(depth), gpu(mask)
    base, base_mask = pp.masked_bilateral_filter(dt, mt, 5, 1.0, 1.0)
    for sc_, ss_ in ((0.0, 1.0), (1.0, 0.0), (-2.0, -0.5)):                 # a sigma <= 0 behaves as 1
        got, gm = pp.masked_bilateral_filter(dt, mt, 5, sc_, ss_)
        assert torch.equal(got, base) and torch.equal(gm, base_mask), (sc_, ss_)
        check_bilateral(f"sigma({sc_},{ss_})", depth, mask, 5, sc_, ss_)
    got, gm = pp.masked_bilateral_filter(dt, mt, 0, 1.0, -1.0)              # d = 0 with sigma_space <= 0: radius lrint(1.5) = 2
    want, wm = pp.masked_bilateral_filter(dt, mt, 5, 1.0, 1.0)
    assert torch.equal(got, want) and torch.equal(gm, wm)
    for bad in (2, 4, -1, -3):                                              # even and negative window sizes
        with pytest.raises(RuntimeError):
            pp.masked_bilateral_filter(dt, mt, bad, sc, ss)
        with pytest.raises(ValueError):
            pm.bilateral32(depth, mask, bad, sc, ss)
    # bool, uint8 and float32 masks: the same result, new_mask in the mask's dtype
    ref, ref_mask = pp.masked_bilateral_filter(dt, mt, d, sc, ss)
    for m2 in (mt.to(torch.uint8), mt.to(torch.uint8) * 255, mt.to(torch.float32) * 0.25):
        got, gm = pp.masked_bilateral_filter(dt, m2, d, sc, ss)
        assert gm.dtype == m2.dtype and torch.equal(got, ref) and torch.equal(gm != 0, ref_mask)
