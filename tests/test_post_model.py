"""CPU tests of tests/post_model.py, the float32 model that DEFINES gaustudio_amd.postprocess (csrc/gsr_post.hip):
against outputs of the reference's own Camera class (tests/golden/py_post.npz), against the independent float64 restatement
oracle/post_oracle.py on the inputs of tests/test_gpu_post_edges.py (tests/post_cases.py), the border rule against its
closed form and np.pad, hand-checked cases, and the float32 form of the bilateral filter against its float64 form (the E of
the GPU test's tolerance, printed per case)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import post_cases as pc  # noqa: E402
import post_model as pm  # noqa: E402
from oracle import post_oracle as po  # noqa: E402

F32 = np.float32
GOLD = os.path.join(HERE, "golden", "py_post.npz")
TOL_P, TOL_N = 2e-5, 1e-4          # the fixture tolerances of tests/test_postprocess.py: points, normals


def invalid(n):
    return (n == -1).all(-1)


def test_model_matches_reference_camera_fixture():
    z = np.load(GOLD)
    K, E, d = z["intrinsics"], z["extrinsics"], z["depth"]
    assert np.abs(pm.points(d, K) - z["points_camera"]).max() < TOL_P
    assert np.abs(pm.points(d, K, E) - z["points_world"]).max() < TOL_P
    for key, kw in (("normals_camera", {}), ("normals_world", dict(E=E)), ("normals_camera_k5", dict(k=5))):
        n = pm.normals(d, K, **kw)
        assert np.array_equal(invalid(n), invalid(z[key])), key
        assert np.abs(n - z[key]).max() < TOL_N, key
    # the fused form is the two functions above on the masked depth
    op = np.random.default_rng(0).random(d.shape).astype(F32)
    p, n = pm.epilogue(d, op, 0.5, K, E)
    dm = np.where(op < 0.5, F32(0), d)
    assert pm.same_bits(p, pm.points(dm, K, E)) and pm.same_bits(n, pm.normals(dm, K, E))


def _close(a, b, tol, depth):
    """|a - b| <= tol where depths and values are O(1) as in the fixture; the 1e30 pixel, whose coordinates cancel, relative to
    its depth; the same non-finite values in the same places."""
    fin = np.isfinite(b)
    if not np.array_equal(np.isnan(a), np.isnan(b)) or not np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)]):
        return False
    with np.errstate(invalid="ignore"):
        scale = np.maximum(np.maximum(1.0, np.abs(b)), np.abs(depth.astype(np.float64))[..., None])
    return bool((np.abs(a[fin] - b[fin]) <= tol * scale[fin]).all())


@pytest.mark.parametrize("H,W", pc.SIZES)
def test_model_matches_float64_restatement_on_the_edge_inputs(H, W):
    """Same invalid sets -- given that no camera-space z lies within 1 ulp of a bound, which is asserted -- and values within
    the fixture tolerances.  (The inputs with depths exactly ON the bounds are the hand case below and the GPU test.)"""
    for cam in pc.CAMERAS:
        K, E = pc.camera(cam, H, W)
        depth = pc.depth_map(H, W, cam, boundary=False)
        zc = pm.points(depth, K)[..., 2]
        for lo, hi in pc.BOUNDS:
            for b in (F32(lo), F32(hi)):
                with np.errstate(invalid="ignore"):
                    assert not (np.abs(zc - b) <= 2 * np.spacing(b)).any(), "precondition: a camera z next to a bound"
        with np.errstate(all="ignore"):
            ref_p = po.depth2point(depth, K, E)
        assert _close(pm.points(depth, K, E), ref_p, TOL_P, depth), cam
        for k in pc.KS + [pc.far_k(H, W)]:
            for lo, hi in pc.BOUNDS:
                n = pm.normals(depth, K, E, k, lo, hi)
                with np.errstate(all="ignore"):
                    ref = po.depth2normal(depth, K, E, k, lo, hi)
                assert np.array_equal(invalid(n), invalid(ref)), (cam, k, lo)
                assert np.abs(n - ref)[~invalid(ref)].max(initial=0.0) < TOL_N, (cam, k, lo)
                if k == pc.far_k(H, W):
                    assert invalid(n).all()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_reflect_101_repeats_until_inside(n):
    """cv2's borderInterpolate rule against the closed form |p| mod 2(n - 1), folded, and against np.pad(mode="reflect")."""
    p = np.arange(-12, n + 12)
    got = pm.reflect101(p, n)
    if n == 1:
        want = np.zeros_like(p)
    else:
        m = 2 * (n - 1)
        q = np.abs(p) % m
        want = np.where(q < n, q, m - q)
    assert np.array_equal(got, want)
    assert got.min() >= 0 and got.max() <= n - 1
    assert np.array_equal(np.pad(np.arange(n), 12, mode="reflect"), got)


def test_normal_of_a_known_plane():
    """3x3 image of the plane n . p = c seen through a pinhole: the centre pixel gets n (oriented towards +z), the border
    pixels have a tap in the zero padding and are invalid."""
    K = np.array([[3.0, 0, 1.0], [0, 3.0, 1.0], [0, 0, 1]], F32)
    nrm = np.array([0.3, -0.2, 1.0]); nrm /= np.linalg.norm(nrm)
    x, y = np.meshgrid(np.arange(3.0), np.arange(3.0))
    rays = np.stack([x, y, np.ones_like(x)], -1) @ np.linalg.inv(K.astype(np.float64)).T
    depth = (2.0 / (rays @ nrm)).astype(F32)                     # rays have z = 1: the depth is the ray parameter
    n = pm.normals(depth, K)
    want_inv = np.ones((3, 3), bool); want_inv[1, 1] = False
    assert np.array_equal(invalid(n), want_inv)
    assert np.abs(n[1, 1] - nrm).max() < 1e-5
    assert np.abs(po.depth2normal(depth, K)[1, 1] - nrm).max() < 1e-5
    # a rigid extrinsic rotates it; a scaled one scales it (no renormalisation)
    _, E = pc.camera("rigid", 3, 3)
    assert np.abs(pm.normals(depth, K, E)[1, 1] - np.linalg.inv(E[:3, :3].astype(np.float64)) @ nrm).max() < 1e-5
    E2 = E.copy(); E2[:3, :3] *= 2
    assert abs(np.linalg.norm(pm.normals(depth, K, E2)[1, 1]) - 0.5) < 1e-5


def test_validity_exactly_on_the_bounds():
    """The bounds are float32 and exclusive: z == f32(d_min) and z == f32(d_max) are invalid, their float32 neighbours inside
    are valid.  f32(1e-3) > 1e-3 as a double: a comparison with the Python double would call it valid."""
    K = np.array([[4.0, 0, 2.0], [0, 4.0, 1.0], [0, 0, 1]], F32)       # last row (0, 0, 1): camera z == depth
    for lo, hi in pc.BOUNDS:
        depth = np.full((2, 4), F32(0.5 * (lo + min(hi, 10.0))), F32)
        depth[0] = [F32(lo), np.nextafter(F32(lo), F32(np.inf)), F32(hi), np.nextafter(F32(hi), F32(-np.inf))]
        assert np.array_equal(pm.points(depth, K)[..., 2], depth)
        want = np.zeros((2, 4), bool); want[0, 0] = want[0, 2] = True
        assert np.array_equal(invalid(pm.normals(depth, K, k=1, d_min=lo, d_max=hi)), want)
        assert np.array_equal(invalid(po.depth2normal(depth, K, k=1, d_min=lo, d_max=hi)), want)
    assert float(F32(1e-3)) > 1e-3


def test_singular_matrices_raise():
    K, E = pc.camera("rigid", 8, 8)
    Ks = K.copy(); Ks[1] = 2 * Ks[0]
    Es = E.copy(); Es[2, :3] = 0                     # a zero row: the determinant is exactly 0
    d = np.ones((8, 8), F32)
    with pytest.raises(ValueError):
        pm.points(d, Ks)
    with pytest.raises(ValueError):
        pm.normals(d, K, Es)
    with pytest.raises(ValueError):
        pm.normals(d, K, k=0)
    with pytest.raises(ValueError):
        pm.epilogue(d, None, 0.5, K, k=7)


def test_bilateral32_on_the_hand_checked_case():
    """The 5x5 case of tests/test_postprocess.py through the float32 model: with sigma = 75 on a [0, 1]-normalised image the
    weights are 1 to within 1e-4, so the filter is the mean over the centre and its 4-neighbours of the normalised image in
    which everything outside the eroded mask is 0."""
    d = np.arange(25, dtype=F32).reshape(5, 5) + 10.0
    m = np.ones((5, 5), np.uint8); m[0, 0] = 0
    out, nm = pm.bilateral32(d, m)
    want = np.ones((5, 5), bool); want[:2, :2] = False
    assert np.array_equal(nm, want) and out.dtype == F32
    assert np.array_equal(out[~nm], d[~nm])
    vmin, vmax = d[want].min(), d[want].max()
    norm = np.where(want, (d - vmin) / (vmax - vmin), 0.0)
    mean = (norm[2, 2] + norm[1, 2] + norm[3, 2] + norm[2, 1] + norm[2, 3]) / 5 * (vmax - vmin) + vmin
    assert abs(out[2, 2] - mean) < 2e-3
    mean = (norm[2, 1] + 0.0 + norm[3, 1] + norm[2, 0] + norm[2, 2]) / 5 * (vmax - vmin) + vmin
    assert abs(out[2, 1] - mean) < 2e-3
    mean = (norm[4, 4] + 2 * norm[3, 4] + 2 * norm[4, 3]) / 5 * (vmax - vmin) + vmin      # reflect-101 at the corner
    assert abs(out[4, 4] - mean) < 2e-3


def test_bilateral_nan_is_outside_the_valid_region():
    """extract_pcd.py:205-232: nanmin / nanmax, the NaN pixel is 0 in the filtered image and restored afterwards -- the same
    result as filtering with that pixel's depth replaced and its normalised value forced to 0; new_mask is unchanged."""
    _, d, m, dd, sc, ss = next(c for c in pc.bilateral_cases() if c[0] == "nan-inside")
    (y, x), = np.argwhere(np.isnan(d))
    out, nm = pm.bilateral32(d, m, dd, sc, ss)
    clean = d.copy(); clean[y, x] = 3.0
    _, nm_clean = pm.bilateral32(clean, m, dd, sc, ss)
    assert np.array_equal(nm, nm_clean) and nm[y, x]
    assert np.isnan(out[y, x]) and np.isnan(out).sum() == 1
    finite = nm & ~np.isnan(d)
    assert (out[finite] >= d[finite].min() - 1.0).all() and (np.abs(out - d)[finite] > 0).any()      # the filter did run
    o_out, o_nm = po.masked_bilateral_filter(d, m, dd, sc, ss)
    assert np.array_equal(o_nm, nm) and np.isnan(o_out[y, x]) and np.isnan(o_out).sum() == 1


@pytest.mark.parametrize("case", pc.bilateral_cases(), ids=lambda c: c[0])
def test_bilateral32_against_bilateral64_and_the_restatement(case):
    """Prints E = max |bilateral32 - bilateral64| and the bound the GPU test derives from it; the independent restatement
    (another float32 evaluation of the same formula, through np.pad) must lie within that bound of bilateral64 too."""
    cid, d, m, dd, sc, ss = case
    ref64, nm, E, bound, info = pm.bilateral_bound(d, m, dd, sc, ss)
    out32, nm32 = pm.bilateral32(d, m, dd, sc, ss)
    o_out, o_nm = po.masked_bilateral_filter(d, m, dd, sc, ss)
    with np.errstate(invalid="ignore"):
        err = float(np.nanmax(np.abs(o_out - ref64)))
    print(f"{cid}: radius {info['radius']} taps {info['taps']} range {info['range']:.4g} max|arg| {info['max_arg']:.3g} "
          f"E {E:.3g} bound {bound:.3g} restatement err/bound {err / bound if bound else 0.0:.3g}")
    assert np.array_equal(nm, nm32) and np.array_equal(nm, o_nm)
    assert np.array_equal(np.isnan(o_out), np.isnan(ref64)) and np.array_equal(np.isnan(out32), np.isnan(ref64))
    assert np.array_equal(out32[~nm], d[~nm])
    # E enters the GPU test's bound, so it must not hide a wrong bilateral32: a float32 sum of T terms in [0, 1] is off by at
    # most about T^2 2^-24 and in practice by a few T 2^-24 (64 T 2^-24 allowed, scaled by the range), plus the two
    # roundings of the de-normalisation at the size of the depths
    assert E <= 64 * info["taps"] * 2.0 ** -24 * max(info["range"], 1e-30) + 2.0 ** -22 * np.abs(d[np.isfinite(d)]).max()
    assert err <= bound
    if bound == 0.0:                                               # nothing filtered: the input comes back
        assert np.array_equal(out32, d) and np.array_equal(o_out, d)
