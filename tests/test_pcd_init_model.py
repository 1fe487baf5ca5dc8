"""CPU tests of the point-cloud seeds: the numpy model tests/pcd_init_model.py against what the reference's own functions
produced (tests/golden/pcd_init_ref.npz, written by tests/golden/make_pcd_init_fixture.py), the float16 logarithm of
depth_seeds against numpy's, and the Python boundary of gaustudio_amd.pcd_init, which raises before any device is needed."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mesh_init_model as mi  # noqa: E402
import pcd_init_model as pim  # noqa: E402
import gaustudio_amd  # noqa: E402
from gaustudio_amd import formats  # noqa: E402
from gaustudio_amd import pcd_init as pi  # noqa: E402

F32 = np.float32
CLOUDS = ("random", "lattice", "duplicates", "line", "clusters")


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(HERE, "golden", "pcd_init_ref.npz")))


def steps(a, b):
    """Number of float32 values between corresponding finite entries (0 = equal)."""
    ia, ib = (np.asarray(x, dtype=F32).view(np.int32).astype(np.int64) for x in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7fffffff), i) for i in (ia, ib))
    return np.abs(ia - ib)


@pytest.mark.parametrize("name", CLOUDS)
def test_model_dist2_against_reference(ref, name):
    """calculate_dist2_python squares a rounded square root in float64, which moves the float32 rounding by one step at most."""
    p, want = ref[f"cloud_{name}"], ref[f"dist2_{name}"]
    assert {"random": 500, "lattice": 125, "duplicates": 50, "line": 30, "clusters": 121}[name] == len(p)
    got = pim.mean_dist2(p)
    assert got.dtype == F32 and got.shape == want.shape and np.isfinite(want).all()
    s = steps(got, want)
    print(f"{name}: {int((s > 0).sum())} of {len(p)} values differ, at most {int(s.max())} step(s)")
    assert s.max() <= 1
    if name == "duplicates":
        assert (got[:40] == 0).all()
    if name == "lattice":
        assert (got == 1).all()


def test_model_seeds_against_create_from_attribute(ref):
    """Everything exact but the scale: torch's float32 log is accurate to 1 ulp, the contract's is correctly rounded."""
    xyz = ref["cloud_random"]
    m = pim.point_seeds(xyz, rgb=ref["seed_in_rgb"], rot=ref["seed_in_rot"], opacity=pim.PCD_OPACITY)
    for k in ("xyz", "f_dc", "f_rest", "opacity", "rot"):
        assert m[k].dtype == F32 and m[k].shape == ref["seed_" + k].shape, k
        assert np.array_equal(m[k], ref["seed_" + k]), k
    s = steps(m["scale"], ref["seed_scale"])
    print(f"scale: {int((s > 0).any(axis=1).sum())} of {len(xyz)} points differ, at most {int(s.max())} step(s)")
    assert m["scale"].shape == (500, 3) and s.max() <= 1
    assert (m["scale"][:, 0] == m["scale"][:, 1]).all() and (m["scale"][:, 0] == m["scale"][:, 2]).all()
    bare = pim.point_seeds(xyz)                           # rgb, rot and opacity defaulted
    for k in ("f_dc", "opacity", "rot"):
        assert np.array_equal(bare[k], ref["bare_" + k]), k
    assert steps(bare["scale"], ref["bare_scale"]).max() <= 1
    assert pim.DEFAULT_OPACITY == F32(pi.default_opacity()) and pim.PCD_OPACITY == F32(pi.PCD_OPACITY)
    assert (m["opacity"] == pim.PCD_OPACITY).all() and (bare["opacity"] == pim.DEFAULT_OPACITY).all()


def test_normal2rotation_is_pcd_pys(ref):
    """pcd.py:12-37 is mesh.py's function: exact on a Fibonacci sphere's inward normals (its (-0,-1,-0) pole included) and on
    the sign() cases; on random normals that are not unit, torch's vectorised kernels round a few entries differently, within
    the 4 ulp of scale that make_mesh_init_fixture.py asserts of the same model."""
    assert np.array_equal(mi.normal2rotation(ref["n2r_normals"]), ref["n2r_rot"], equal_nan=True)
    got, want = mi.normal2rotation(ref["seed_in_normals"]), ref["seed_in_rot"]
    assert np.abs(got.astype(np.float64) - want).max() <= 4 * np.spacing(F32(np.abs(want).max()))


@pytest.mark.parametrize("samples", [2, 9, 100])
def test_sky_against_fibonacci_sphere(ref, samples):
    p, n = pim.fibonacci_sphere(samples)
    assert np.array_equal(p.astype(F32), ref[f"fib_{samples}_points"].astype(F32))
    assert np.array_equal(n.astype(F32), ref[f"fib_{samples}_normals"].astype(F32))
    p2, n2 = pi.fibonacci_sphere(samples)
    assert np.array_equal(p2, p) and np.array_equal(n2, n)


def test_sky_points_shells():
    xyz, nrm = pi.sky_points(3, [50, 55])
    mx, mn = pim.sky_points(3, [50, 55])
    assert xyz.dtype == F32 and xyz.shape == (18, 3) and np.array_equal(xyz, mx) and np.array_equal(nrm, mn)
    p, n = pim.fibonacci_sphere(9)
    assert np.array_equal(xyz[9:], (p * 55.0).astype(F32)) and np.array_equal(nrm[:9], nrm[9:])
    one, _ = pi.sky_points(3, 100.0)
    assert np.array_equal(one, (p * 100.0).astype(F32))


def test_half_log_is_numpys():
    """All 31 745 non-negative float16 values up to +inf: half(float32(log(float64(h)))) is numpy's float16 log."""
    h = np.arange(0, 0x7c01, dtype=np.uint16).view(np.float16)
    assert len(h) == 31745 and np.isposinf(h[-1]) and h[0] == 0
    with np.errstate(all="ignore"):
        want = np.log(h)
    got = pim.half_log(h)
    assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert np.isneginf(got[0])


def test_depth_pack_model_is_the_reference_arithmetic():
    """depth.py:50-89 restated literally in numpy: the float16 cache, the uint8 colours, np.log of the float16 scales."""
    rng = np.random.default_rng(3)
    H, W = 7, 5
    pts = rng.uniform(-3, 3, (H, W, 3)).astype(F32)
    img = rng.uniform(0, 1, (H, W, 3)).astype(F32)
    img[0, 0], img[0, 1] = 0.0, 1.0
    depth = rng.uniform(0.5, 4, (H, W)).astype(F32)
    depth[2, 3] = 0.0
    fx, fy = 61.5, 60.25
    world_scale = depth / F32((F32(fx) + F32(fy)) / 2)
    pcd = np.hstack((pts.reshape(-1, 3), img.reshape(-1, 3), world_scale.reshape(-1, 1))).astype("float16")
    with np.errstate(all="ignore"):
        colors = (pcd[:, 3:6] * 255).astype("uint8")
        log_scales = np.log(pcd[:, 6:].astype("float16"))
    xyz, rgb, scale = pim.depth_pack(pts, img, depth, fx, fy)
    assert np.array_equal(xyz, pcd[:, :3].astype(F32))
    assert np.array_equal(rgb, colors.astype(F32) / F32(255.0)) and rgb[0, 0] == 0 and rgb[1, 0] == 1
    assert np.array_equal(scale, np.repeat(log_scales.astype(F32), 3, axis=1)) and np.isneginf(scale[2 * W + 3]).all()
    cloud = pim.depth_seeds([(xyz, rgb, scale)])
    assert (cloud["opacity"] == 0).all() and (cloud["rot"] == F32([1, 0, 0, 0])).all()


# ------------------------------------------------------------------------------------------------------------- boundary
def t(shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def test_exports():
    for name in ("mean_dist2", "point_seeds", "pcd_init_from_ply", "sky_seeds", "depth_seeds"):
        assert getattr(gaustudio_amd, name) is getattr(pi, name)
    assert callable(pi.pcd_init) and gaustudio_amd.pcd_init is pi


def test_boundary_raises_before_any_device():
    with pytest.raises(TypeError):
        pi.mean_dist2(np.zeros((5, 3), dtype=F32))
    with pytest.raises(ValueError):
        pi.mean_dist2(t((5, 2)))
    with pytest.raises(TypeError):
        pi.mean_dist2(t((5, 3), torch.float64))
    for n in (0, 1, 3):
        with pytest.raises(ValueError, match="at least 4"):
            pi.mean_dist2(t((n, 3)))
        with pytest.raises(ValueError, match="at least 4"):
            pi.point_seeds(t((n, 3)))
        with pytest.raises(ValueError, match="at least 4"):
            pi.pcd_init(t((n, 3)))
    with pytest.raises(ValueError):
        pi.mean_dist2(t((5, 3)), cell_target=0)
    with pytest.raises(ValueError, match="not both"):
        pi.point_seeds(t((5, 3)), rot=t((5, 4)), normals=t((5, 3)))
    for bad in (-1, 4, 1.5, True):
        with pytest.raises(ValueError):
            pi.point_seeds(t((5, 3)), sh_degree=bad)
    with pytest.raises(ValueError):
        pi.point_seeds(t((5, 3)), rgb=t((4, 3)))
    with pytest.raises(ValueError):
        pi.point_seeds(t((5, 3)), rot=t((5, 3)))
    with pytest.raises(ValueError):
        pi.point_seeds(t((5, 3)), opacity=t((5,)))
    with pytest.raises(TypeError):
        pi.point_seeds(t((5, 3)), scale=t((5, 3), torch.float16))
    with pytest.raises(TypeError):
        pi.point_seeds(t((5, 3)), opacity="0.1")
    with pytest.raises(ValueError):
        pi.point_seeds(t((5, 3)), dist2=t((4,)))
    with pytest.raises(ValueError, match="not both"):
        pi.point_seeds(t((5, 3)), scale=t((5, 3)), dist2=t((5,)))
    for res in (1, 0, -3):
        with pytest.raises(ValueError):
            pi.sky_seeds(resolution=res)
    with pytest.raises(TypeError):
        pi.sky_seeds(resolution=2.5)
    with pytest.raises(ValueError):
        pi.sky_seeds(resolution=3, sh_degree=7)
    with pytest.raises(ValueError):
        pi.depth_seeds([])
    with pytest.raises(ValueError):
        pi.depth_seeds([(t((4, 5)), t((4, 5)), np.eye(3), np.eye(4))])
    with pytest.raises(TypeError):
        pi.depth_seeds([(t((4, 5), torch.float64), t((4, 5, 3)), np.eye(3), np.eye(4))])


def test_cpu_tensors_raise_runtime_error():
    with pytest.raises(RuntimeError, match="ROCm"):
        pi.mean_dist2(t((5, 3)))
    with pytest.raises(RuntimeError, match="ROCm"):
        pi.point_seeds(t((5, 3)))
    with pytest.raises(RuntimeError, match="ROCm"):
        pi.point_seeds(t((0, 3)), scale=t((0, 3)))
    with pytest.raises(RuntimeError, match="ROCm"):
        pi.pcd_init(t((5, 3)), t((5, 3)), t((5, 3)))
    with pytest.raises(RuntimeError, match="ROCm"):
        pi.depth_seeds([(t((4, 5)), t((4, 5, 3)), np.eye(3), np.eye(4))])


def test_ply_point_cloud(tmp_path):
    """x, y, z; uchar colours / 255 in float64, then float32; normals when all three are there."""
    rng = np.random.default_rng(8)
    rec = np.zeros(6, dtype=[("x", "f4"), ("y", "f4"), ("z", "f4"), ("nx", "f4"), ("ny", "f4"), ("nz", "f4"),
                             ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for k in ("x", "y", "z", "nx", "ny", "nz"):
        rec[k] = rng.normal(size=6)
    for k in ("red", "green", "blue"):
        rec[k] = rng.integers(0, 256, 6)
    path = str(tmp_path / "cloud.ply")
    formats.write_ply_vertices(path, rec)
    p, c, n = pi.ply_point_cloud(path)
    assert p.dtype == F32 and np.array_equal(p, np.stack([rec["x"], rec["y"], rec["z"]], axis=1))
    assert np.array_equal(c, (np.stack([rec["red"], rec["green"], rec["blue"]], axis=1).astype(np.float64) / 255).astype(F32))
    assert np.array_equal(n, np.stack([rec["nx"], rec["ny"], rec["nz"]], axis=1))
    bare = str(tmp_path / "bare.ply")
    formats.write_ply_vertices(bare, rec[["x", "y", "z"]])
    p2, c2, n2 = pi.ply_point_cloud(bare)
    assert np.array_equal(p2, p) and c2 is None and n2 is None
    with pytest.raises(RuntimeError, match="ROCm"):
        pi.pcd_init_from_ply(path, device="cpu")
