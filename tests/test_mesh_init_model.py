"""CPU tests of the float32 model of gsr_mesh_seeds (tests/mesh_init_model.py) against what the
reference's own functions returned on the CPU (tests/golden/py_mesh_init.npz, written by tests/golden/make_mesh_init_fixture.py)
and against hand cases.  Each function is compared on the fixture's own inputs; the tolerance for torch's CPU arithmetic is
4 ulp of each output's scale (the spacing of float32 at the output's largest magnitude), the sign() cases agree exactly."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mesh_init_model as mi  # noqa: E402
from gaustudio_amd import mesh_init  # noqa: E402,F401  (the module these seeds model)

F32 = np.float32
NS = (1, 3, 4, 6)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "py_mesh_init.npz"))


def assert_ulps(got, want, limit=4.0, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == F32 and got.shape == want.shape, what
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin], equal_nan=True), what
    unit = np.spacing(F32(np.abs(want[fin]).max()))
    err = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64)).max() / unit
    print(f"{what}: {err:.2f} ulp of scale")
    assert err <= limit, f"{what}: {err} ulp of scale"


def test_fixture_is_the_model_mesh(fx):
    v, f, nr, col = mi.random_mesh()
    assert f.shape == (40, 3)
    for k, a in (("verts", v), ("faces", f), ("normals", nr), ("colors", col)):
        assert np.array_equal(fx[k], a)
    assert "asserted <= 4" in str(fx["meta"])


@pytest.mark.parametrize("n", NS)
def test_tables(fx, n):
    assert np.array_equal(mi.bary_table(n), fx[f"bary_{n}"])
    assert F32(mi.RADIUS[n]) == F32(fx[f"radius_{n}"])
    assert fx[f"pos_{n}"].shape == (40 * n, 3)


@pytest.mark.parametrize("n", NS)
def test_positions_normals_colours_scales(fx, n):
    v, f, nr, col = fx["verts"], fx["faces"], fx["normals"], fx["colors"]
    assert_ulps(mi.bary_sum(v, f, n), fx[f"pos_{n}"], what="_compute_gaussian_positions")
    assert_ulps(mi.surface_normals(nr, f, n), fx[f"nrm_{n}"], what="_compute_surface_normals")
    assert_ulps(mi.bary_sum(col, f, n), fx[f"col_{n}"], what="_compute_colors")
    assert_ulps(mi.scales(v, f, n), fx[f"scl_{n}"], what="_compute_scales")


@pytest.mark.parametrize("n", NS)
def test_normal2rotation(fx, n):
    assert_ulps(mi.normal2rotation(fx[f"nrm_{n}"]), fx[f"rot_{n}"], what="normal2rotation")


def test_rotmat2quaternion(fx):
    R = fx["rand_R"]
    assert np.isnan(fx["rand_q"]).any() and np.isfinite(fx["rand_q"]).any()      # 1 + trace < 0 for some: NaN, as torch.sqrt
    assert_ulps(mi.quaternion(R[:, :, 0], R[:, :, 1], R[:, :, 2]), fx["rand_q"], what="rotmat2quaternion")


def test_sign_cases_agree_exactly(fx):
    got = mi.normal2rotation(fx["quirk_normals"])
    assert np.array_equal(got, fx["quirk_rot"], equal_nan=True)


def test_sign_cases_by_hand():
    r = F32(np.sqrt(F32(1) + F32(1e-6)) / F32(2))            # R0 = 0 (and with it R1): trace = n_z + 1e-6
    q = mi.normal2rotation(F32([[1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 1, 0], [0, 0, -1]]))
    assert np.array_equal(q[0], F32([r, 0, F32(1) / (F32(4) * r), 0]))           # (R02 - R20) / 4r = n_x / 4r
    assert np.array_equal(q[1], F32([r, 0, F32(-1) / (F32(4) * r), 0]))
    r2 = F32(np.sqrt(F32(1) + (F32(3) + F32(1e-6))) / F32(2))                    # the identity
    assert np.array_equal(q[2], F32([r2, 0, 0, 0]))
    # n = (0, 1, 0): R0 = (1, 0, 0), sign(n_z) = 0 -> R1 = 0; trace = 1 + 1e-6; x = (R21 - R12) / 4r = -n_y / 4r
    r3 = F32(np.sqrt(F32(1) + (F32(1) + F32(1e-6))) / F32(2))
    assert np.array_equal(q[3], F32([r3, F32(-1) / (F32(4) * r3), 0, 0]))
    # n = (0, 0, -1): R0 = (1, 0, 0), R1 = n x R0 = (0, -1, 0) times sign(-1) sign(-1) = 1: trace = -1 + 1e-6
    r4 = F32(np.sqrt(F32(1) + ((F32(1) + F32(-1)) + F32(-1) + F32(1e-6))) / F32(2))
    assert q[4, 0] == r4 and 0 < r4 < 1e-3 and np.array_equal(q[4, 1:], F32([0, 0, 0]))


def test_seeds_equal_create_from_attribute(fx):
    v, f, nr, col = fx["verts"], fx["faces"], fx["normals"], fx["colors"]
    m = mi.seeds(v, f, nr, col, 1)
    for k in ("xyz", "f_dc", "scale", "rot"):
        assert m[k].shape == fx["seed_" + k].shape
        assert_ulps(m[k], fx["seed_" + k], what="create_from_attribute " + k)
    assert np.array_equal(m["f_rest"], fx["seed_f_rest"]) and m["f_rest"].shape == (40, 15, 3)
    assert np.array_equal(m["opacity"], fx["seed_opacity"]) and np.isposinf(m["opacity"]).all()
    # rgb=None: create_from_attribute takes ones -> f_dc = 0.5 / C0
    nc = mi.seeds(v, f, nr, None, 1)["f_dc"]
    assert_ulps(nc, fx["seed_nocolor_f_dc"], what="rgb=None f_dc")
    assert np.array_equal(nc, np.full((40, 1, 3), F32(0.5) / F32(mi.C0), dtype=F32))


@pytest.mark.parametrize("n", NS)
def test_hand_triangle(n):
    """A 3-4-5 triangle in the plane z = 1 with the normal (0, 0, 1): centroid-symmetric positions, scale from the edge 3."""
    v = F32([[0, 0, 1], [3, 0, 1], [0, 4, 1]])
    f = np.array([[0, 1, 2]], dtype=np.int32)
    nr = F32([[0, 0, 1]] * 3)
    col = F32([[1, 0, 0], [0, 1, 0], [0, 0, 1]])
    m = mi.seeds(v, f, nr, col, n)
    b = np.asarray(mi.BARY[n])
    assert np.allclose(m["xyz"], b @ v.astype(np.float64), atol=1e-6) and np.allclose(m["xyz"][:, 2], 1, atol=1e-6)
    assert np.allclose(m["f_dc"][:, 0], (b - 0.5) / mi.C0, atol=1e-6)
    s = np.log(2 * 3 * mi.RADIUS[n] + 1e-7)
    assert np.allclose(m["scale"][:, :2], s, atol=1e-6) and np.array_equal(m["scale"][:, 2], np.full(n, mi.log32(F32(1e-7))))
    assert np.allclose(m["rot"], [[1, 0, 0, 0]], atol=1e-6) and m["rot"].shape == (n, 4)


def test_zero_area_triangle_scale():
    v = F32([[0.5, 0.5, 0.5]] * 3)
    m = mi.seeds(v, np.array([[0, 1, 2]], dtype=np.int32), F32([[0, 0, 1]] * 3), None, 1)
    assert np.array_equal(m["scale"], np.full((1, 3), mi.log32(F32(1e-7)), dtype=F32))
    assert abs(float(m["scale"][0, 0]) - np.log(1e-7)) < 1e-5
