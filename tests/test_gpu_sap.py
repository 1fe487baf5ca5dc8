"""The HIP Shape-as-Points stage (gaustudio_amd.sap over csrc/gsr_psr.hip) against its CPU model (tests/sap_model.py) and the
outputs of the reference's Python recorded in tests/golden/py_sap.npz.

Bounds, and where they come from:
  * rasterize / grid_interp: device and model add the same float32 terms in float64, in different orders, and round once:
    at most 1 float32 ulp apart.  Counts, the node-aligned quirk cases and two runs of the same call: exactly equal.
  * spectral kernel, fed the model's spectrum: device and model run the same float32 chain; the only input that may differ
    is the filter G = float(exp(...)) (device and host exp in float64 may differ in the last bit, which can move the cast by
    one float32 ulp = 2 units of 2^-24).  Carried through the chain in units of 2^-24 relative to the magnitude sum_d |N_d| G
    |w_d| / |Lap + 1e-6| of a component: 2 (G) + 1/2 (N G) + 1/2 (times w) + 2 * 1/2 (the two additions) + 1/2 (the division)
    = 4.5, rounded up to SPECTRAL_UNITS = 5.
  * DPSR end to end against the float64 model: 4 x E_ref, E_ref the reference's own float32 error from the fixture (hipFFT
    and the CPU FFT are different float32 FFTs of the same error order).
  * marching cubes, fed the same grid as the model: vertices, faces and their order exactly equal.
Measured figures on an MI355X: DESIGN.md s14."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sap_model as sm  # noqa: E402
from test_sap_model import fields  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "py_sap.npz")
SPECTRAL_UNITS = 5
EREF_FACTOR = 4


def sap():
    from gaustudio_amd import sap as s
    return s


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def ulps_apart(a, b):
    """|a - b| in units of the float32 spacing at the larger magnitude."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def random_cloud(n, seed, channels=3):
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 3), dtype=np.float32)
    pts[: n // 8] = pts[: n // 8].round(1) % 1.0           # repeated coordinates, some of them on nodes
    return np.minimum(pts, np.float32(1 - 2 ** -24)), rng.normal(size=(n, channels)).astype(np.float32)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("res", [(32, 32, 32), (20, 24, 36)])
def test_rasterize_matches_the_model(fx, res, weighted):
    want, k = sm.rasterize32(fx["V"], fx["normals"], res, weighted)
    got, cnt = sap().point_rasterize(dev(fx["V"]), dev(fx["normals"]), res, weighted=weighted, return_counts=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3,) + res and got.grad_fn is None
    d = ulps_apart(got.cpu().numpy(), want)
    print(f"rasterize {res} weighted={weighted}: max {d.max():.2f} ulp, {(d > 0).sum()} of {d.size} values differ")
    assert d.max() <= 1
    assert np.array_equal(cnt.cpu().numpy(), k)


@pytest.mark.parametrize("n,res,channels", [(1, (2, 2, 2), 1), (5000, (7, 5, 3), 4), (200000, (64, 64, 64), 3), (300000, (16, 16, 16), 2)])
def test_rasterize_random_clouds_and_determinism(n, res, channels):
    pts, vals = random_cloud(n, n, channels)
    want, k = sm.rasterize32(pts, vals, res, True)
    a, ca = sap().point_rasterize(dev(pts), dev(vals), res, weighted=True, return_counts=True)
    b, cb = sap().point_rasterize(dev(pts), dev(vals), res, weighted=True, return_counts=True)
    assert torch.equal(a, b) and torch.equal(ca, cb), "two runs differ"
    assert np.array_equal(ca.cpu().numpy(), k)
    d = ulps_apart(a.cpu().numpy(), want)
    print(f"n={n} res={res}: max {d.max():.2f} ulp, max pairs per node {k.max()}")
    assert d.max() <= 1
    u = sap().point_rasterize(dev(pts), dev(vals), res, weighted=False)
    assert ulps_apart(u.cpu().numpy(), sm.rasterize32(pts, vals, res, False)[0]).max() <= 1


def test_node_aligned_quirks_are_exact(fx):
    ones = torch.ones((2, 3), device=DEV)
    for weighted, key, total in ((False, "quirk_u", 6.0), (True, "quirk_w", 0.75)):
        got, cnt = sap().point_rasterize(dev(fx["quirk_pts"]), ones, (8, 8, 8), weighted=weighted, return_counts=True)
        got = got.cpu().numpy()
        assert np.array_equal(got, fx[key]) and got.sum() == total
        assert int(cnt.sum()) == 16 and int((cnt > 0).sum()) == 2


@pytest.mark.parametrize("bad", [1.0, float("nan"), float("inf"), -1e-9])
def test_points_outside_the_unit_cube_raise(bad):
    pts = np.full((100, 3), 0.5, np.float32)
    pts[37, 1] = bad
    with pytest.raises(ValueError):
        sap().point_rasterize(dev(pts), torch.ones((100, 3), device=DEV), (8, 8, 8))
    with pytest.raises(ValueError):
        sap().grid_interp(torch.zeros((8, 8, 8), device=DEV), dev(pts))
    with pytest.raises(ValueError):
        sap().DPSR((8, 8, 8))(torch.rand((2, 10, 3), device=DEV), torch.rand((2, 10, 3), device=DEV))


@pytest.mark.parametrize("res", [(32, 32, 32), (20, 24, 36), (9, 6, 5)])
def test_spectral_kernel_matches_the_model(fx, res):
    s, _, _ = sm.rasterize(fx["V"], fx["normals"], res)
    spec = np.fft.rfftn(s, axes=(1, 2, 3)).astype(np.complex64)
    want, scale = sm.spectral32(spec, res, 2.0)
    got = sap().spectral_solve(dev(spec), res, 2.0).cpu().numpy()
    assert got.dtype == np.complex64 and got[0, 0, 0] == 0
    bound = SPECTRAL_UNITS * sm.U * scale
    err = np.maximum(np.abs(got.real.astype(np.float64) - want.real), np.abs(got.imag.astype(np.float64) - want.imag))
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"spectral {res}: {(got != want).sum()} of {got.size} elements differ, max err / (2^-24 scale) = "
              f"{np.nanmax(np.where(scale > 0, err / (sm.U * scale), 0)):.2f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("key,res", [("32", (32, 32, 32)), ("nc", (20, 24, 36))])
def test_dpsr_end_to_end(fx, key, res):
    want = sm.dpsr64(fx["V"], fx["normals"], res, 2.0)
    dpsr = sap().DPSR(res, sig=2)
    phi = dpsr(dev(fx["V"]), dev(fx["normals"]))
    assert tuple(phi.shape) == res and phi.dtype == torch.float32 and phi.grad_fn is None
    again = dpsr(dev(fx["V"])[None], dev(fx["normals"])[None])
    assert tuple(again.shape) == (1,) + res and torch.equal(again[0], phi), "two runs differ"
    err = np.abs(phi.cpu().numpy().astype(np.float64) - want).max()
    eref = float(fx["eref_" + key])
    ref_err = np.abs(phi.cpu().numpy() - fx["phi_" + key]).max()
    print(f"DPSR {res}: max |device - float64 model| = {err:.3e} = {err / eref:.2f} x E_ref ({eref:.3e}); "
          f"max |device - reference float32| = {ref_err:.3e}; phi[0,0,0] = {float(phi[0, 0, 0])}")
    assert err <= EREF_FACTOR * eref
    assert float(phi[0, 0, 0]) == 0.5


def test_dpsr_options(fx):
    V, N = dev(fx["V"]), dev(fx["normals"])
    res = (20, 24, 36)
    for kw in (dict(scale=False), dict(shift=False), dict(scale=False, shift=False), dict(weighted=True)):
        want = sm.dpsr64(fx["V"], fx["normals"], res, 2.0, **kw)
        got = sap().DPSR(res, sig=2, **kw)(V, N).cpu().numpy()
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"DPSR {kw}: relative error {err:.3e}")
        assert err < 1e-5
    t = sap().DPSR(res, sig=2)(V, N, apply_tanh=True).cpu().numpy()
    assert np.abs(t - np.tanh(sm.dpsr64(fx["V"], fx["normals"], res, 2.0))).max() < 1e-5


def test_grid_interp_matches_the_model(fx):
    for grid, pts in ((fx["phi_32"], fx["V"]), (fx["phi_nc"], random_cloud(20000, 3)[0])):
        s, _ = sm.interp(grid, pts)
        got, mean = sap().grid_interp(dev(grid), dev(pts), return_mean=True)
        d = ulps_apart(got.cpu().numpy(), s.astype(np.float32))
        print(f"grid_interp {grid.shape}: max {d.max():.2f} ulp")
        assert d.max() <= 1
        m = got.cpu().numpy().astype(np.float64).mean()
        assert abs(float(mean) - m) <= len(pts) * 2.0 ** -52 * np.abs(got.cpu().numpy()).astype(np.float64).mean()
        again, mean2 = sap().grid_interp(dev(grid), dev(pts), return_mean=True)
        assert torch.equal(again, got) and torch.equal(mean, mean2)


def assert_mc_equal(grid, level, what):
    v, f = sm.marching_cubes(grid, level)
    gv, gf = sap().marching_cubes(dev(grid), level)
    assert gv.dtype == torch.float32 and gf.dtype == torch.int32
    assert gv.shape == v.shape and gf.shape == f.shape, f"{what}: {tuple(gv.shape)} / {tuple(gf.shape)} vs {v.shape} / {f.shape}"
    assert np.array_equal(gv.cpu().numpy(), v), f"{what}: vertices differ"
    assert np.array_equal(gf.cpu().numpy(), f), f"{what}: faces differ"
    return v, f


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres"])
def test_marching_cubes_equals_the_model_on_analytic_fields(name):
    g = fields(29)[name].astype(np.float32)[:, :27, 1:]
    assert_mc_equal(g, 0.013, name)             # non-cubic crop: the torus leaves the grid, the mesh is open there
    assert_mc_equal(-g, -0.05, name + " negated")


@pytest.mark.parametrize("n", [2, 3, 64, 256])
def test_marching_cubes_sphere_sizes(n):
    x = np.linspace(-1, 1, n, dtype=np.float32)
    g = np.sqrt(x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2) - np.float32(0.71)
    v, f = assert_mc_equal(g.astype(np.float32), 0.0, f"sphere {n}")
    print(f"sphere {n}^3: {len(v)} vertices, {len(f)} faces")
    if n >= 64:
        assert sm.is_closed(f) and sm.euler_characteristic(v, f) == 2


def test_marching_cubes_boundary_crossing_and_empty():
    g = fields(17)["sphere"].astype(np.float32) - np.float32(0.6)     # the surface leaves the grid: open, still equal
    assert_mc_equal(g, 0.0, "open")
    v, f = sap().marching_cubes(torch.ones((5, 6, 7), device=DEV), 0.0)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)


def test_marching_cubes_of_the_reference_phi(fx):
    v, f = assert_mc_equal(np.tanh(fx["phi_32"]), 0.0, "tanh(phi_32)")
    assert sm.is_closed(f) and sm.euler_characteristic(v, f) == 2
    assert_mc_equal(np.tanh(fx["phi_nc"]), 0.0, "tanh(phi_nc)")


def test_mesh_sap_on_the_fixture_cloud(fx, tmp_path):
    from gaustudio_amd import formats, mesh_clean
    model_v, model_f = sm.marching_cubes(np.tanh(fx["phi_32"]), 0.0)
    assert sm.is_closed(model_f) and sm.euler_characteristic(model_v, model_f) == 2      # the condition of the comparison
    shape = sap().ShapeAsPoints.from_pointcloud(dev(fx["points"]), dev(fx["normals"]), dpsr_res=32)
    unit = torch.sigmoid(shape.xyz).cpu().numpy()
    print(f"max |device unit-cube coordinate - reference| = {np.abs(unit - fx['V']).max():.3e}")
    vertices, faces, v_unit = shape.generate_mesh()
    assert vertices.dtype == torch.float32 and faces.dtype == torch.int32 and vertices.grad_fn is None
    f = faces.cpu().numpy()
    assert sm.is_closed(f) and sm.euler_characteristic(vertices.cpu().numpy(), f) == 2
    idx = (v_unit * 32).cpu().numpy().astype(np.float64)
    d = np.sqrt(((idx[:, None, :] - model_v[None].astype(np.float64)) ** 2).sum(-1)).min(1)
    print(f"mesh_sap: {len(idx)} vertices / {len(f)} faces (model on the reference phi: {len(model_v)} / {len(model_f)}); "
          f"max distance to the nearest model vertex = {d.max():.3e} voxels")
    assert d.max() <= 1.0
    # world units: the inverse of the unit-cube map
    back = (v_unit.cpu().numpy() * 2 - 1) * fx["scale"] + fx["center"]
    assert np.abs(vertices.cpu().numpy() - back).max() < 1e-5
    v2, f2 = sap().mesh_sap(dev(fx["points"]), dev(fx["normals"]), dpsr_res=32)
    assert torch.equal(v2, vertices) and torch.equal(f2, faces)
    # downstream: cleaning keeps the single component, the PLY round trip keeps the counts
    cv, cf, removed = mesh_clean.remove_small_components(vertices, faces)
    assert removed == 0 and cv.shape == vertices.shape and cf.shape == faces.shape
    path = str(tmp_path / "fused_mesh.ply")
    formats.write_ply_mesh(path, cv, cf)
    rv, rf = formats.read_ply_mesh(path)
    assert rv.shape == tuple(vertices.shape) and rf.shape == tuple(faces.shape)
    assert np.array_equal(rv, vertices.cpu().numpy()) and np.array_equal(rf, f)


def test_argument_checks():
    s = sap()
    with pytest.raises(RuntimeError):
        s.point_rasterize(torch.rand(4, 3), torch.rand(4, 3), (8, 8, 8))             # CPU tensors: no fallback
    with pytest.raises(ValueError):
        s.point_rasterize(torch.rand(4, 3, device=DEV), torch.rand(4, 5, device=DEV), (8, 8, 8))
    with pytest.raises(ValueError):
        s.point_rasterize(torch.rand(4, 3, device=DEV), torch.rand(4, 3, device=DEV), (8, 1, 8))
    with pytest.raises(TypeError):
        s.marching_cubes(torch.zeros((4, 4, 4), dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError):
        s.ShapeAsPoints(dpsr_resolution=64)
