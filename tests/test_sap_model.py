"""The CPU model of gaustudio_amd.sap (tests/sap_model.py) against what the reference's Python produced on the CPU
(tests/golden/py_sap.npz, written by tests/golden/make_sap_fixture.py), and the model's marching cubes on analytic fields.

Bounds.  The reference adds a node's k float32 terms one after the other in float32: any order of such a sum lies within
(k - 1) * 2^-24 * sum|terms| of the exact sum (first-order bound of recursive summation), which the model's float64 sum
stands for; weighted=True divides by k in float32 (one more rounding, 2^-24 |result|).  grid_interp is the same with k = 8.
phi is held to E_ref, the reference's own float32 error against the float64 model, which the fixture generator measured."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sap_model as sm  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "py_sap.npz")


@pytest.fixture(scope="module")
def fx():
    import gaustudio_amd.sap  # noqa: F401  (the module under test exists; its kernels are exercised in test_gpu_sap.py)
    return dict(np.load(GOLDEN))


def test_raster_within_the_summation_bound_of_the_reference(fx):
    s, k, a = sm.rasterize(fx["V"], fx["normals"], (32, 32, 32))
    bound = np.maximum(k - 1, 0)[None] * sm.U * a
    err = np.abs(fx["ras_u"].astype(np.float64) - s)
    print(f"unweighted: max err {err.max():.3e}, max bound {bound.max():.3e}, max k {k.max()}")
    assert (err <= bound).all()
    kk = np.maximum(k, 1)[None]
    errw = np.abs(fx["ras_w"].astype(np.float64) - s / kk)
    assert (errw <= bound / kk + sm.U * np.abs(fx["ras_w"])).all()
    assert (k > 0).sum() > 1000 and k.sum() == 8 * len(fx["V"])


def test_node_aligned_quirks(fx):
    for weighted, key, total in ((False, "quirk_u", 6.0), (True, "quirk_w", 0.75)):
        out, k = sm.rasterize32(fx["quirk_pts"], np.ones((2, 3), np.float32), (8, 8, 8), weighted)
        assert np.array_equal(out, fx[key]) and out.sum() == total
        assert k.sum() == 16 and (k > 0).sum() == 2          # both "corners" of every axis land on the point's own node


def test_interp_within_the_summation_bound_of_the_reference(fx):
    s, a = sm.interp(fx["phi_32"], fx["V"])
    err = np.abs(fx["fv_32"].astype(np.float64) - s)
    print(f"grid_interp: max err {err.max():.3e}, max bound {(7 * sm.U * a).max():.3e}")
    assert (err <= 7 * sm.U * a).all()


@pytest.mark.parametrize("key,res", [("32", (32, 32, 32)), ("nc", (20, 24, 36))])
def test_phi_within_eref(fx, key, res):
    phi = sm.dpsr64(fx["V"], fx["normals"], res, float(fx["sig"]))
    err = np.abs(fx["phi_" + key] - phi).max()
    print(f"phi {res}: max |reference - model| = {err:.3e}, E_ref = {float(fx['eref_' + key]):.3e}")
    assert err <= float(fx["eref_" + key]) and float(fx["eref_" + key]) < 2e-6
    assert fx["phi_32"][0, 0, 0] == 0.5 and 0.85 < (fx["phi_32"] > 0).mean() < 0.95


def test_spectral32_follows_the_float64_solve(fx):
    s, _, _ = sm.rasterize(fx["V"], fx["normals"], (20, 24, 36))
    spec = np.fft.rfftn(s, axes=(1, 2, 3))
    Phi, scale = sm.spectral32(spec.astype(np.complex64), (20, 24, 36), 2.0)
    phi = np.fft.irfftn(Phi.astype(np.complex128), s=(20, 24, 36), axes=(0, 1, 2))
    ref = sm.dpsr64(fx["V"], fx["normals"], (20, 24, 36), 2.0, scale=False, shift=False)
    assert np.abs(phi - ref).max() < 1e-5 * np.abs(ref).max()


NO_REJECT = (2, 3, 5, 6, 7, 10, 12, 24, 36, 255, 256)
ONE_REJECT = (100, 129)
OFF_NODE_INTEGER = (7, 10, 12, 24, 36, 100, 255)


@pytest.mark.parametrize("r", sorted(set(NO_REJECT + ONE_REJECT + OFF_NODE_INTEGER)))
def test_near_node_coords_hold_the_edges(r):
    """What tests/test_gpu_sap_edges.py relies on: the set holds the coordinate below 1 whose quotient rounds up to r (r = 100,
    129) and coordinates whose quotient is an integer although the point is off the node."""
    c = sm.near_node_coords(r)
    assert c.dtype == np.float32 and (np.diff(c) > 0).all() and c[0] == 0 and c[-1] < 1
    nodes = (np.arange(r, dtype=np.float64) / r).astype(np.float32)
    assert np.isin(nodes, c).all() and np.isin(np.nextafter(nodes[1:], np.float32(0)), c).all()
    assert np.float32(1 - 2.0 ** -24) in c
    cs = np.float32(1.0) / np.float32(r)
    q = c / cs
    assert q.dtype == np.float32
    rejected = np.floor(q) >= r
    off_node = (q == np.floor(q)) & (np.floor(q) * cs != c)
    print(f"r={r}: {len(c)} coordinates, {rejected.sum()} rejected, {off_node.sum()} with an integer quotient off the node")
    assert rejected.sum() == (1 if r in ONE_REJECT else 0)
    if r in OFF_NODE_INTEGER:
        assert off_node.sum() >= 1
    pts = np.zeros((len(c), 3), np.float32)
    pts[:, 1] = c
    assert np.array_equal(~sm.valid(pts, (2, r, 2)), rejected)
    # every accepted coordinate indexes inside the grid, and its two weights are those of a point in or on the cell
    (i0, i1), (w0, w1) = sm._axis(c[~rejected], r)
    assert i0.min() >= 0 and i0.max() < r and i1.min() >= 0 and i1.max() < r
    assert ((i1 == i0) | (i1 == (i0 + 1) % r)).all()
    assert (w0 >= 0).all() and (w1 >= 0).all() and np.abs(w0.astype(np.float64) + w1 - 1).max() < 1e-4


def test_normalize32_is_the_float32_chain():
    rng = np.random.default_rng(5)
    g = rng.normal(size=(5, 4, 3)).astype(np.float32)
    m = 0.1234567890123
    v = g.astype(np.float64) - float(np.float32(m))
    want = -v / abs(v[0, 0, 0]) * 0.5
    got = sm.normalize32(g, m)
    assert got.dtype == np.float32 and got[0, 0, 0] == (-0.5 if v[0, 0, 0] > 0 else 0.5)
    assert np.abs(got - want).max() <= 4 * sm.U * np.abs(want).max()
    assert np.array_equal(sm.normalize32(g, m, scale=False), g - np.float32(m))
    assert np.array_equal(sm.normalize32(g, None, scale=False), g) and np.array_equal(sm.normalize32(g, m, False, False), g)
    assert np.array_equal(sm.normalize32(g, None), (-g) / np.abs(g[0, 0, 0]) * np.float32(0.5))
    assert np.array_equal(sm.normalize32(g, m, shift=False), sm.normalize32(g, None))


@pytest.mark.parametrize("res,n,measured", [((9, 7, 5), 3000, 1.7e-7), ((129, 129, 129), 70000, 5.4e-7)])
def test_dpsr32_cpu_gives_eref(res, n, measured):
    """E_ref of a shape without a recorded fixture: the float32 CPU run against the float64 model.  `measured` is the figure
    of this chain with numpy 2.2.6 / scipy 1.15.3; another FFT build may move it, not its order."""
    P, N = sm.ellipsoid_cloud(n, seed=1)
    V = sm.unit_cube(P)[0]
    phi = sm.dpsr32_cpu(V, N, res, 2.0)            # asserts a complex64 spectrum and a float32 grid inside
    assert phi.dtype == np.float32 and phi.shape == res and phi[0, 0, 0] == 0.5
    eref = np.abs(phi - sm.dpsr64(V, N, res, 2.0)).max()
    print(f"dpsr32_cpu {res}: E_ref = {eref:.3e}")
    assert measured / 3 < eref < measured * 3
    assert eref < 2e-6                               # the ceiling test_phi_within_eref holds the recorded E_ref to


def fields(n):
    x = np.linspace(-1, 1, n)
    X, Y, Z = np.meshgrid(x, x * 0.9, x * 1.1, indexing="ij")
    return {
        "sphere": np.sqrt(X ** 2 + Y ** 2 + Z ** 2) - 0.63,
        "torus": np.sqrt((np.sqrt(X ** 2 + Y ** 2) - 0.55) ** 2 + Z ** 2) - 0.23,
        "two_spheres": np.minimum(np.sqrt((X - 0.4) ** 2 + Y ** 2 + Z ** 2) - 0.3, np.sqrt((X + 0.4) ** 2 + Y ** 2 + Z ** 2) - 0.33),
    }


@pytest.mark.parametrize("name,chi", [("sphere", 2), ("torus", 0), ("two_spheres", 4)])
def test_model_marching_cubes_is_closed_and_on_the_level(name, chi):
    g = fields(29)[name].astype(np.float32)
    level = 0.013
    v, f = sm.marching_cubes(g, level)
    assert len(f) > 200 and sm.is_closed(f) and sm.euler_characteristic(v, f) == chi
    assert np.array_equal(np.unique(f), np.arange(len(v)))
    # every vertex sits on a grid edge and the field, interpolated along that edge, is the level
    frac = v - np.floor(v)
    assert ((frac != 0).sum(1) <= 1).all()
    lo = np.floor(v).astype(int)
    hi = np.minimum(lo + (frac != 0), np.array(g.shape) - 1)
    a, b = g[lo[:, 0], lo[:, 1], lo[:, 2]].astype(np.float64), g[hi[:, 0], hi[:, 1], hi[:, 2]].astype(np.float64)
    val = a + (b - a) * frac.max(1)
    assert np.abs(val - level).max() < 1e-6
    # normals towards increasing value: away from the centre line of each shape is enough for the sphere
    if name == "sphere":
        n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        c = v[f].mean(1) - (np.array(g.shape) - 1) / 2
        assert ((n * c).sum(1) > 0).all()


def test_model_marching_cubes_normals_for_all_256_cases():
    def grad(fc, p):
        out = np.zeros(3)
        for i, (cx, cy, cz) in enumerate(sm.CORNERS):
            wx, wy, wz = (p[0] if cx else 1 - p[0]), (p[1] if cy else 1 - p[1]), (p[2] if cz else 1 - p[2])
            out += fc[i] * np.array([(1 if cx else -1) * wy * wz, wx * (1 if cy else -1) * wz, wx * wy * (1 if cz else -1)])
        return out

    for case in range(256):
        fc = np.array([-1.0 if (case >> i) & 1 else 1.0 for i in range(8)])
        g = np.empty((2, 2, 2), np.float32)
        for i, (cx, cy, cz) in enumerate(sm.CORNERS):
            g[cx, cy, cz] = fc[i]
        v, f = sm.marching_cubes(g, 0.0)
        assert len(f) == sm.NTRIS[case] and len(v) == sum(fc[a] * fc[b] < 0 for a, b in sm._tables.EDGES)
        for t in f:
            a, b, c = v[t].astype(np.float64)
            assert np.cross(b - a, c - a) @ grad(fc, (a + b + c) / 3) > 1e-9, (case, t)
