"""The Poisson half of gaustudio_amd.sap (csrc/gsr_psr.hip) at the sizes and coordinates the default resolution brings and
tests/test_gpu_sap.py does not reach: grids past the 2048-block launch cap of the two streaming kernels, odd sizes on every
axis, the scalar tail and the misaligned fallback of psr_normalize, more than 256 block partials in psr_mean, the fourth pass
of the rasterizer's radix sort, coordinates beside the grid nodes, and the occupancy extremes of the rasterizer.  The CPU model
(tests/sap_model.py) is the reference throughout.

Bounds, and where they come from (the first four as in test_gpu_sap.py):
  * rasterize / grid_interp: the same float32 terms added in float64 in another order, rounded once: 1 float32 ulp; counts exact;
  * spectral kernel fed the model's spectrum: SPECTRAL_UNITS * 2^-24 * scale;
  * the mean of the samples: a float64 sum of n terms in another order, n * 2^-52 * mean|s|;
  * DPSR end to end against the float64 model: EREF_FACTOR * E_ref, E_ref = max |dpsr32_cpu - dpsr64| computed here on the CPU;
  * normalize_grid without tanh: the float32 chain of sap_model.normalize32, bit for bit (the library is built with correctly
    rounded float32 division and without contraction);
  * tanh: the ROCm headers state no bound for tanhf.  TANH_ULPS is twice the maximum measured on an MI355X against float64 tanh
    of the exact float32 argument, rounded up.
Measured figures on an MI355X: DESIGN.md s14."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sap_model as sm  # noqa: E402
from test_gpu_sap import DEV, EREF_FACTOR, SPECTRAL_UNITS, dev, random_cloud, sap, ulps_apart  # noqa: E402

pytestmark = pytest.mark.gpu
TANH_ULPS = 3           # 2 x the measured maximum (1.38 ulp), rounded up: see the module docstring
LAUNCH_CAP = 2048 * 256   # lanes of a capped launch of psr_spectral / psr_normalize
BIG = (129, 129, 129)
SMALL = (9, 7, 5)


def poison(shape, dtype=torch.float32):
    """The functions under test write into torch.empty: hand the block such a call is likely to get back to the allocator
    full of NaN, so that an element the kernel leaves out does not hold the right value from an earlier call."""
    t = torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    torch.cuda.synchronize()
    del t


def tanh_ulps(got, pre):
    """|got - tanh(pre)| in float32 ulps of the exact result, tanh in float64 of the float32 argument."""
    want = np.tanh(np.asarray(pre, np.float32).astype(np.float64))
    return np.abs(np.asarray(got, np.float32).astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


class Cloud:
    """ellipsoid_cloud(n, seed=1) in the unit cube and what the model makes of it, each computed once."""

    def __init__(self, res, n):
        self.res = res
        P, self.N = sm.ellipsoid_cloud(n, seed=1)
        self.V = sm.unit_cube(P)[0]
        assert sm.valid(self.V, res).all()
        self._cache = {}

    def get(self, key, fn):
        if key not in self._cache:
            v = fn()
            for a in (v if isinstance(v, tuple) else (v,)):
                a.setflags(write=False)
            self._cache[key] = v
        return self._cache[key]

    @property
    def ras64(self):
        return self.get("ras", lambda: sm.rasterize(self.V, self.N, self.res)[0])

    @property
    def phi64(self):
        return self.get("phi64", lambda: sm.dpsr64(self.V, self.N, self.res, 2.0))

    @property
    def phi32(self):
        return self.get("phi32", lambda: sm.dpsr32_cpu(self.V, self.N, self.res, 2.0))


@pytest.fixture(scope="module")
def clouds():
    return {BIG: Cloud(BIG, 70000), SMALL: Cloud(SMALL, 3000)}


# ------------------------------------------------------------------------------------------------ 1. spectral past the cap
def test_spectral_kernel_past_the_launch_cap(clouds):
    c = clouds[BIG]
    spec = np.fft.rfftn(c.ras64, axes=(1, 2, 3)).astype(np.complex64)
    want, scale = sm.spectral32(spec, BIG, 2.0)
    assert want.size == 129 * 129 * 65 > 2 * LAUNCH_CAP
    for p in range(1, 3):                          # the condition: every later pass of the grid-stride loop has work to show
        assert np.abs(want.reshape(-1)[p * LAUNCH_CAP:(p + 1) * LAUNCH_CAP]).max() > 0
    poison((129, 129, 65, 2))
    got = sap().spectral_solve(dev(spec), BIG, 2.0).cpu().numpy()
    assert got.dtype == np.complex64 and got[0, 0, 0] == 0
    bound = SPECTRAL_UNITS * sm.U * scale
    err = np.maximum(np.abs(got.real.astype(np.float64) - want.real), np.abs(got.imag.astype(np.float64) - want.imag))
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"spectral {BIG}: {(got != want).sum()} of {got.size} elements differ, max err / (2^-24 scale) = "
              f"{np.nanmax(np.where(scale > 0, err / (sm.U * scale), 0)):.2f}")
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ 2. normalize_grid
def norm_grid(shape):
    """values of magnitudes 1e-3 .. 4 (after the scaling up to about 8: tanh from its linear range to saturation), g[0,0,0]
    of order one so that the scaling keeps them there."""
    rng = np.random.default_rng(shape[0] * 1000 + shape[2])
    g = (rng.normal(size=shape) * 10.0 ** rng.uniform(-3, 0.6, size=shape)).astype(np.float32)
    g[0, 0, 0] = 1.5
    mean = float(g.astype(np.float64).mean()) + 0.3 + 2.0 ** -30       # no float32
    return g, mean


def misaligned(flat, o, shape):
    """a contiguous view of `shape` whose address is 4 * o bytes past a 16-byte boundary"""
    buf = torch.zeros(flat.numel() + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[o:o + flat.numel()].copy_(flat)
    v = buf[o:o + flat.numel()].view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * o
    return v


@pytest.mark.parametrize("shape,tail", [(BIG, 1), (SMALL, 3), ((5, 5, 2), 2), ((2, 2, 2), 0)])
def test_normalize_grid_bit_for_bit(shape, tail):
    g, mean = norm_grid(shape)
    count = g.size
    assert count % 4 == tail and (count // 4 > LAUNCH_CAP) == (shape == BIG)
    gd = dev(g)
    assert gd.data_ptr() % 16 == 0
    md = torch.tensor([mean], dtype=torch.float64, device=DEV)
    worst = 0.0
    for with_mean in (True, False):
        for scale in (True, False):
            want = sm.normalize32(g, mean if with_mean else None, scale)
            kw = dict(mean=md if with_mean else None, scale=scale)
            poison(shape)
            got = sap().normalize_grid(gd, **kw)
            assert got.dtype == torch.float32 and tuple(got.shape) == shape and got.data_ptr() != gd.data_ptr()
            bad = got.cpu().numpy() != want
            assert not bad.any(), f"mean={with_mean} scale={scale}: {bad.sum()} of {count} differ, first at flat index {np.argmax(bad)}"
            poison(shape)
            t = sap().normalize_grid(gd, apply_tanh=True, **kw)
            u = tanh_ulps(t.cpu().numpy(), want)
            worst = max(worst, float(u.max()))
            assert u.max() <= TANH_ULPS, f"mean={with_mean} scale={scale}: tanh {u.max():.2f} ulp at flat index {np.argmax(u)}"
            for o in (1, 2, 3):
                view = misaligned(gd.reshape(-1), o, shape)
                poison(shape)
                m = sap().normalize_grid(view, **kw)
                assert torch.equal(m, got), f"offset {o}, mean={with_mean} scale={scale}: the misaligned result differs"
                poison(shape)
                assert torch.equal(sap().normalize_grid(view, apply_tanh=True, **kw), t), f"offset {o}: tanh differs"
                assert torch.equal(view, gd), "normalize_grid changed its input"
            assert torch.equal(gd.cpu(), torch.from_numpy(g)), "normalize_grid changed its input"
    print(f"normalize_grid {shape} (tail {tail}): bit-equal to normalize32; tanh max {worst:.3f} ulp")


# ------------------------------------------------------------------------------------------------ 3. mean over > 256 partials
@pytest.mark.parametrize("n", [65536, 65537, 70000])
def test_grid_interp_mean_over_more_than_256_partials(n):
    res = (20, 24, 36)
    grid = (1 + np.random.default_rng(7).random(res)).astype(np.float32)
    pts = random_cloud(n, 11)[0]
    s, _ = sm.interp(grid, pts)
    got, mean = sap().grid_interp(dev(grid), dev(pts), return_mean=True)
    got = got.cpu().numpy()
    assert (got >= 1).all()                        # positive samples: a dropped partial moves the mean by 1/n relative at least
    d = ulps_apart(got, s.astype(np.float32))
    m = got.astype(np.float64).mean()
    bound = n * 2.0 ** -52 * np.abs(got).astype(np.float64).mean()
    print(f"grid_interp n={n} ({(n + 255) // 256} partials): max {d.max():.2f} ulp, |mean - float64 mean| = "
          f"{abs(float(mean) - m):.3e}, bound {bound:.3e}")
    assert d.max() <= 1
    assert abs(float(mean) - m) <= bound


# ------------------------------------------------------------------------------------------------ 4. DPSR end to end
@pytest.mark.parametrize("res", [BIG, SMALL])
def test_dpsr_end_to_end_odd_grids(clouds, res):
    c = clouds[res]
    eref = np.abs(c.phi32 - c.phi64).max()
    V, N = dev(c.V), dev(c.N)
    dpsr = sap().DPSR(res, sig=2)
    poison(res)
    phi = dpsr(V, N)
    assert tuple(phi.shape) == res and phi.dtype == torch.float32 and phi.grad_fn is None
    got = phi.cpu().numpy()
    err = np.abs(got.astype(np.float64) - c.phi64).max()
    print(f"DPSR {res}: E_ref = {eref:.3e}; max |device - float64 model| = {err:.3e} = {err / eref:.2f} x E_ref; "
          f"max |device - float32 CPU run| = {np.abs(got - c.phi32).max():.3e}; phi[0,0,0] = {float(phi[0, 0, 0])}")
    assert err <= EREF_FACTOR * eref
    assert float(phi[0, 0, 0]) == 0.5
    poison(res)
    assert torch.equal(dpsr(V, N), phi), "two runs differ"
    batched = dpsr(V[None], N[None])
    assert tuple(batched.shape) == (1,) + res and torch.equal(batched[0], phi), "the batched form differs"
    poison(res)
    t = dpsr(V, N, apply_tanh=True)
    u = tanh_ulps(t.cpu().numpy(), got)
    print(f"DPSR {res} apply_tanh: max {u.max():.3f} ulp from tanh of the plain result")
    assert u.max() <= TANH_ULPS
    if res != BIG:
        return
    model_v, model_f = sm.marching_cubes(np.tanh(c.phi64).astype(np.float32), 0.0)
    assert sm.is_closed(model_f) and sm.euler_characteristic(model_v, model_f) == 2      # the condition of the comparison
    gv, gf = sap().marching_cubes(t, 0.0)
    gv, gf = gv.cpu().numpy(), gf.cpu().numpy()
    assert sm.is_closed(gf) and sm.euler_characteristic(gv, gf) == 2
    from scipy.spatial import cKDTree
    d = cKDTree(model_v.astype(np.float64)).query(gv.astype(np.float64))[0]
    print(f"marching cubes {res}: {len(gv)} vertices / {len(gf)} faces (model: {len(model_v)} / {len(model_f)}); "
          f"max distance to the nearest model vertex = {d.max():.3e} voxels")
    assert d.max() <= 1.0


# ------------------------------------------------------------------------------------------------ 5. beside the nodes
def near_node_cloud(res, seed, at_least=2000):
    """Every valid near_node_coords value of every axis at least once; the other two coordinates from their own near-node
    sets for half of the points, uniform for the rest."""
    rng = np.random.default_rng(seed)
    sets = []
    for d in range(3):
        c = sm.near_node_coords(res[d])
        probe = np.zeros((len(c), 3), np.float32)
        probe[:, d] = c
        sets.append(c[sm.valid(probe, res)])
    reps = -(-at_least // sum(len(s) for s in sets))
    rows = []
    for d in range(3):
        for _ in range(reps):
            p = rng.random((len(sets[d]), 3), dtype=np.float32)
            near = rng.random(len(p)) < 0.5
            for e in range(3):
                if e != d:
                    p[near, e] = rng.choice(sets[e], size=int(near.sum()))
            p[:, d] = sets[d]
            rows.append(p)
    pts = np.minimum(np.concatenate(rows), np.float32(1 - 2.0 ** -24))
    pts = pts[rng.permutation(len(pts))]
    for d in range(3):
        assert np.isin(sets[d], pts[:, d]).all()
    assert sm.valid(pts, res).all()
    return pts, rng.normal(size=(len(pts), 4)).astype(np.float32), sets


@pytest.mark.parametrize("res", [(3, 5, 7), (10, 12, 6), (100, 129, 36)])
def test_coordinates_beside_the_nodes(res):
    pts, vals, sets = near_node_cloud(res, sum(res))
    # the condition: the cloud holds coordinates whose quotient is an integer off the node, on some axis
    off_node = 0
    for d in range(3):
        cs = np.float32(1.0) / np.float32(res[d])
        q = sets[d] / cs
        off_node += int(((q == np.floor(q)) & (np.floor(q) * cs != sets[d])).sum())
    assert off_node >= 1
    for weighted in (False, True):
        want, k = sm.rasterize32(pts, vals, res, weighted)
        got, cnt = sap().point_rasterize(dev(pts), dev(vals), res, weighted=weighted, return_counts=True)
        assert np.array_equal(cnt.cpu().numpy(), k), f"weighted={weighted}: counts differ at {(cnt.cpu().numpy() != k).sum()} nodes"
        d = ulps_apart(got.cpu().numpy(), want)
        print(f"near-node cloud {res}, {len(pts)} points ({off_node} integer quotients off the node), weighted={weighted}: "
              f"max {d.max():.2f} ulp, {(d > 0).sum()} of {d.size} values differ, max pairs per node {k.max()}")
        assert d.max() <= 1
    grid = np.random.default_rng(3).normal(size=res).astype(np.float32)
    s, _ = sm.interp(grid, pts)
    fv = sap().grid_interp(dev(grid), dev(pts)).cpu().numpy()
    d = ulps_apart(fv, s.astype(np.float32))
    print(f"near-node cloud {res}: grid_interp max {d.max():.2f} ulp")
    assert d.max() <= 1


@pytest.mark.parametrize("axis,r", [(0, 100), (1, 129)])
def test_the_coordinate_whose_quotient_rounds_up_to_the_size_is_refused(axis, r):
    res = (100, 129, 36)
    c = sm.near_node_coords(r)
    q = np.floor(c / (np.float32(1.0) / np.float32(r)))
    rejected, accepted = c[q >= r], c[q < r].max()
    assert len(rejected) == 1 and accepted < rejected[0] < 1
    pts, vals, _ = near_node_cloud(res, 5, at_least=200)
    grid = torch.zeros(res, device=DEV)
    pts[123, axis] = rejected[0]
    assert not sm.valid(pts, res)[123] and sm.valid(pts, res).sum() == len(pts) - 1
    with pytest.raises(ValueError):
        sap().point_rasterize(dev(pts), dev(vals), res)
    with pytest.raises(ValueError):
        sap().grid_interp(grid, dev(pts))
    pts[123, axis] = accepted
    assert sm.valid(pts, res).all()
    want, k = sm.rasterize32(pts, vals, res, True)
    got, cnt = sap().point_rasterize(dev(pts), dev(vals), res, return_counts=True)
    assert np.array_equal(cnt.cpu().numpy(), k) and ulps_apart(got.cpu().numpy(), want).max() <= 1
    fv = sap().grid_interp(grid + 1, dev(pts)).cpu().numpy()
    assert ulps_apart(fv, sm.interp(np.ones(res, np.float32), pts)[0].astype(np.float32)).max() <= 1


# ------------------------------------------------------------------------------------------------ 6. occupancy extremes
def check_raster(pts, vals, res, what):
    """counts exact, values within 1 ulp (weighted and unweighted), two runs bit-equal"""
    for weighted in (True, False):
        want, k = sm.rasterize32(pts, vals, res, weighted)
        a, ca = sap().point_rasterize(dev(pts), dev(vals), res, weighted=weighted, return_counts=True)
        b, cb = sap().point_rasterize(dev(pts), dev(vals), res, weighted=weighted, return_counts=True)
        assert torch.equal(a, b) and torch.equal(ca, cb), f"{what}: two runs differ"
        assert np.array_equal(ca.cpu().numpy(), k), f"{what}: counts differ"
        got = a.cpu().numpy()
        hit = (got != 0) | (want != 0)              # elsewhere both are zero: 0 ulp
        d = ulps_apart(got[hit], want[hit])
        print(f"{what} weighted={weighted}: max {d.max():.2f} ulp, {(d == 1).sum()} values 1 ulp off, {(d > 1).sum()} further, "
              f"of {hit.sum()} non-zero; max pairs per node {k.max()}")
        assert d.max() <= 1
    return k


@pytest.mark.parametrize("weighted", [False, True])
def test_rasterize_no_points(weighted):
    pts, vals = torch.zeros((0, 3), device=DEV), torch.zeros((0, 4), device=DEV)
    poison((4, 7, 5, 3))
    grid, cnt = sap().point_rasterize(pts, vals, (7, 5, 3), weighted=weighted, return_counts=True)
    assert tuple(grid.shape) == (4, 7, 5, 3) and tuple(cnt.shape) == (7, 5, 3)
    assert not grid.any() and not cnt.any()


def test_rasterize_all_points_in_the_last_cell():
    rng = np.random.default_rng(21)
    pts = (np.float32(0.875) + rng.random((20000, 3), dtype=np.float32) * np.float32(0.125)).astype(np.float32)
    pts = np.minimum(pts, np.float32(1 - 2.0 ** -24))
    pts[rng.choice(20000, 5000, replace=False)] = pts[0]
    assert (np.floor(pts / np.float32(0.125)) == 7).all() and 20000 > 4 * 4096      # one cell, one digit, five sort tiles
    vals = rng.normal(size=(20000, 3)).astype(np.float32)
    k = check_raster(pts, vals, (8, 8, 8), "20000 points in cell (7,7,7) of 8^3")
    corners = k[np.ix_([0, 7], [0, 7], [0, 7])]
    assert (corners == 20000).all() and k.sum() == 8 * 20000                         # all eight nodes, through the wrap


def test_rasterize_two_cubed():
    pts, vals = random_cloud(5000, 2, 4)
    k = check_raster(pts, vals, (2, 2, 2), "5000 points at 2^3")
    assert k.sum() == 8 * 5000


def test_rasterize_fourth_sort_pass():
    res = (257, 256, 256)
    rng = np.random.default_rng(257)
    pts = np.minimum(rng.random((5000, 3), dtype=np.float32), np.float32(1 - 2.0 ** -24))
    pts[rng.choice(5000, 100, replace=False), 0] = np.float32(0.998)
    cell = ((np.floor(pts[:, 0] / (np.float32(1) / np.float32(257))).astype(np.int64) * 256
             + np.floor(pts[:, 1] * np.float32(256)).astype(np.int64)) * 256 + np.floor(pts[:, 2] * np.float32(256)).astype(np.int64))
    assert (cell >= 2 ** 24).sum() >= 100 and (cell < 2 ** 24).sum() >= 4000         # the fourth digit is 1 for some, 0 for most
    vals = rng.normal(size=(5000, 1)).astype(np.float32)
    k = check_raster(pts, vals, res, "5000 points at (257,256,256)")
    assert k.sum() == 8 * 5000


# ------------------------------------------------------------------------------------------------ 7. empty clouds
@pytest.mark.parametrize("shift", [True, False])
def test_dpsr_refuses_an_empty_cloud(shift):
    dpsr = sap().DPSR((8, 8, 8), sig=2, shift=shift)
    for shape in ((0, 3), (1, 0, 3)):
        with pytest.raises(ValueError):
            dpsr(torch.zeros(shape, device=DEV), torch.zeros(shape, device=DEV))
    phi = dpsr(torch.full((1, 3), 0.3, device=DEV), torch.ones((1, 3), device=DEV))    # one point is a cloud
    assert tuple(phi.shape) == (8, 8, 8)
