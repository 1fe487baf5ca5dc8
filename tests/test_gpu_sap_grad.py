"""The backward of the HIP Shape-as-Points stage (gaustudio_amd.sap over csrc/gsr_psr.hip) against its CPU model
(tests/sap_grad_model.py) and the reference's recorded float32 error (tests/golden/py_sap_grad.npz).

Bounds, and where they come from:
  * rasterize / interp / psr2mesh backward: device and model add the same float32 terms in float64, in different orders, and
    round once: 1 float32 ulp of the model's sum, plus the most two float64 orders of k terms can differ by, k * 2^-52 *
    sum|terms| (it matters only where the terms cancel to nearly nothing, as on node-aligned points).
  * normalize backward: grad_in is one float32 chain per element, the same on both sides: at most 1 ulp (it is equal);
    grad_mean is a float64 sum of the float32 grad_in in another order: count * 2^-52 * sum|grad_in|.
  * spectral backward: the forward's argument (test_gpu_sap.py).  The only input that may differ is G (2 units of 2^-24);
    then the division, the product with w_d and the product with G, one unit each at most: 5 = SPECTRAL_UNITS.
  * DPSR end to end against the float64 model: EREF_FACTOR x the reference's own float32 gradient error from the fixture
    (hipFFT and the CPU FFT are different float32 FFTs of the same error order).
  * mesh vertices, faces and vertex normals, given the same grid: exactly equal.
  * descent: the reference alone reaches 11 % of the initial loss in these 20 steps (make_sap_grad_fixture.py prints it);
    the condition is half."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sap_grad_model as gm  # noqa: E402
import sap_model as sm  # noqa: E402
from test_sap_model import fields  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))
SPECTRAL_UNITS = 5
EREF_FACTOR = 4
RES_16, RES_NC = (16, 16, 16), (12, 10, 14)


def sap():
    from gaustudio_amd import sap as s
    return s


def dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "py_sap.npz")))


@pytest.fixture(scope="module")
def gx():
    return dict(np.load(os.path.join(HERE, "golden", "py_sap_grad.npz")))


def assert_same_terms_sum(got, want64, abs64, k, what):
    """got float32 (device) against the model's float64 sum of the same float32 terms."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want64.shape, (what, got.dtype, got.shape, want64.shape)
    w32 = want64.astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(w32), np.abs(got))).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want64)
    tol = ulp + k * 2.0 ** -52 * abs64
    print(f"{what}: max err / ulp = {(err / ulp).max():.2f}, {(got != w32).sum()} of {got.size} values differ from the rounded model")
    assert (err <= tol).all(), what


def edge_cloud(n, res, channels, seed):
    """random points; an eighth on one-decimal coordinates, the last rows in the last cell of each axis (their upper corner
    wraps to node 0) and exactly on nodes (all 8 corners are the point's own node)."""
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 3), dtype=np.float32)
    pts[: n // 8] = pts[: n // 8].round(1) % 1.0
    special = []
    for d in range(3):
        p = np.full(3, 0.3, np.float32)
        p[d] = np.float32(1.0) - np.float32(0.25) / np.float32(res[d])
        special.append(p)
    special.append(np.array([1.0 - 0.5 / res[0], 1.0 - 0.5 / res[1], 1.0 - 0.5 / res[2]], np.float32))
    special.append(np.zeros(3, np.float32))
    special.append(np.array([1.0 / res[0], 0.0, (res[2] - 1.0) / res[2]], np.float32))
    special = np.minimum(np.stack(special), np.float32(1 - 2 ** -24))[:n]
    pts[n - len(special):] = special
    pts = np.minimum(pts, np.float32(1 - 2 ** -24))
    assert sm.valid(pts, res).all()
    return pts, rng.normal(size=(n, channels)).astype(np.float32)


CASES = [(1, (2, 2, 2), 1), (257, (7, 5, 3), 4), (513, (7, 5, 3), 1), (513, (7, 5, 3), 4)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n,res,channels", CASES)
def test_rasterize_backward_matches_the_model(n, res, channels, weighted):
    pts, vals = edge_cloud(n, res, channels, n + channels)
    gg = np.random.default_rng(n).normal(size=(channels,) + res).astype(np.float32)
    counts = sm.rasterize(pts, vals, res)[1]
    gv, gp, av, ap = gm.rasterize_bwd(gg, pts, vals, res, weighted, counts, with_abs=True)
    runs = []
    for _ in range(2):
        p, v = dev(pts, True), dev(vals, True)
        grid = sap().point_rasterize(p, v, res, weighted=weighted)
        assert grid.grad_fn is not None
        grid.backward(dev(gg))
        runs.append((p.grad, v.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two backward runs differ"
    assert_same_terms_sum(runs[0][1].cpu().numpy(), gv, av, 8, f"grad_values n={n} {res} C={channels} weighted={weighted}")
    assert_same_terms_sum(runs[0][0].cpu().numpy(), gp, ap, 8 * channels, f"grad_points n={n} {res} C={channels} weighted={weighted}")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("res", [RES_16, RES_NC])
def test_rasterize_backward_of_the_fixture_cloud(fx, res, weighted):
    pts, vals = fx["V"], fx["normals"]
    gg = np.stack([gm.loss_weights(res, seed=21 + c) for c in range(3)])
    counts = sm.rasterize(pts, vals, res)[1]
    gv, gp, av, ap = gm.rasterize_bwd(gg, pts, vals, res, weighted, counts, with_abs=True)
    p, v = dev(pts, True), dev(vals, True)
    grid, cnt = sap().point_rasterize(p, v, res, weighted=weighted, return_counts=True)
    assert np.array_equal(cnt.cpu().numpy(), counts) and not cnt.requires_grad
    grid.backward(dev(gg))
    assert_same_terms_sum(v.grad.cpu().numpy(), gv, av, 8, f"fixture grad_values {res} weighted={weighted}")
    assert_same_terms_sum(p.grad.cpu().numpy(), gp, ap, 24, f"fixture grad_points {res} weighted={weighted}")


def test_node_aligned_points_get_minus_r_times_the_grid_gradient(fx, gx):
    for weighted, tag in ((False, "u"), (True, "w")):
        p, v = dev(fx["quirk_pts"], True), torch.ones((2, 3), device=DEV, requires_grad=True)
        sap().point_rasterize(p, v, (8, 8, 8), weighted=weighted).sum().backward()
        assert np.array_equal(p.grad.cpu().numpy(), gx[f"quirk_{tag}_gp"]) and np.array_equal(v.grad.cpu().numpy(), gx[f"quirk_{tag}_gv"])
    assert np.array_equal(gx["quirk_u_gp"], np.full((2, 3), -24.0, np.float32))


@pytest.mark.parametrize("n,res", [(1, (2, 2, 2)), (257, (7, 5, 3)), (513, (7, 5, 3)), (4000, RES_16), (4000, RES_NC)])
def test_interp_backward_matches_the_model(fx, n, res):
    pts = fx["V"] if n == 4000 else edge_cloud(n, res, 1, n)[0]
    rng = np.random.default_rng(n + 1)
    grid = rng.normal(size=res).astype(np.float32)
    go = rng.normal(size=n).astype(np.float32)
    gp, ap = gm.interp_bwd(grid, pts, go, with_abs=True)
    s, k, a = sm.rasterize(pts, go[:, None], res)
    runs = []
    for _ in range(2):
        g, p = dev(grid, True), dev(pts, True)
        out = sap().grid_interp(g, p)
        assert out.grad_fn is not None
        out.backward(dev(go))
        runs.append((g.grad, p.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two backward runs differ"
    assert_same_terms_sum(runs[0][1].cpu().numpy(), gp, ap, 8, f"interp grad_points n={n} {res}")
    assert_same_terms_sum(runs[0][0].cpu().numpy(), s[0], a[0], int(k.max()), f"interp grad_grid n={n} {res}")


def test_interp_mean_sends_its_gradient_through_every_sample(fx):
    pts, res = fx["V"][:513], (7, 5, 3)
    grid = np.random.default_rng(8).normal(size=res).astype(np.float32)
    g, p = dev(grid, True), dev(pts, True)
    out, mean = sap().grid_interp(g, p, return_mean=True)
    assert mean.dtype == torch.float64 and mean.grad_fn is not None
    (mean * 3.0).sum().backward()
    go = np.full(513, np.float32(3.0 / 513), np.float32)
    gp, ap = gm.interp_bwd(grid, pts, go, with_abs=True)
    assert_same_terms_sum(p.grad.cpu().numpy(), gp, ap, 8, "mean -> grad_points")
    s, k, a = sm.rasterize(pts, go[:, None], res)
    assert_same_terms_sum(g.grad.cpu().numpy(), s[0], a[0], int(k.max()), "mean -> grad_grid")


@pytest.mark.parametrize("shape", [(2, 2, 2), (7, 5, 3), RES_16])
@pytest.mark.parametrize("scale,apply_tanh,shift", [(True, True, True), (True, False, True), (False, True, False), (True, True, False)])
def test_normalize_backward_matches_the_model(shape, scale, apply_tanh, shift):
    rng = np.random.default_rng(sum(shape))
    grid = rng.normal(size=shape).astype(np.float32)
    go = rng.normal(size=shape).astype(np.float32)
    m = np.array([0.37])
    runs = []
    for _ in range(2):
        g = dev(grid, True)
        mean = dev(m, True) if shift else None
        out = sap().normalize_grid(g, mean, scale=scale, apply_tanh=apply_tanh)
        assert out.grad_fn is not None
        out.backward(dev(go))
        runs.append((g.grad, mean.grad if shift else None, out.detach()))
    assert torch.equal(runs[0][0], runs[1][0]) and (not shift or torch.equal(runs[0][1], runs[1][1])), "two backward runs differ"
    a = np.abs(grid.reshape(-1)[0] - np.float32(m[0])) if shift else np.abs(grid.reshape(-1)[0])
    gin, gmean = gm.normalize_bwd32(go, runs[0][2].cpu().numpy(), a, scale, apply_tanh)
    got = runs[0][0].cpu().numpy()
    d = np.abs(got.astype(np.float64) - gin) / np.spacing(np.maximum(np.abs(got), np.abs(gin))).astype(np.float64)
    print(f"normalize backward {shape} scale={scale} tanh={apply_tanh} shift={shift}: max {d.max():.2f} ulp")
    assert d.max() <= 1
    if shift:
        assert tuple(runs[0][1].shape) == (1,) and runs[0][1].dtype == torch.float64
        assert abs(float(runs[0][1]) - gmean) <= gin.size * 2.0 ** -52 * np.abs(gin).astype(np.float64).sum()


@pytest.mark.parametrize("res", [(2, 2, 2), (9, 6, 5), RES_NC, RES_16])
def test_spectral_backward_matches_the_model(res):
    rng = np.random.default_rng(res[0])
    shape = (res[0], res[1], res[2] // 2 + 1)
    spec = (rng.normal(size=(3,) + shape) + 1j * rng.normal(size=(3,) + shape)).astype(np.complex64)
    gphi = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)
    want, scale = gm.spectral_bwd32(gphi, res, 2.0)
    runs = []
    for _ in range(2):
        x = dev(spec, True)
        Phi = sap().spectral_solve(x, res, 2.0)
        assert Phi.grad_fn is not None
        Phi.backward(dev(gphi))
        runs.append(x.grad)
    assert torch.equal(torch.view_as_real(runs[0]), torch.view_as_real(runs[1])), "two backward runs differ"
    got = runs[0].cpu().numpy()
    assert got.dtype == np.complex64 and (got[:, 0, 0, 0] == 0).all()
    err = np.maximum(np.abs(got.real.astype(np.float64) - want.real), np.abs(got.imag.astype(np.float64) - want.imag))
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"spectral backward {res}: {(got != want).sum()} of {got.size} elements differ, max err / (2^-24 scale) = "
              f"{np.nanmax(np.where(scale > 0, err / (sm.U * scale), 0)):.2f}")
    assert (err <= SPECTRAL_UNITS * sm.U * scale).all()


@pytest.mark.parametrize("key,res", [("16", RES_16), ("nc", RES_NC)])
def test_dpsr_gradients_end_to_end(fx, gx, key, res):
    W = gm.loss_weights(res)
    _, gV, gN = gm.dpsr_loss_grads(fx["V"], fx["normals"], res, 2.0, W)
    runs = []
    for batched in (False, True):
        V, N = dev(fx["V"], True), dev(fx["normals"], True)
        phi = sap().DPSR(res, sig=2)(V[None], N[None], apply_tanh=True)[0] if batched else sap().DPSR(res, sig=2)(V, N, apply_tanh=True)
        assert phi.grad_fn is not None and tuple(phi.shape) == res
        (phi * dev(W)).sum().backward()
        runs.append((V.grad, N.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two backward runs differ"
    for name, got, want in (("V", runs[0][0], gV), ("N", runs[0][1], gN)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
        eref = float(gx[f"eref_grad_{name}_{key}"])
        ref_err = np.abs(got.cpu().numpy() - gx[f"g{name}_{key}"]).max()
        print(f"DPSR {res} grad {name}: max |device - float64 model| = {err:.3e} = {err / eref:.2f} x E_ref ({eref:.3e}); "
              f"max |device - reference float32| = {ref_err:.3e}; scale {float(gx[f'gscale_{name}_{key}']):.3e}")
        assert err <= EREF_FACTOR * eref


def test_dpsr_gradients_with_tanh_outside_and_options(fx):
    """tanh applied by torch after DPSR, and the weighted / unshifted / unscaled variants, give finite gradients of the right
    shape; tanh outside equals tanh inside up to the float32 rounding of torch's own tanh backward."""
    res = RES_NC
    W = dev(gm.loss_weights(res))
    V, N = dev(fx["V"], True), dev(fx["normals"], True)
    (sap().DPSR(res, sig=2)(V, N, apply_tanh=True) * W).sum().backward()
    inside = (V.grad.clone(), N.grad.clone())
    V.grad = N.grad = None
    (torch.tanh(sap().DPSR(res, sig=2)(V, N)) * W).sum().backward()
    for a, b in zip(inside, (V.grad, N.grad)):
        assert (a - b).abs().max() <= 1e-5 * a.abs().max()
    for kw in (dict(weighted=True), dict(shift=False), dict(scale=False), dict(scale=False, shift=False)):
        V.grad = N.grad = None
        (sap().DPSR(res, sig=2, **kw)(V, N) * W).sum().backward()
        assert torch.isfinite(V.grad).all() and torch.isfinite(N.grad).all() and V.grad.abs().max() > 0 and N.grad.abs().max() > 0


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_psr2mesh_equals_the_model(name):
    g = fields(17)[name].astype(np.float32)[:, :15, 1:]
    v_unit, faces, normals = gm.psr2mesh(g)
    dv = np.random.default_rng(6).normal(size=v_unit.shape).astype(np.float32)
    want, vals = gm.psr2mesh_bwd(g, dv)
    _, k, a = sm.rasterize(v_unit, vals[:, None], g.shape)
    gv, gf, gn = sap().marching_cubes(dev(g), 0.0, return_normals=True)
    assert np.array_equal(gn.cpu().numpy(), normals), "vertex normals differ"
    runs = []
    for _ in range(2):
        grid = dev(g, True)
        vu, f = sap().psr2mesh(grid)
        assert vu.grad_fn is not None and not f.requires_grad and f.dtype == torch.int32
        assert np.array_equal(vu.detach().cpu().numpy(), v_unit) and np.array_equal(f.cpu().numpy(), faces) and torch.equal(f, gf)
        (vu * dev(dv)).sum().backward()
        runs.append(grid.grad)
    assert torch.equal(runs[0], runs[1]), "two backward runs differ"
    assert_same_terms_sum(runs[0].cpu().numpy(), want, a[0], int(k.max()), f"psr2mesh grad_grid {name}")
    plain = sap().psr2mesh(dev(g))
    assert plain[0].grad_fn is None and np.array_equal(plain[0].cpu().numpy(), v_unit)


def test_nothing_requires_grad_nothing_records(fx):
    s = sap()
    V, N = dev(fx["V"]), dev(fx["normals"])
    grid = s.point_rasterize(V, N, RES_NC)
    spec = torch.fft.rfftn(grid, dim=(1, 2, 3))
    outs = [grid, s.grid_interp(grid[0], V), s.spectral_solve(spec, RES_NC, 2.0), s.normalize_grid(grid[0]),
            s.DPSR(RES_NC, sig=2)(V, N), s.psr2mesh(s.DPSR(RES_NC, sig=2)(V, N, apply_tanh=True))[0]]
    Vg, Ng = dev(fx["V"], True), dev(fx["normals"], True)
    with torch.no_grad():
        outs += [s.point_rasterize(Vg, Ng, RES_NC), s.DPSR(RES_NC, sig=2)(Vg, Ng), s.grid_interp(grid[0], Vg)]
    for o in outs:
        assert o.grad_fn is None and not o.requires_grad
    assert torch.equal(outs[-2], outs[4]), "the grad path and the plain path of DPSR give different grids"
    assert torch.equal(s.DPSR(RES_NC, sig=2)(Vg, Ng).detach(), outs[4])
    shape = s.ShapeAsPoints.from_pointcloud(dev(fx["points"]), dev(fx["normals"]), dpsr_res=16)
    assert all(not p.requires_grad for p in shape.parameters()) and shape.generate_mesh()[0].grad_fn is None


def test_adam_descends_on_the_grid_loss():
    start, nrm, target = gm.descent_clouds()
    s = sap()
    shape = s.ShapeAsPoints.from_pointcloud(dev(start), dev(nrm), dpsr_res=16, dpsr_sig=2)
    with torch.no_grad():
        tgt = s.DPSR(RES_16, sig=2)(s.ShapeAsPoints.transform(dev(target), shape.center, shape.scale), dev(nrm), apply_tanh=True)
    assert shape.requires_grad_() is shape
    params = shape.parameters()
    assert len(params) == 2 and params[0] is shape.xyz and params[1] is shape.normals and all(p.is_leaf and p.requires_grad for p in params)
    opt = torch.optim.Adam(params, lr=1e-2)
    losses = []
    for _ in range(21):
        opt.zero_grad()
        loss = ((shape.psr_grid() - tgt) ** 2).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print(f"descent: loss {losses[0]:.3e} -> {losses[20]:.3e} after 20 Adam steps ({100 * losses[20] / losses[0]:.1f} % of the initial loss)")
    assert losses[20] < 0.5 * losses[0]
    # the mesh of the fitted cloud carries gradients back to the parameters
    opt.zero_grad()
    vertices, faces, v_unit = shape.generate_mesh()
    assert vertices.grad_fn is not None and not faces.requires_grad and len(faces) > 0
    (vertices ** 2).sum().backward()
    assert shape.xyz.grad.abs().max() > 0 and shape.normals.grad.abs().max() > 0
    assert torch.isfinite(shape.xyz.grad).all() and torch.isfinite(shape.normals.grad).all()
