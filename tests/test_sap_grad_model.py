"""The CPU model of the Shape-as-Points backward (tests/sap_grad_model.py) against the gradients torch autograd gave the
reference's Python on the CPU (tests/golden/py_sap_grad.npz, written by tests/golden/make_sap_grad_fixture.py), against central
finite differences in float64, and against torch's convention for complex gradients.

Bounds.  A gradient entry is a sum of k float32 terms (k = 8 for grad_values and grid_interp, 8 C = 24 for grad_points of
point_rasterize, the pairs on a node for the grid gradient of grid_interp), which the reference adds in float32: the
summation bound used for the forward (tests/test_sap_model.py), (k - 1) * 2^-24 * sum|terms| around the model's float64 sum.
The whole solver is held to E_ref, the reference's own float32 error against the float64 model, which the fixture generator
measured, and E_ref itself to 1e-6 of the gradient's scale."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sap_grad_model as gm  # noqa: E402
import sap_model as sm  # noqa: E402
from test_sap_model import fields  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
RES_16, RES_NC, N_RAS = (16, 16, 16), (12, 10, 14), 512


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "py_sap.npz")))


@pytest.fixture(scope="module")
def gx():
    return dict(np.load(os.path.join(HERE, "golden", "py_sap_grad.npz")))


def test_the_module_offers_the_differentiable_interface():
    import inspect
    from gaustudio_amd import sap
    assert callable(sap.psr2mesh)
    assert callable(sap.ShapeAsPoints.requires_grad_) and callable(sap.ShapeAsPoints.parameters)
    assert "return_normals" in inspect.signature(sap.marching_cubes).parameters


@pytest.mark.parametrize("key,res", [("16", RES_16), ("nc", RES_NC)])
def test_dpsr_gradients_within_eref_of_the_reference(fx, gx, key, res):
    _, gV, gN = gm.dpsr_loss_grads(fx["V"], fx["normals"], res, 2.0, gm.loss_weights(res))
    for name, mod in (("V", gV), ("N", gN)):
        err = np.abs(gx[f"g{name}_{key}"] - mod).max()
        eref, scale = float(gx[f"eref_grad_{name}_{key}"]), float(gx[f"gscale_{name}_{key}"])
        print(f"DPSR {res} grad {name}: max |reference - model| = {err:.3e}, E_ref = {eref:.3e} = {eref / scale:.2e} of scale")
        assert err <= eref and eref <= 1e-6 * scale


@pytest.mark.parametrize("weighted,tag", [(False, "u"), (True, "w")])
def test_rasterize_gradients_within_the_summation_bound_of_the_reference(fx, gx, weighted, tag):
    P, vals = fx["V"][:N_RAS], fx["normals"][:N_RAS]
    Wc = np.stack([gm.loss_weights(RES_NC, seed=21 + c) for c in range(3)])
    counts = sm.rasterize(P, vals, RES_NC)[1]
    gv, gp, av, ap = gm.rasterize_bwd(Wc, P, vals, RES_NC, weighted, counts, with_abs=True)
    ev, ep = np.abs(gx[f"ras_{tag}_gv"] - gv), np.abs(gx[f"ras_{tag}_gp"] - gp)
    bv, bp = 7 * sm.U * av, 23 * sm.U * ap
    print(f"rasterize weighted={weighted}: grad_values max err {ev.max():.3e} (bound {bv.max():.3e}), grad_points {ep.max():.3e} "
          f"(bound {bp.max():.3e})")
    assert (ev <= bv).all() and (ep <= bp).all()


def test_node_aligned_points_get_minus_r_times_the_grid_gradient(fx, gx):
    """a point on a node: all 8 corners are that node, only corner (0,0,0) has weight 1 and only it has a non-zero
    derivative, -R on every axis (sign(0) = 0 for the others)."""
    ones, g = np.ones((2, 3), np.float32), np.ones((3, 8, 8, 8), np.float32)
    counts = sm.rasterize(fx["quirk_pts"], ones, (8, 8, 8))[1]
    for weighted, tag, div in ((False, "u", 1.0), (True, "w", 8.0)):
        gv, gp = gm.rasterize_bwd(g, fx["quirk_pts"], ones, (8, 8, 8), weighted, counts)
        assert np.array_equal(gp, np.full((2, 3), -8.0 * 3 / div)) and np.array_equal(gv, np.full((2, 3), 1.0 / div))
        assert np.array_equal(gx[f"quirk_{tag}_gp"], gp.astype(np.float32)) and np.array_equal(gx[f"quirk_{tag}_gv"], gv.astype(np.float32))


def test_interp_gradients_within_the_summation_bound_of_the_reference(fx, gx):
    P = fx["V"][:N_RAS]
    Wg = gm.loss_weights(RES_16, seed=31)
    go = np.random.default_rng(32).normal(size=N_RAS).astype(np.float32)
    gp, ap = gm.interp_bwd(Wg, P, go, with_abs=True)
    ep = np.abs(gx["interp_gp"] - gp)
    print(f"grid_interp: grad_points max err {ep.max():.3e} (bound {(7 * sm.U * ap).max():.3e}), "
          f"max err / (2^-24 sum|terms|) = {(ep / np.maximum(sm.U * ap, 1e-300)).max():.2f}")
    assert (ep <= 7 * sm.U * ap).all()
    s, k, a = sm.rasterize(P, go[:, None], RES_16)
    eg = np.abs(gx["interp_gg"] - s[0])
    assert (eg <= np.maximum(k - 1, 0) * sm.U * a[0]).all()
    assert np.array_equal(gm.interp_bwd_grid(P, go, RES_16), s[0])


def away_from_faces(pts, size, margin=0.05):
    q = np.asarray(pts, np.float64) * np.asarray(size, np.float64)
    f = q - np.floor(q)
    return ((f > margin) & (f < 1 - margin)).all(1)


def fd(f, x, i, d, h=1e-6):
    xp, xm = x.copy(), x.copy()
    xp[i, d] += h
    xm[i, d] -= h
    return (f(xp) - f(xm)) / (2 * h)


def test_the_two_gathers_against_finite_differences():
    rng = np.random.default_rng(5)
    size = (7, 5, 3)
    P = rng.random((40, 3))
    P = P[away_from_faces(P, size)]
    vals = rng.normal(size=(len(P), 2))
    W = rng.normal(size=(2,) + size)
    grid = rng.normal(size=size)
    go = rng.normal(size=len(P))
    assert len(P) >= 10
    for weighted in (False, True):
        counts = gm.rasterize_fwd(P, vals, size, weighted)[1]
        gv, gp = gm.rasterize_bwd(W, P, vals, size, weighted, counts, dtype=np.float64)
        for i in range(0, len(P), 3):
            for d in range(3):
                want = fd(lambda x: (gm.rasterize_fwd(x, vals, size, weighted)[0] * W).sum(), P, i, d)
                assert abs(gp[i, d] - want) <= 1e-6 * max(1.0, abs(want))
            for c in range(2):
                want = fd(lambda v: (gm.rasterize_fwd(P, v, size, weighted)[0] * W).sum(), vals, i, c)
                assert abs(gv[i, c] - want) <= 1e-6 * max(1.0, abs(want))
    gp = gm.interp_bwd(grid, P, go, dtype=np.float64)
    for i in range(0, len(P), 3):
        for d in range(3):
            want = fd(lambda x: (gm.interp_fwd(grid, x) * go).sum(), P, i, d)
            assert abs(gp[i, d] - want) <= 1e-6 * max(1.0, abs(want))


def test_the_solver_against_finite_differences(fx):
    keep = away_from_faces(fx["V"].astype(np.float64), RES_NC)
    V, N = fx["V"][keep][:200].astype(np.float64), fx["normals"][keep][:200].astype(np.float64)
    W = gm.loss_weights(RES_NC)
    _, gV, gN = gm.dpsr_loss_grads(V, N, RES_NC, 2.0, W, wdtype=np.float64)
    v0 = gm.dpsr_loss_grads(V, N, RES_NC, 2.0, W, np.float64, False)[1]      # |v0| is a constant of the backward: held still
    scale_v, scale_n = np.abs(gV).max(), np.abs(gN).max()
    for i in (0, 17, 101, 199):
        for d in range(3):
            wv = fd(lambda x: gm.dpsr_loss_grads(x, N, RES_NC, 2.0, W, np.float64, False, v0)[0], V, i, d)
            wn = fd(lambda x: gm.dpsr_loss_grads(V, x, RES_NC, 2.0, W, np.float64, False, v0)[0], N, i, d)
            assert abs(gV[i, d] - wv) <= 1e-6 * scale_v and abs(gN[i, d] - wn) <= 1e-6 * scale_n


def test_spectral_rule_is_torchs_convention_for_complex_gradients():
    size, sig = (4, 4, 4), 2.0
    rng = np.random.default_rng(9)
    spec = (rng.normal(size=(3, 4, 4, 3)) + 1j * rng.normal(size=(3, 4, 4, 3)))
    gphi = (rng.normal(size=(4, 4, 3)) + 1j * rng.normal(size=(4, 4, 3)))
    c = torch.from_numpy(gm.spectral_coeffs(size, sig))
    x = torch.from_numpy(spec).requires_grad_(True)
    Phi = (c * x).sum(0)
    (want,) = torch.autograd.grad(Phi, x, torch.from_numpy(gphi))
    want = want.numpy()
    assert np.abs(np.conj(c.numpy()) * gphi[None] - want).max() <= 1e-12 * np.abs(want).max()
    got, scale = gm.spectral_bwd32(gphi.astype(np.complex64), size, sig)
    assert (got[:, 0, 0, 0] == 0).all()
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    assert (err <= 8 * sm.U * scale + 1e-30).all()          # float32 input, filter, division, two products and slack
    # the forward the rule belongs to: Phi of the float32 model is sum_d c_d N_d
    phi32, _ = sm.spectral32(spec.astype(np.complex64), size, sig)
    assert np.abs(phi32 - Phi.detach().numpy()).max() <= 1e-5 * np.abs(phi32).max()


def test_normalize_rule_against_finite_differences():
    rng = np.random.default_rng(2)
    v = rng.normal(size=105)
    go = rng.normal(size=105)
    m, a = 0.3, abs(v[0] - 0.3)
    f = lambda vv, mm: (np.tanh(-(vv - mm) / a * 0.5) * go).sum()                      # noqa: E731  |v0| held still
    out = np.tanh(-(v - m) / a * 0.5).astype(np.float32)
    gin, gmean = gm.normalize_bwd32(go.astype(np.float32), out, np.float32(a), True, True)
    h = 1e-6
    for i in (0, 1, 50, 104):
        e = np.zeros(105)
        e[i] = h
        assert abs(gin[i] - (f(v + e, m) - f(v - e, m)) / (2 * h)) <= 1e-5 * np.abs(gin).max()
    assert abs(gmean - (f(v, m + h) - f(v, m - h)) / (2 * h)) <= 1e-5 * np.abs(gin).sum()


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_mesh_rule_spreads_every_vertex_value_with_weights_that_sum_to_one(name):
    g = fields(17)[name].astype(np.float32)
    v_unit, faces, n = gm.psr2mesh(g)
    dv = np.random.default_rng(4).normal(size=v_unit.shape).astype(np.float32)
    grad_grid, vals = gm.psr2mesh_bwd(g, dv)
    assert len(vals) == len(v_unit) > 100 and grad_grid.shape == g.shape
    total = vals.astype(np.float64).sum()
    assert abs(grad_grid.sum() - total) <= 8 * sm.U * np.abs(vals).astype(np.float64).sum()
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() <= 4 * sm.U


def test_normals_of_a_sphere_point_outwards():
    n = 24
    x = np.arange(n, dtype=np.float64)
    c = np.array([11.3, 12.1, 11.7])
    d = np.sqrt((x[:, None, None] - c[0]) ** 2 + (x[None, :, None] - c[1]) ** 2 + (x[None, None, :] - c[2]) ** 2)
    g = (d - 8.2).astype(np.float32)                       # an index-unit distance field
    v, _ = sm.marching_cubes(g, 0.0)
    nrm = gm.mc_normals(g, 0.0).astype(np.float64)
    r = v.astype(np.float64) - c
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    cos = (nrm * r).sum(1)
    print(f"sphere normals: min cos = {cos.min():.6f}")
    assert cos.min() > 0.999                               # central differences of a radius-8 sphere: O(h^2 / r^2) off radial
    # one-sided differences on the faces of the grid: a plane field crossing the boundary keeps its exact normal
    p = (0.3 * x[:, None, None] + 0.5 * x[None, :, None] - 0.2 * x[None, None, :] - 4.05).astype(np.float32)
    want = np.array([0.3, 0.5, -0.2]) / np.linalg.norm([0.3, 0.5, -0.2])
    assert np.abs(gm.mc_normals(p, 0.0) - want).max() < 1e-5
