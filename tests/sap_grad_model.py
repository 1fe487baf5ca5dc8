"""CPU model of the backward of gaustudio_amd.sap (csrc/gsr_psr.hip), written from the gradient contract in INTEGRATION.md
s17a -- not from the reference's program text.  numpy; torch (CPU, float64) only for the adjoints of the two FFTs.

The five rules, each with `dtype`: float32 = the device's chain of float32 terms, returned as their exact float64 sums (what
the device rounds once); float64 = the same formulas in float64 throughout (weights too), what finite differences check.

  * corners_d(): index, weight and weight derivative of the 8 corners: a factor |p - pos| / cs differentiates to
    sign(p - pos) / cs with sign(0) = 0; dw[:, k, d] is the weight of corner k with the factor of axis d so replaced;
  * rasterize_bwd(), interp_bwd(): gathers over the 8 corners (k0 slowest);
  * spectral_bwd32(): grad_N_d = conj(c_d) grad_Phi, zero at element 0, in the device's float32 chain;
  * normalize_bwd32(): grad_in and grad_mean = -sum(grad_in), |v0| a constant;
  * mc_normals(), psr2mesh_bwd(): vertex normals and the rule dv/dphi = -n spread trilinearly;
  * dpsr_loss_grads(): loss = sum(tanh(DPSR(V, N)) * W) and its V / N gradients in float64 (wdtype: float32 weights as in
    sap_model.dpsr64, or float64 throughout for finite differences).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sap_model as sm  # noqa: E402

f32, f64 = np.float32, np.float64


def loss_weights(size, seed=11):
    """the fixed weights W of the scalar loss sum(tanh(phi) * W)."""
    return np.random.default_rng(seed).normal(size=tuple(size)).astype(f32)


# ------------------------------------------------------------------------------------------------------ corners
def _axis_d(p, size, dtype):
    p = np.asarray(p, dtype)
    cs = dtype(1.0) / dtype(size)
    q = p / cs
    f0 = np.floor(q)
    i0 = f0.astype(np.int64)
    i1 = np.fmod(np.ceil(q), dtype(size)).astype(np.int64)
    x0 = f0 * cs
    x1 = (f0 + dtype(1.0)) * cs
    w = (np.abs(p - x1) / cs, np.abs(p - x0) / cs)
    d = (np.sign(p - x1) / cs, np.sign(p - x0) / cs)
    assert w[0].dtype == dtype and d[0].dtype == dtype
    return (i0, i1), w, d


def corners_d(pts, size, dtype=f32):
    """-> idx [N,8] int64, w [N,8], dw [N,8,3] in `dtype`; corner k = (k0, k1, k2), k0 slowest."""
    pts = np.asarray(pts, dtype)
    assert sm.valid(pts.astype(f32), size).all()
    ax = [_axis_d(pts[:, d], size[d], dtype) for d in range(3)]
    n = len(pts)
    idx = np.empty((n, 8), np.int64)
    w = np.empty((n, 8), dtype)
    dw = np.empty((n, 8, 3), dtype)
    for c in range(8):
        k = (c >> 2, (c >> 1) & 1, c & 1)
        idx[:, c] = (ax[0][0][k[0]] * size[1] + ax[1][0][k[1]]) * size[2] + ax[2][0][k[2]]
        wx, wy, wz = ax[0][1][k[0]], ax[1][1][k[1]], ax[2][1][k[2]]
        sx, sy, sz = ax[0][2][k[0]], ax[1][2][k[1]], ax[2][2][k[2]]
        w[:, c] = (wx * wy) * wz
        dw[:, c, 0] = (sx * wy) * wz
        dw[:, c, 1] = (wx * sy) * wz
        dw[:, c, 2] = (wx * wy) * sz
    return idx, w, dw


def _sum_corners(t):
    """[N,8,...] terms -> float64 sums over the corners in corner order."""
    t = t.astype(f64)
    s = np.zeros(t.shape[:1] + t.shape[2:])
    for c in range(8):
        s = s + t[:, c]
    return s


# ------------------------------------------------------------------------------------------------------ forward (for FD)
def rasterize_fwd(pts, vals, size, weighted, dtype=f64):
    idx, w, _ = corners_d(pts, size, dtype)
    nn = size[0] * size[1] * size[2]
    vals = np.asarray(vals, dtype)
    k = np.bincount(idx.ravel(), minlength=nn)
    out = np.stack([np.bincount(idx.ravel(), weights=(w * vals[:, c:c + 1]).ravel().astype(f64), minlength=nn)
                    for c in range(vals.shape[1])])
    if weighted:
        out = out / np.maximum(k, 1)[None]
    return out.reshape((vals.shape[1],) + tuple(size)), k.reshape(size)


def interp_fwd(grid, pts, dtype=f64):
    idx, w, _ = corners_d(pts, grid.shape, dtype)
    return _sum_corners(np.asarray(grid, dtype).ravel()[idx] * w)


# ------------------------------------------------------------------------------------------------------ the gathers
def rasterize_bwd(gg, pts, vals, size, weighted, counts=None, dtype=f32, with_abs=False):
    """gg [C,R0,R1,R2], counts [R0,R1,R2] (the forward's, needed when weighted) -> (grad_values [N,C], grad_points [N,3]),
    float64 sums of `dtype` terms: w g' and (dw g') v, g' = g / max(count, 1) when weighted.  with_abs adds the two sums of
    |term| (what a summation bound is measured against)."""
    idx, w, dw = corners_d(pts, size, dtype)
    vals = np.asarray(vals, dtype)
    C = vals.shape[1]
    g = np.asarray(gg, dtype).reshape(C, -1)
    if weighted:
        g = g / np.maximum(np.asarray(counts).reshape(-1), 1).astype(dtype)[None]
    assert g.dtype == dtype
    gv, av = np.empty((len(idx), C)), np.empty((len(idx), C))
    gp, ap = np.zeros((len(idx), 3)), np.zeros((len(idx), 3))
    for c in range(C):
        gc = g[c][idx]                                                   # [N,8]
        gv[:, c] = _sum_corners(w * gc)
        av[:, c] = _sum_corners(np.abs(w * gc))
        t = (dw * gc[:, :, None]) * vals[:, c][:, None, None]
        assert t.dtype == dtype
        gp = gp + _sum_corners(t)
        ap = ap + _sum_corners(np.abs(t))
    return (gv, gp, av, ap) if with_abs else (gv, gp)


def interp_bwd(grid, pts, gout, dtype=f32, with_abs=False):
    """-> grad_points [N,3]: float64 sums of the `dtype` terms (grid[node] dw) grad_out (with_abs: and the sums of |term|)."""
    idx, _, dw = corners_d(pts, grid.shape, dtype)
    lat = np.asarray(grid, dtype).ravel()[idx]
    t = (lat[:, :, None] * dw) * np.asarray(gout, dtype)[:, None, None]
    assert t.dtype == dtype
    return (_sum_corners(t), _sum_corners(np.abs(t))) if with_abs else _sum_corners(t)


def interp_bwd_grid(pts, gout, size):
    """the adjoint scatter: float64 sums of the float32 terms w * grad_out per node."""
    return sm.rasterize(pts, np.asarray(gout, f32)[:, None], size)[0][0]


# ------------------------------------------------------------------------------------------------------ streams
def spectral_coeffs(size, sig):
    """c_d of Phi = sum_d c_d N_d in float64: -i w_d G / (Lap + 1e-6), zero at element 0.  [3,R0,R1,R2h] complex128."""
    K = sm._freqs(size)
    dis = np.sqrt(K[0] ** 2 + K[1] ** 2 + K[2] ** 2)
    G = np.exp(-0.5 * ((sig * 2.0) * dis / float(size[0])) ** 2)
    om = [K[d] * 2.0 * np.pi for d in range(3)]
    lap = -(om[0] ** 2 + om[1] ** 2 + om[2] ** 2)
    c = np.stack([-1j * om[d] * G / (lap + 1e-6) for d in range(3)])
    c[:, 0, 0, 0] = 0
    return c


def spectral_bwd32(gphi, size, sig):
    """gphi complex64 [R0,R1,R2h] -> (grad_spectrum complex64 [3,...], scale float64 [3,...] = (|Re a| + |Im a|) |w_d| G, the
    magnitude one float32 rounding is measured against).  Chain: a = gphi / den, (-Im a w_d, Re a w_d), times G."""
    gphi = np.asarray(gphi, np.complex64)
    G = sm.gaussian_filter32(size, sig)
    K = sm._freqs(size)
    om = [(K[d].astype(f32) * f32(2.0)) * f32(np.pi) for d in range(3)]
    lap = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]
    den = (-lap) + f32(1e-6)
    ar, ai = gphi.real / den, gphi.imag / den
    out = np.empty((3,) + gphi.shape, np.complex64)
    scale = np.empty((3,) + gphi.shape)
    for d in range(3):
        re, im = ((-ai) * om[d]) * G, (ar * om[d]) * G
        assert re.dtype == f32
        out[d].real, out[d].imag = re, im
        scale[d] = (np.abs(ar.astype(f64)) + np.abs(ai.astype(f64))) * np.abs(om[d].astype(f64)) * G
    out[:, 0, 0, 0] = 0
    return out, scale


def normalize_bwd32(gout, out, a, scale=True, apply_tanh=False):
    """float32 chain: g = grad_out (1 - out^2) [tanh]; (-g) / a * 0.5 [scale].  -> (grad_in float32, grad_mean float64)."""
    g = np.asarray(gout, f32)
    if apply_tanh:
        o = np.asarray(out, f32)
        g = g * (f32(1.0) - o * o)
    if scale:
        g = (-g) / f32(a) * f32(0.5)
    assert g.dtype == f32
    return g, -g.astype(f64).sum()


# ------------------------------------------------------------------------------------------------------ mesh rule
def node_gradient(grid):
    """[R0,R1,R2,3] float32: central differences in index units, one-sided on the faces of the grid."""
    g = np.ascontiguousarray(grid, f32)
    out = np.empty(g.shape + (3,), f32)
    for d in range(3):
        gm = np.moveaxis(g, d, 0)
        o = np.empty_like(gm)
        o[1:-1] = (gm[2:] - gm[:-2]) * f32(0.5)
        o[0] = gm[1] - gm[0]
        o[-1] = gm[-1] - gm[-2]
        out[..., d] = np.moveaxis(o, 0, d)
    return out


def mc_normals(grid, level=0.0):
    """unit vertex normals [nv,3] float32 in the vertex order of sap_model.marching_cubes: ga + t (gb - ga) at the vertex's own
    t, divided by max(|n|, 1e-6); float32 operation for operation."""
    g = np.ascontiguousarray(grid, f32)
    R = g.shape
    level = f32(level)
    inside = g < level
    flags = np.zeros(R + (3,), bool)
    flags[:-1, :, :, 0] = inside[:-1] != inside[1:]
    flags[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    flags[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    hit = np.nonzero(flags.reshape(-1))[0]
    node, axis = hit // 3, hit % 3
    stride = np.asarray((R[1] * R[2], R[2], 1))
    gf = g.reshape(-1)
    a = gf[node]
    b = gf[node + stride[axis]]
    t = (level - a) / (b - a)
    ng = node_gradient(g).reshape(-1, 3)
    ga, gb = ng[node], ng[node + stride[axis]]
    n = ga + t[:, None] * (gb - ga)
    ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    n = n / np.maximum(ln, f32(1e-6))[:, None]
    assert n.dtype == f32
    return n


def psr2mesh(grid):
    """-> (v_unit float32 [nv,3] = vertices / (R0, R1, R2), faces, normals)."""
    v, f = sm.marching_cubes(grid, 0.0)
    return v / np.asarray(grid.shape, f32)[None], f, mc_normals(grid, 0.0)


def mesh_values(dv, normals):
    """-<dL/dv, n> in float32: -((dv0 n0 + dv1 n1) + dv2 n2)."""
    dv, n = np.asarray(dv, f32), np.asarray(normals, f32)
    return -((dv[:, 0] * n[:, 0] + dv[:, 1] * n[:, 1]) + dv[:, 2] * n[:, 2])


def psr2mesh_bwd(grid, dv):
    """grad_grid as float64 sums of the float32 terms w * (-<dL/dv, n>), and the values themselves."""
    v_unit, _, n = psr2mesh(grid)
    vals = mesh_values(dv, n)
    return sm.rasterize(v_unit, vals[:, None], grid.shape)[0][0], vals


# ------------------------------------------------------------------------------------------------------ the whole solver
def _fft_vjp(fn, x, g):
    import torch
    xt = torch.from_numpy(np.ascontiguousarray(x)).requires_grad_(True)
    y = fn(xt)
    (gx,) = torch.autograd.grad(y, xt, torch.from_numpy(np.ascontiguousarray(g)).to(y.dtype))
    return gx.numpy()


def dpsr_loss_grads(V, N, size, sig, W, wdtype=f32, want_grads=True, v0=None):
    """loss = sum(tanh(DPSR(V, N; sig, scale, shift, unweighted)) * W) in float64 (weights in `wdtype`) and its gradients
    towards V and N by the five rules; |v0| a constant, the FFT adjoints from torch (float64).  v0: use this |v0| instead of
    the cloud's own (finite differences must hold the detached constant still); want_grads=False returns (loss, |v0|)."""
    import torch
    size = tuple(size)
    idx, w, dw = corners_d(V, size, wdtype)
    w, dw = w.astype(f64), dw.astype(f64)
    N = np.asarray(N, f64)
    n, nn = len(idx), size[0] * size[1] * size[2]
    ras = np.stack([np.bincount(idx.ravel(), weights=(w * N[:, c:c + 1]).ravel(), minlength=nn) for c in range(3)])
    ras = ras.reshape((3,) + size)
    c = spectral_coeffs(size, sig)
    Phi = (c * np.fft.rfftn(ras, axes=(1, 2, 3))).sum(0)
    phi = np.fft.irfftn(Phi, s=size, axes=(0, 1, 2))
    m = (phi.ravel()[idx] * w).sum(1).mean()
    v = phi - m
    a = abs(v[0, 0, 0]) if v0 is None else v0
    t = np.tanh(-v / a * 0.5)
    W = np.asarray(W, f64)
    loss = float((t * W).sum())
    if not want_grads:
        return loss, a
    gin = W * (1 - t * t) * (-0.5 / a)
    go = -gin.sum() / n                                           # the mean's gradient on every sample
    gphi = gin + np.bincount(idx.ravel(), weights=(w * go).ravel(), minlength=nn).reshape(size)
    gV = (phi.ravel()[idx][:, :, None] * dw).sum(1) * go
    gPhi = _fft_vjp(lambda x: torch.fft.irfftn(x, s=size, dim=(0, 1, 2)), Phi, gphi)
    gspec = np.conj(c) * gPhi[None]
    gras = _fft_vjp(lambda x: torch.fft.rfftn(x, dim=(1, 2, 3)), ras, gspec).reshape(3, -1)
    gN = np.stack([(w * gras[ch][idx]).sum(1) for ch in range(3)], 1)
    for ch in range(3):
        gV = gV + (dw * gras[ch][idx][:, :, None]).sum(1) * N[:, ch:ch + 1]
    return loss, gV, gN


# ------------------------------------------------------------------------------------------------------ descent
def descent_clouds(n=2000):
    """The descent of the GPU test and of the fixture generator: (start, normals, target) float32 in world units.  target = the
    noisy ellipsoid of sap_model (semi-axes 1, 0.7, 0.5), start = the same samples stretched towards a sphere; the unit cube
    is the one ShapeAsPoints.from_pointcloud derives from `start` (sap_model.unit_cube), the target mapped into it."""
    target, nrm = sm.ellipsoid_cloud(n, seed=3)
    start = (target * np.array([1.0, 1.25, 1.6], f32)).astype(f32)
    return start, nrm, target
