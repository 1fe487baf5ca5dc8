"""Shape-as-Points meshing on the GPU (csrc/gsr_psr.hip): what gs-extract-pcd --meshing sap runs on the cleaned cloud,
`mesh_sap` -> `ShapeAsPoints.from_o3d_pointcloud(pcd).to_o3d_mesh()` (gaustudio/models/sap.py), i.e. the Poisson solver `DPSR`
of gaustudio/utils/graphics_utils.py:19-333 and a marching cubes over its grid (the reference goes through skimage on the CPU).

    grid = point_rasterize(pts, vals, (R0, R1, R2), weighted=True)       # graphics_utils.point_rasterize
    fv = grid_interp(grid, pts)                                            # graphics_utils.grid_interp
    phi = DPSR((R0, R1, R2), sig=2)(V, N)                                  # rasterize -> rfftn -> spectral solve -> irfftn -> normalise
    verts, faces = marching_cubes(phi, level=0.0)                          # index units
    v_unit, faces = psr2mesh(phi)                                          # graphics_utils.PSR2Mesh: unit-cube vertices
    vertices, faces = mesh_sap(points, normals, dpsr_res=256)              # the whole stage, world units

DIFFERENTIABLE, as the reference's DPSR (an nn.Module of differentiable torch ops) and PSR2Mesh (an autograd Function) are:
point_rasterize, grid_interp, spectral_solve, normalize_grid, DPSR and psr2mesh record a backward whenever grad mode is on and
one of their inputs requires grad; ShapeAsPoints.requires_grad_() turns the cloud (logit-space xyz, normals) into the
parameters Shape-as-Points exists to optimise.  With no input requiring grad, or under torch.no_grad(), every function takes
the forward-only path and returns tensors without a grad_fn.  First derivatives only.  The two FFTs are torch.fft (hipFFT) and
differentiate themselves; everything between and around them, forward and backward, is hand-written HIP.  Deterministic in
both directions: no float atomics, bit-identical from run to run.

Contract and quirks: INTEGRATION.md s17 (forward), s17a (gradients).  ROCm tensors only, no CPU fallback; every call runs on
the current stream of the tensors' device.
"""
import ctypes
import functools

import torch
from torch.autograd.function import once_differentiable

from ._abi import Workspace, call, on_rocm
from .pcd_fusion import _ERRORS, _device_tensor

MAX_CHANNELS = 4


def _res(size):
    try:
        res = tuple(int(r) for r in size)
    except TypeError:
        raise TypeError("size must be a sequence of three ints") from None
    if len(res) != 3 or any(int(r) != r0 for r, r0 in zip(res, size)):
        raise ValueError(f"size must be three ints, got {size}")
    if min(res) < 2 or res[0] * res[1] * res[2] >= 2 ** 30:
        raise ValueError(f"every grid size must be >= 2 and their product < 2^30, got {res}")
    return res


def _grid(name, grid):
    if not torch.is_tensor(grid):
        raise TypeError(f"{name} must be a torch tensor")
    if grid.dim() != 3:
        raise ValueError(f"{name} must have shape [R0, R1, R2], got {list(grid.shape)}")
    if grid.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {grid.dtype}")
    return _res(grid.shape)


def _point_errors(what):
    return {-2: f"{what}: a point coordinate is not finite or lies outside [0, 1)", **_ERRORS}


@functools.lru_cache(maxsize=16)
def _res_tensor(res, device):
    """(R0, R1, R2) as a float32 tensor on `device`, made once per grid shape and device."""
    return torch.tensor(res, dtype=torch.float32, device=device)


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


# ------------------------------------------------------------------------------------------------------ the raw calls
# detached, contiguous device tensors in, fresh tensors out; the autograd Functions below and the forward-only paths share them
def _rasterize_raw(pts, vals, res, weighted, want_counts):
    dev = pts.device
    n, C = pts.shape[0], vals.shape[1]
    grid = torch.empty((C,) + res, dtype=torch.float32, device=dev)
    counts = torch.empty(res, dtype=torch.int32, device=dev) if want_counts else None
    call("gsr_psr_rasterize", dev, pts, n, vals, C, *res, bool(weighted), grid, counts, workspace=True,
         errors=_point_errors("point_rasterize"))
    return grid, counts


def _interp_raw(grid, res, pts, want_mean):
    dev = pts.device
    out = torch.empty(pts.shape[0], dtype=torch.float32, device=dev)
    mean = torch.empty(1, dtype=torch.float64, device=dev) if want_mean else None
    call("gsr_psr_interp", dev, grid, *res, pts, pts.shape[0], out, mean, workspace=True, errors=_point_errors("grid_interp"))
    return out, mean


def _normalize_raw(grid, mean, scale, apply_tanh):
    dev = grid.device
    out = torch.empty_like(grid)
    params = torch.empty(2, dtype=torch.float32, device=dev)
    call("gsr_psr_normalize", dev, grid, out, ctypes.c_longlong(grid.numel()), mean, bool(scale), bool(apply_tanh), params,
         errors=_ERRORS)
    return out, params


# ------------------------------------------------------------------------------------------------------ autograd
class _Rasterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, vals, res, weighted, want_counts):
        p, v = pts.detach().contiguous(), vals.detach().contiguous()
        grid, counts = _rasterize_raw(p, v, res, weighted, bool(weighted or want_counts))      # the backward reads them when weighted
        ctx.save_for_backward(p, v, counts)
        ctx.res, ctx.weighted = res, bool(weighted)
        ctx.set_materialize_grads(False)
        if counts is not None:
            ctx.mark_non_differentiable(counts)
        return grid, counts

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_grid, _grad_counts):
        if grad_grid is None:
            return None, None, None, None, None
        p, v, counts = ctx.saved_tensors
        dev = p.device
        gp = torch.zeros_like(p) if ctx.needs_input_grad[0] else None       # zeros: an empty cloud launches nothing
        gv = torch.zeros_like(v) if ctx.needs_input_grad[1] else None
        call("gsr_psr_rasterize_bwd", dev, grad_grid.contiguous(), p, p.shape[0], v, v.shape[1], *ctx.res, ctx.weighted, counts,
             gv, gp, workspace=True, errors=_point_errors("point_rasterize backward"))
        return gp, gv, None, None, None


class _Interp(torch.autograd.Function):
    """(samples, mean or None) of grid at pts; the mean's gradient reaches the samples as grad_mean / N."""

    @staticmethod
    def forward(ctx, grid, pts, want_mean):
        g, p = grid.detach().contiguous(), pts.detach().contiguous()
        out, mean = _interp_raw(g, tuple(g.shape), p, want_mean)
        ctx.save_for_backward(g, p)
        ctx.set_materialize_grads(False)
        return out, mean

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, grad_mean):
        if grad_out is None and grad_mean is None:
            return None, None, None
        g, p = ctx.saved_tensors
        dev, n, res = p.device, p.shape[0], tuple(g.shape)
        if grad_out is None:
            go = (grad_mean / n).to(torch.float32).expand(n).contiguous()
        else:
            go = grad_out.contiguous()
            if grad_mean is not None:
                go = go + (grad_mean / n).to(torch.float32)
        gg = gp = None
        if ctx.needs_input_grad[0]:             # the adjoint of the gather is the forward's scatter, one channel
            gg = _rasterize_raw(p, go.unsqueeze(1).contiguous(), res, False, False)[0][0]
        if ctx.needs_input_grad[1]:
            gp = torch.empty_like(p)
            call("gsr_psr_interp_bwd", dev, g, *res, p, n, go, gp, workspace=True, errors=_point_errors("grid_interp backward"))
        return gg, gp, None


class _Spectral(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spectrum, res, sig):
        ctx.res, ctx.sig = res, sig
        return _spectral_raw(spectrum.detach(), res, sig)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_phi):
        res = ctx.res
        dev = grad_phi.device
        gphi = torch.view_as_real(grad_phi.to(torch.complex64).resolve_conj().contiguous())
        gspec = torch.empty((3, res[0], res[1], res[2] // 2 + 1, 2), dtype=torch.float32, device=dev)
        call("gsr_psr_spectral_bwd", dev, gphi, *res, ctypes.c_double(ctx.sig), gspec, errors=_ERRORS)
        return torch.view_as_complex(gspec), None, None


class _Normalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, mean, scale, apply_tanh):
        out, params = _normalize_raw(grid.detach().contiguous(), None if mean is None else mean.detach(), scale, apply_tanh)
        ctx.save_for_backward(out, params)
        ctx.scale, ctx.apply_tanh, ctx.has_mean = bool(scale), bool(apply_tanh), mean is not None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        out, params = ctx.saved_tensors
        dev = out.device
        grad_in = torch.empty_like(out)
        want_mean = ctx.has_mean and ctx.needs_input_grad[1]
        grad_mean = torch.empty(1, dtype=torch.float64, device=dev) if want_mean else None
        call("gsr_psr_normalize_bwd", dev, grad_out.contiguous(), out, ctypes.c_longlong(out.numel()), params, ctx.scale,
             ctx.apply_tanh, grad_in, grad_mean, workspace=True, errors=_ERRORS)
        return (grad_in if ctx.needs_input_grad[0] else None), grad_mean, None, None


class _PSR2Mesh(torch.autograd.Function):
    """graphics_utils.PSR2Mesh with the Shape-as-Points rule dv/dphi = -n on per-vertex normals (the reference multiplies by
    per-face normals there, which only has a shape when V == F: INTEGRATION.md s17a)."""

    @staticmethod
    def forward(ctx, grid):
        g = grid.detach().contiguous()
        verts, faces, normals = _marching_cubes(g, tuple(g.shape), 0.0, True)
        v_unit = verts / _res_tensor(tuple(g.shape), g.device)
        ctx.save_for_backward(v_unit, normals)
        ctx.res = tuple(g.shape)
        ctx.mark_non_differentiable(faces)
        return v_unit, faces

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_v, _grad_faces):
        v_unit, n = ctx.saved_tensors
        vals = -((grad_v[:, 0] * n[:, 0] + grad_v[:, 1] * n[:, 1]) + grad_v[:, 2] * n[:, 2])
        return _rasterize_raw(v_unit, vals.unsqueeze(1).contiguous(), ctx.res, False, False)[0][0]


# ------------------------------------------------------------------------------------------------------ public stages
def point_rasterize(pts, vals, size, weighted=True, return_counts=False):
    """graphics_utils.point_rasterize for one cloud: pts [N,3] float32 in [0, 1), vals [N,C] float32 (C <= 4), size
    (R0, R1, R2) -> grid [C,R0,R1,R2] float32, periodic.  The index and weight arithmetic is the reference's fp32 chain; a
    node's terms are added in fp64 in a fixed order and rounded once.  weighted=True divides by the number of (point, corner)
    pairs on the node (zero-weight pairs of node-aligned coordinates included, 0 counted as 1); return_counts adds that
    number as int32 [R0,R1,R2].  ValueError for a coordinate that is not finite or outside [0, 1).  Differentiable towards
    pts and vals (a weight factor |p - pos| / cubesize differentiates to sign(p - pos) / cubesize, sign(0) = 0; the counts
    are constants)."""
    pts = _device_tensor("pts", pts, 3)
    if not torch.is_tensor(vals) or vals.dim() != 2 or not 1 <= vals.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"vals must have shape [N, C] with 1 <= C <= {MAX_CHANNELS}")
    vals = _device_tensor("vals", vals)
    if vals.shape[0] != pts.shape[0]:
        raise ValueError("vals must have one row per point")
    res = _res(size)
    on_rocm(pts=pts, vals=vals)
    if vals.device != pts.device:
        raise ValueError("pts and vals must be on the same device")
    if _wants_grad(pts, vals):
        grid, counts = _Rasterize.apply(pts, vals, res, bool(weighted), bool(return_counts))
    else:
        grid, counts = _rasterize_raw(pts.detach().contiguous(), vals.detach().contiguous(), res, weighted, return_counts)
    return (grid, counts) if return_counts else grid


def _interp(grid, pts, want_mean):
    res = _grid("grid", grid)
    pts = _device_tensor("pts", pts, 3)
    if pts.shape[0] < 1:
        raise ValueError("grid_interp needs at least one point")
    on_rocm(grid=grid, pts=pts)
    if grid.device != pts.device:
        raise ValueError("grid and pts must be on the same device")
    if _wants_grad(grid, pts):
        return _Interp.apply(grid, pts, bool(want_mean))
    return _interp_raw(grid.detach().contiguous(), res, pts.detach().contiguous(), want_mean)


def grid_interp(grid, pts, return_mean=False):
    """graphics_utils.grid_interp for one scalar grid: grid [R0,R1,R2] float32, pts [N,3] float32 in [0, 1) -> [N] float32,
    periodic trilinear samples (the 8 corner terms in the reference's order, added in fp64, rounded once).  return_mean adds
    the fixed-order fp64 mean of the samples (float64 [1], on the device).  Differentiable towards grid (the adjoint scatter)
    and pts, through the samples and through the mean."""
    out, mean = _interp(grid, pts, return_mean)
    return (out, mean) if return_mean else out


def _spectral_raw(spectrum, res, sig):
    dev = spectrum.device
    spec = torch.view_as_real(spectrum.contiguous())
    phi = torch.empty((res[0], res[1], res[2] // 2 + 1, 2), dtype=torch.float32, device=dev)
    call("gsr_psr_spectral", dev, spec, *res, ctypes.c_double(float(sig)), phi, errors=_ERRORS)
    return torch.view_as_complex(phi)


def spectral_solve(spectrum, size, sig):
    """The spectral Poisson solve of DPSR.forward: spectrum = rfftn of the rasterized normals [3,R0,R1,R2/2+1] complex64 ->
    Phi [R0,R1,R2/2+1] complex64 (Gaussian filter of width sig, divergence, inverse Laplacian, Phi[0,0,0] = 0).  Differentiable:
    grad_spectrum_d = conj(c_d) grad_Phi (PyTorch's convention for complex gradients), zero at element 0."""
    res = _res(size)
    if not torch.is_tensor(spectrum) or spectrum.dtype != torch.complex64:
        raise TypeError("spectrum must be a complex64 tensor")
    if tuple(spectrum.shape) != (3, res[0], res[1], res[2] // 2 + 1):
        raise ValueError(f"spectrum must have shape [3, {res[0]}, {res[1]}, {res[2] // 2 + 1}], got {list(spectrum.shape)}")
    on_rocm(spectrum=spectrum)
    if _wants_grad(spectrum):
        return _Spectral.apply(spectrum, res, float(sig))
    return _spectral_raw(spectrum.detach(), res, sig)


def normalize_grid(grid, mean=None, scale=True, apply_tanh=False):
    """The tail of DPSR.forward in one pass: grid - float32(mean) when mean (float64 [1] device tensor) is given, then with
    scale -v / |v[0,0,0]| * 0.5 (v[0,0,0] after the shift), then with apply_tanh tanh(v).  Returns a new tensor.
    Differentiable towards grid and mean; |v[0,0,0]| is a constant of the backward, as the reference detaches it."""
    _grid("grid", grid)
    on_rocm(grid=grid, mean=mean)
    dev = grid.device
    if mean is not None and (mean.dtype != torch.float64 or mean.numel() != 1 or mean.device != dev):
        raise ValueError("mean must be a float64 tensor with one element on the device of grid")
    if _wants_grad(grid, mean):
        return _Normalize.apply(grid, mean, bool(scale), bool(apply_tanh))
    return _normalize_raw(grid.detach().contiguous(), None if mean is None else mean.detach(), scale, apply_tanh)[0]


class DPSR:
    """graphics_utils.DPSR(res, sig, scale, shift, weighted): `dpsr(V, N) -> phi`.  V, N: [N,3] float32 (V in [0, 1)) -> phi
    [R0,R1,R2]; the reference's batched [1,N,3] -> [1,R0,R1,R2].  Batch size 1 only, N >= 1 (ValueError for an empty cloud,
    whatever the options).  `apply_tanh=True` folds the tanh that ShapeAsPoints.generate_mesh applies next into the
    normalisation pass.  Differentiable towards V and N whenever one of them requires grad (and grad mode is on); the result
    has no grad_fn otherwise."""

    def __init__(self, res, sig=10, scale=True, shift=True, weighted=False):
        self.res = _res(res)
        self.sig = float(sig)
        self.scale, self.shift, self.weighted = bool(scale), bool(shift), bool(weighted)

    def __call__(self, V, N, apply_tanh=False):
        if not torch.is_tensor(V) or not torch.is_tensor(N):
            raise TypeError("V and N must be torch tensors")
        if V.shape != N.shape:
            raise ValueError("V and N must have the same shape")
        batched = V.dim() == 3
        if batched:
            if V.shape[0] != 1:
                raise ValueError(f"DPSR runs one cloud per call (batch size 1), got a batch of {V.shape[0]}")
            V, N = V[0], N[0]
        V = _device_tensor("V", V, 3)
        N = _device_tensor("N", N, 3)
        if V.shape[0] < 1:
            raise ValueError("DPSR needs at least one point")       # no samples to shift by, and 0 / 0 in the scaling
        on_rocm(V=V, N=N)
        with torch.set_grad_enabled(_wants_grad(V, N)):
            ras = point_rasterize(V, N, self.res, weighted=self.weighted)
            spec = torch.fft.rfftn(ras, dim=(1, 2, 3))
            Phi = spectral_solve(spec, self.res, self.sig)
            phi = torch.fft.irfftn(Phi, s=self.res, dim=(0, 1, 2))
            if self.shift or self.scale or apply_tanh:
                mean = _interp(phi, V, True)[1] if self.shift else None
                phi = normalize_grid(phi, mean, scale=self.scale, apply_tanh=apply_tanh)
        return phi.unsqueeze(0) if batched else phi

    forward = __call__


def _marching_cubes(grid, res, level, want_normals):
    dev = grid.device
    nn = res[0] * res[1] * res[2]
    info = torch.empty(nn, dtype=torch.int32, device=dev)
    voff = torch.empty(nn + 1, dtype=torch.int32, device=dev)
    toff = torch.empty(nn + 1, dtype=torch.int32, device=dev)
    nv, nt = ctypes.c_int(0), ctypes.c_int(0)
    ws = Workspace(dev)                 # released when the mesh is returned
    normals = None
    with torch.cuda.device(dev):
        call("gsr_psr_mc_classify", dev, grid, *res, ctypes.c_float(level), info, voff, toff, ctypes.byref(nv), ctypes.byref(nt),
             workspace=ws, errors=_ERRORS)
        verts = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((nt.value, 3), dtype=torch.int32, device=dev)
        call("gsr_psr_mc_emit", dev, grid, *res, ctypes.c_float(level), info, voff, toff, verts, faces, errors=_ERRORS)
        if want_normals:
            normals = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
            if nv.value:
                call("gsr_psr_mc_normals", dev, grid, *res, ctypes.c_float(level), info, voff, normals, errors=_ERRORS)
    return verts, faces, normals


def marching_cubes(grid, level=0.0, return_normals=False):
    """Dense indexed marching cubes of grid [R0,R1,R2] float32 at `level` (not periodic): (verts [nv,3] float32 in index
    units, faces [nf,3] int32).  A corner is inside iff value < level, triangle normals point towards increasing value; one
    vertex per crossing edge, at i + (level - a) / (b - a) in fp32; vertices ordered by (lower node of the edge, axis),
    triangles by (cube, table order).  Watertight away from the grid boundary and deterministic by construction.
    return_normals adds unit vertex normals [nv,3] float32: the grid's gradient (central differences in index units, one-sided
    on the faces of the grid) at the two ends of the vertex's edge, interpolated with the vertex's t, normalised with
    eps 1e-6.  Not differentiable itself: psr2mesh is."""
    res = _grid("grid", grid)
    on_rocm(grid=grid)
    verts, faces, normals = _marching_cubes(grid.detach().contiguous(), res, level, return_normals)
    return (verts, faces, normals) if return_normals else (verts, faces)


def psr2mesh(grid):
    """graphics_utils.PSR2Mesh for one grid [R0,R1,R2] float32: (v_unit [nv,3] float32 = marching-cubes vertices at level 0 /
    (R0, R1, R2), faces [nf,3] int32, not differentiable).  Backward: the Shape-as-Points rule dv/dphi = -n with the unit
    vertex normals of marching_cubes, spread trilinearly: grad_grid = point_rasterize(v_unit, -<dL/dv, n>, res,
    weighted=False)."""
    _grid("grid", grid)
    on_rocm(grid=grid)
    if _wants_grad(grid):
        return _PSR2Mesh.apply(grid)
    verts, faces = marching_cubes(grid, 0.0)
    return verts / _res_tensor(tuple(grid.shape), grid.device), faces


class ShapeAsPoints:
    """gaustudio/models/sap.py ShapeAsPoints ('sap_pcd') for the path gs-extract-pcd takes, from_pointcloud -> generate_mesh,
    and as the optimisable cloud the reference registers: requires_grad_() makes the logit-space `xyz` and the `normals` leaf
    parameters, parameters() hands them to an optimiser, and generate_mesh() then returns vertices that carry gradients back
    through transform, psr2mesh, DPSR and the sigmoid."""

    default_conf = dict(dpsr_res=256, dpsr_sig=2, dpsr_scale=True, dpsr_shift=True, dpsr_weighted=False)

    def __init__(self, **conf):
        unknown = set(conf) - set(self.default_conf)
        if unknown:
            raise TypeError(f"unknown ShapeAsPoints option(s): {sorted(unknown)}")
        self.config = dict(self.default_conf, **conf)
        r = int(self.config["dpsr_res"])
        self.dpsr = DPSR((r, r, r), sig=self.config["dpsr_sig"], scale=self.config["dpsr_scale"],
                         shift=self.config["dpsr_shift"], weighted=self.config["dpsr_weighted"])
        self.xyz = self.normals = self.center = self.scale = None

    @staticmethod
    def transform(verts, center, scale, inverse=False):
        """models/sap.py:35-42."""
        if inverse:
            out = verts * 2. - 1.
            return out * scale + center
        out = (verts - center) / scale
        return (out + 1.) / 2.

    @classmethod
    def from_pointcloud(cls, points, normals, **conf):
        """from_o3d_pointcloud (models/sap.py:130-163) on device tensors: center = mean, scale = max|p - center| * 1.2, the
        unit-cube coordinates stored as logit(p) like the reference does (generate_mesh applies sigmoid again: the round trip
        moves the last bit of a coordinate, and is kept)."""
        points = _device_tensor("points", points, 3)
        normals = _device_tensor("normals", normals, 3)
        if normals.shape[0] != points.shape[0]:
            raise ValueError("normals must have one row per point")
        if points.shape[0] < 1:
            raise ValueError("ShapeAsPoints needs at least one point")
        on_rocm(points=points, normals=normals)
        if normals.device != points.device:
            raise ValueError("points and normals must be on the same device")
        self = cls(**conf)
        with torch.no_grad():
            points = points.detach()
            self.center = points.mean(dim=0)
            self.scale = (points - self.center).abs().max() * 1.2
            unit = self.transform(points, self.center, self.scale)
            self.xyz = torch.log(unit / (1 - unit))
            self.normals = normals.detach().contiguous()
        return self

    def requires_grad_(self, flag=True):
        """Make `xyz` (logit space) and `normals` leaf tensors that require grad (or stop them).  Returns self."""
        if self.xyz is None:
            raise RuntimeError("ShapeAsPoints holds no points: build it with from_pointcloud")
        self.xyz = self.xyz.detach().requires_grad_(bool(flag))
        self.normals = self.normals.detach().requires_grad_(bool(flag))
        return self

    def parameters(self):
        """[xyz, normals]: what an optimiser steps."""
        if self.xyz is None:
            raise RuntimeError("ShapeAsPoints holds no points: build it with from_pointcloud")
        return [self.xyz, self.normals]

    def psr_grid(self):
        """tanh(DPSR(sigmoid(xyz), normals)) [R,R,R]: the indicator grid generate_mesh runs marching cubes on; carries
        gradients when the cloud requires grad."""
        if self.xyz is None:
            raise RuntimeError("ShapeAsPoints holds no points: build it with from_pointcloud")
        return self.dpsr(torch.sigmoid(self.xyz), self.normals, apply_tanh=True)

    def generate_mesh(self):
        """-> (vertices [nv,3] float32 world units, faces [nf,3] int32, v_unit [nv,3] = index-unit vertices / R)."""
        if self.xyz is None:
            raise RuntimeError("ShapeAsPoints holds no points: build it with from_pointcloud")
        if _wants_grad(self.xyz, self.normals):
            v_unit, faces = psr2mesh(self.psr_grid())
            return self.transform(v_unit, self.center, self.scale, True), faces, v_unit
        with torch.no_grad():
            pts = torch.sigmoid(self.xyz)
            grid = self.dpsr(pts, self.normals, apply_tanh=True)
            verts, faces = marching_cubes(grid, 0.0)
            v_unit = verts / grid.shape[-1]
            vertices = self.transform(v_unit, self.center, self.scale, True)
        return vertices, faces, v_unit


def mesh_sap(points, normals, **conf):
    """extract_pcd.py mesh_sap on the device: (vertices float32 [nv,3], faces int32 [nf,3]) of the cleaned cloud, ready for
    mesh_clean.remove_small_components, mesh_raster and formats.write_ply_mesh.  conf: dpsr_res (256), dpsr_sig (2),
    dpsr_scale, dpsr_shift, dpsr_weighted."""
    vertices, faces, _ = ShapeAsPoints.from_pointcloud(points, normals, **conf).generate_mesh()
    return vertices, faces
