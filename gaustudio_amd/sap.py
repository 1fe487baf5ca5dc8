"""Shape-as-Points meshing on the GPU (csrc/gsr_psr.hip): what gs-extract-pcd --meshing sap runs on the cleaned cloud,
`mesh_sap` -> `ShapeAsPoints.from_o3d_pointcloud(pcd).to_o3d_mesh()` (gaustudio/models/sap.py), i.e. the Poisson solver `DPSR`
of gaustudio/utils/graphics_utils.py:19-333 and a marching cubes over its grid (the reference goes through skimage on the CPU).

    grid = point_rasterize(pts, vals, (R0, R1, R2), weighted=True)       # graphics_utils.point_rasterize
    fv = grid_interp(grid, pts)                                            # graphics_utils.grid_interp
    phi = DPSR((R0, R1, R2), sig=2)(V, N)                                  # rasterize -> rfftn -> spectral solve -> irfftn -> normalise
    verts, faces = marching_cubes(phi, level=0.0)                          # index units
    vertices, faces = mesh_sap(points, normals, dpsr_res=256)              # the whole stage, world units

FORWARD ONLY: this is an extraction stage, which the reference runs outside any optimisation loop.  No returned tensor carries
a grad_fn; gradients (the "differentiable" half of DPSR) are out of scope.  The two FFTs are torch.fft (hipFFT); everything
between and around them is hand-written HIP.  Deterministic: no float atomics, bit-identical from run to run.

Contract and quirks: INTEGRATION.md s17.  ROCm tensors only, no CPU fallback; every call runs on the current stream of the
tensors' device.
"""
import ctypes

import torch

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


def point_rasterize(pts, vals, size, weighted=True, return_counts=False):
    """graphics_utils.point_rasterize for one cloud: pts [N,3] float32 in [0, 1), vals [N,C] float32 (C <= 4), size
    (R0, R1, R2) -> grid [C,R0,R1,R2] float32, periodic.  The index and weight arithmetic is the reference's fp32 chain; a
    node's terms are added in fp64 in a fixed order and rounded once.  weighted=True divides by the number of (point, corner)
    pairs on the node (zero-weight pairs of node-aligned coordinates included, 0 counted as 1); return_counts adds that
    number as int32 [R0,R1,R2].  ValueError for a coordinate that is not finite or outside [0, 1).  Forward only."""
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
    dev = pts.device
    pts, vals = pts.detach().contiguous(), vals.detach().contiguous()
    n, C = pts.shape[0], vals.shape[1]
    grid = torch.empty((C,) + res, dtype=torch.float32, device=dev)
    counts = torch.empty(res, dtype=torch.int32, device=dev) if return_counts else None
    call("gsr_psr_rasterize", dev, pts, n, vals, C, *res, bool(weighted), grid, counts, workspace=True,
         errors=_point_errors("point_rasterize"))
    return (grid, counts) if return_counts else grid


def _interp(grid, pts, want_mean):
    res = _grid("grid", grid)
    pts = _device_tensor("pts", pts, 3)
    if pts.shape[0] < 1:
        raise ValueError("grid_interp needs at least one point")
    on_rocm(grid=grid, pts=pts)
    if grid.device != pts.device:
        raise ValueError("grid and pts must be on the same device")
    dev = pts.device
    grid, pts = grid.detach().contiguous(), pts.detach().contiguous()
    out = torch.empty(pts.shape[0], dtype=torch.float32, device=dev)
    mean = torch.empty(1, dtype=torch.float64, device=dev) if want_mean else None
    call("gsr_psr_interp", dev, grid, *res, pts, pts.shape[0], out, mean, workspace=True, errors=_point_errors("grid_interp"))
    return out, mean


def grid_interp(grid, pts, return_mean=False):
    """graphics_utils.grid_interp for one scalar grid: grid [R0,R1,R2] float32, pts [N,3] float32 in [0, 1) -> [N] float32,
    periodic trilinear samples (the 8 corner terms in the reference's order, added in fp64, rounded once).  return_mean adds
    the fixed-order fp64 mean of the samples (float64 [1], on the device).  Forward only."""
    out, mean = _interp(grid, pts, return_mean)
    return (out, mean) if return_mean else out


def spectral_solve(spectrum, size, sig):
    """The spectral Poisson solve of DPSR.forward: spectrum = rfftn of the rasterized normals [3,R0,R1,R2/2+1] complex64 ->
    Phi [R0,R1,R2/2+1] complex64 (Gaussian filter of width sig, divergence, inverse Laplacian, Phi[0,0,0] = 0).  Forward only."""
    res = _res(size)
    if not torch.is_tensor(spectrum) or spectrum.dtype != torch.complex64:
        raise TypeError("spectrum must be a complex64 tensor")
    if tuple(spectrum.shape) != (3, res[0], res[1], res[2] // 2 + 1):
        raise ValueError(f"spectrum must have shape [3, {res[0]}, {res[1]}, {res[2] // 2 + 1}], got {list(spectrum.shape)}")
    on_rocm(spectrum=spectrum)
    dev = spectrum.device
    spec = torch.view_as_real(spectrum.detach().contiguous())
    phi = torch.empty((res[0], res[1], res[2] // 2 + 1, 2), dtype=torch.float32, device=dev)
    call("gsr_psr_spectral", dev, spec, *res, ctypes.c_double(float(sig)), phi, errors=_ERRORS)
    return torch.view_as_complex(phi)


def normalize_grid(grid, mean=None, scale=True, apply_tanh=False):
    """The tail of DPSR.forward in one pass: grid - float32(mean) when mean (float64 [1] device tensor) is given, then with
    scale -v / |v[0,0,0]| * 0.5 (v[0,0,0] after the shift), then with apply_tanh tanh(v).  Returns a new tensor."""
    _grid("grid", grid)
    on_rocm(grid=grid, mean=mean)
    dev = grid.device
    if mean is not None and (mean.dtype != torch.float64 or mean.numel() != 1 or mean.device != dev):
        raise ValueError("mean must be a float64 tensor with one element on the device of grid")
    grid = grid.detach().contiguous()
    out = torch.empty_like(grid)
    params = torch.empty(2, dtype=torch.float32, device=dev)
    call("gsr_psr_normalize", dev, grid, out, ctypes.c_longlong(grid.numel()), mean, bool(scale), bool(apply_tanh), params,
         errors=_ERRORS)
    return out


class DPSR:
    """graphics_utils.DPSR(res, sig, scale, shift, weighted), forward only: `dpsr(V, N) -> phi`.  V, N: [N,3] float32 (V in
    [0, 1)) -> phi [R0,R1,R2]; the reference's batched [1,N,3] -> [1,R0,R1,R2].  Batch size 1 only, N >= 1 (ValueError for an
    empty cloud, whatever the options).  `apply_tanh=True` folds
    the tanh that ShapeAsPoints.generate_mesh applies next into the normalisation pass.  The result has no grad_fn: gradients
    are out of scope."""

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
        with torch.no_grad():
            ras = point_rasterize(V, N, self.res, weighted=self.weighted)
            spec = torch.fft.rfftn(ras, dim=(1, 2, 3))
            Phi = spectral_solve(spec, self.res, self.sig)
            phi = torch.fft.irfftn(Phi, s=self.res, dim=(0, 1, 2))
            if self.shift or self.scale or apply_tanh:
                mean = _interp(phi, V, True)[1] if self.shift else None
                phi = normalize_grid(phi, mean, scale=self.scale, apply_tanh=apply_tanh)
        return phi.unsqueeze(0) if batched else phi

    forward = __call__


def marching_cubes(grid, level=0.0):
    """Dense indexed marching cubes of grid [R0,R1,R2] float32 at `level` (not periodic): (verts [nv,3] float32 in index
    units, faces [nf,3] int32).  A corner is inside iff value < level, triangle normals point towards increasing value; one
    vertex per crossing edge, at i + (level - a) / (b - a) in fp32; vertices ordered by (lower node of the edge, axis),
    triangles by (cube, table order).  Watertight away from the grid boundary and deterministic by construction."""
    res = _grid("grid", grid)
    on_rocm(grid=grid)
    dev = grid.device
    grid = grid.detach().contiguous()
    nn = res[0] * res[1] * res[2]
    info = torch.empty(nn, dtype=torch.int32, device=dev)
    voff = torch.empty(nn + 1, dtype=torch.int32, device=dev)
    toff = torch.empty(nn + 1, dtype=torch.int32, device=dev)
    nv, nt = ctypes.c_int(0), ctypes.c_int(0)
    ws = Workspace(dev)                 # released when the mesh is returned
    with torch.cuda.device(dev):
        call("gsr_psr_mc_classify", dev, grid, *res, ctypes.c_float(level), info, voff, toff, ctypes.byref(nv), ctypes.byref(nt),
             workspace=ws, errors=_ERRORS)
        verts = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((nt.value, 3), dtype=torch.int32, device=dev)
        call("gsr_psr_mc_emit", dev, grid, *res, ctypes.c_float(level), info, voff, toff, verts, faces, errors=_ERRORS)
    return verts, faces


class ShapeAsPoints:
    """gaustudio/models/sap.py ShapeAsPoints ('sap_pcd') for the path gs-extract-pcd takes: from_pointcloud -> generate_mesh.
    Forward only (no grad_fn on any result; gradients are out of scope)."""

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

    def generate_mesh(self):
        """-> (vertices [nv,3] float32 world units, faces [nf,3] int32, v_unit [nv,3] = index-unit vertices / R)."""
        if self.xyz is None:
            raise RuntimeError("ShapeAsPoints holds no points: build it with from_pointcloud")
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
