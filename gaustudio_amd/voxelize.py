"""Mesh voxelization on the GPU (csrc/gsr_voxel.hip): what the reference's `VoxelInitializer`
(gaustudio/pipelines/initializers/mesh.py:252-442) does to turn a triangle mesh into Gaussian seeds -- normalise the mesh to
the unit cube, voxelize it, put one Gaussian at the centre of every voxel the surface touches.

    grid = voxelize_mesh(vertices, faces, voxel_size, min_bound, max_bound)      # Open3D's create_from_triangle_mesh_within_bounds
    near = closest_on_mesh(grid, vertices, faces, vertex_colors)                   # closest triangle, barycentric weights, colour
    vn, scale, center = normalize_mesh(vertices)                                   # _normalize_mesh, mesh.py:327-352
    cloud = voxel_seeds(vertices, faces, vertex_colors, voxel_size=1 / 256)        # build_model -> formats.GaussianCloud
    grid, cloud = voxel_init(vertices, faces, vertex_colors)

Everything geometric is float64 on the device, operation for operation that of tests/mesh_voxel_model.py: the set of occupied
voxels does not depend on a float32 rounding.  Contract and the reference's quirks (the +inf raw opacity, its dead colour call,
the two voxel-centre formulas, the 1024 limit): INTEGRATION.md s20.  `MeshInitializer` (one Gaussian per triangle) is not
covered.  ROCm tensors only, no CPU fallback; every call runs on the current stream of the tensors' device.
"""
import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from ._abi import Workspace, call, check_mesh, on_rocm, same_device
from .formats import GaussianCloud

MAX_RES = 1024                      # GSR_VOXEL_MAX_RES
C0 = 0.28209479177387814            # gaustudio/utils/sh_utils.py
UNIT_MIN, UNIT_MAX = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)


@dataclass
class VoxelGrid:
    grid_index: torch.Tensor        # int32 [nvox,3], in ascending linear index (i0 n1 + i1) n2 + i2 (Open3D's loop order)
    voxel_index: torch.Tensor       # int32 [nvox], that linear index
    pair_start: torch.Tensor        # int32 [nvox+1]: voxel q overlaps the triangles pair_tri[pair_start[q]:pair_start[q+1]]
    pair_tri: torch.Tensor          # int32 [npairs], ascending within a voxel
    shape: Tuple[int, int, int]
    voxel_size: float
    origin: Tuple[float, float, float]           # min_bound
    occupancy: Optional[torch.Tensor] = None     # int32 [ceil(n0 n1 n2 / 32)]: bit t & 31 of word t >> 5

    @property
    def num_voxels(self):
        return int(self.voxel_index.shape[0])

    def centers(self):
        """float64 [nvox,3]: ((i + 0.5) voxel_size) + origin, Open3D's get_voxel_center_coordinate.  (The overlap test is run
        around (origin + voxel_size / 2) + i voxel_size; the two coincide when voxel_size is a power of two.)"""
        org = torch.tensor(self.origin, dtype=torch.float64, device=self.grid_index.device)
        return (self.grid_index.to(torch.float64) + 0.5) * float(self.voxel_size) + org


# ------------------------------------------------------------------------------------------------------ argument checks
def _mesh(vertices, faces, vertex_colors=None, vertex_dtypes=(torch.float32, torch.float64)):
    """Shapes and dtypes first, then devices, so that those errors need no GPU.  Returns the device."""
    if not torch.is_tensor(vertices) or not torch.is_tensor(faces):
        raise TypeError("vertices and faces must be torch tensors")
    limit = "the mesh must have fewer than 2^28 vertices and faces"
    check_mesh(vertices, faces, vertex_colors, vertex_dtypes=vertex_dtypes, max_verts=(2 ** 28, limit), max_faces=(2 ** 28, limit),
               device_exc=ValueError)
    same_device(vertices.device, ref="vertices", faces=faces, vertex_colors=vertex_colors)
    return vertices.device


def _bounds(voxel_size, min_bound, max_bound):
    try:
        vs = float(voxel_size)
        lo, hi = tuple(float(v) for v in min_bound), tuple(float(v) for v in max_bound)
    except TypeError:
        raise TypeError("voxel_size must be a number, min_bound and max_bound sequences of three numbers") from None
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("min_bound and max_bound must have three entries")
    if not (vs > 0 and math.isfinite(vs)):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
    if not all(math.isfinite(v) for v in lo + hi):
        raise ValueError("min_bound and max_bound must be finite")
    ext = [(b - a) / vs for a, b in zip(lo, hi)]
    if not all(e < 2 ** 31 for e in ext):
        raise ValueError(f"the grid must have between 2 and {MAX_RES} voxels along every axis")
    shape = tuple(int(math.floor(e + 0.5)) for e in ext)          # std::round
    if min(shape) < 2 or max(shape) > MAX_RES:
        raise ValueError(f"the grid must have between 2 and {MAX_RES} voxels along every axis, got {shape} "
                         f"(voxel_size {vs}, bounds {lo} .. {hi})")
    return vs, lo, hi, shape


def _grid_args(vs, lo, shape):
    """The arguments every gsr_voxel_* entry shares: voxel size, min bound, n0, n1, n2."""
    return (ctypes.c_double(vs), (ctypes.c_double * 3)(*lo), *shape)


# ------------------------------------------------------------------------------------------------------ voxelization
def _empty_grid(vs, lo, shape, dev, occupancy):
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    nn = shape[0] * shape[1] * shape[2]
    return VoxelGrid(z(0, 3), z(0), z(1), z(0), shape, vs, lo, z((nn + 31) // 32) if occupancy else None)


def voxelize_stages(vertices, faces, voxel_size, min_bound, max_bound, return_occupancy=False, on_stage=None):
    """voxelize_mesh with a hook: on_stage(name) is called on the host right before each stage is enqueued ('plan', 'count',
    'emit', 'sort') and after the last one ('done'); events recorded there bracket the stages, each with the read-back that
    ends it (tools/mesh_voxel_timing.py)."""
    vs, lo, hi, shape = _bounds(voxel_size, min_bound, max_bound)
    dev = _mesh(vertices, faces)
    mark = on_stage if on_stage is not None else (lambda name: None)
    v = vertices.detach().to(torch.float64).contiguous()
    f = faces.detach().to(torch.int32).contiguous()
    nv, nf = v.shape[0], f.shape[0]
    if nf == 0:
        return _empty_grid(vs, lo, shape, dev, return_occupancy)
    if nv == 0:
        raise ValueError("voxelize_mesh: faces given without vertices")
    grid = _grid_args(vs, lo, shape)
    ws = Workspace(dev)                 # one for all stages, released when the grid is returned
    run = lambda name, *args, workspace=False, error="bad argument": call(
        name, dev, *args, workspace=workspace, what="voxelize_mesh", errors={-2: "{what}: " + error})
    ints = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        mark("plan")
        tri_box, col_start = ints(nf * 6), ints(nf + 1)
        num_items = ctypes.c_int(0)
        run("gsr_voxel_plan", v, nv, f, nf, *grid, tri_box, col_start, ctypes.byref(num_items), workspace=ws,
            error="a face index lies outside [0, V), a vertex coordinate is not finite, or the mesh covers more than 2^30 voxel columns")
        mark("count")
        item_start = ints(num_items.value + 1)
        num_pairs = ctypes.c_int(0)
        run("gsr_voxel_count", v, f, nf, *grid, tri_box, col_start, num_items, item_start, ctypes.byref(num_pairs), workspace=ws,
            error="more than 2^30 (voxel, triangle) pairs")
        npairs = num_pairs.value
        if npairs == 0:
            mark("done")
            return _empty_grid(vs, lo, shape, dev, return_occupancy)
        mark("emit")
        pair_voxel, pair_tri_in = ints(npairs), ints(npairs)
        run("gsr_voxel_emit", v, f, nf, *grid, tri_box, col_start, num_items, item_start, pair_voxel, pair_tri_in)
        mark("sort")
        voxel_index, pair_start, pair_tri = ints(npairs), ints(npairs + 1), ints(npairs)
        grid_index = torch.empty((npairs, 3), dtype=torch.int32, device=dev)
        nn = shape[0] * shape[1] * shape[2]
        occ = ints((nn + 31) // 32) if return_occupancy else None
        num_voxels = ctypes.c_int(0)
        run("gsr_voxel_sort", pair_voxel, pair_tri_in, num_pairs, *shape, voxel_index, pair_start, pair_tri, grid_index, occ,
            ctypes.byref(num_voxels), workspace=ws)
        mark("done")
    nvox = num_voxels.value
    return VoxelGrid(grid_index[:nvox].clone(), voxel_index[:nvox].clone(), pair_start[:nvox + 1].clone(), pair_tri, shape, vs, lo, occ)


def voxelize_mesh(vertices, faces, voxel_size, min_bound=UNIT_MIN, max_bound=UNIT_MAX, return_occupancy=False):
    """VoxelGrid.create_from_triangle_mesh_within_bounds: the voxels of the grid n_d = round((max_bound_d - min_bound_d) /
    voxel_size) (2 <= n_d <= 1024) that overlap a triangle, by the float64 triangle / box separating-axis test; touching
    counts.  vertices [V,3] float32 or float64 (used as float64, NOT normalised), faces [F,3] int32 / int64, on a ROCm
    device.  ValueError for a face index out of range or a coordinate that is not finite.  A mesh that touches no voxel
    (F = 0 included) gives an empty VoxelGrid."""
    return voxelize_stages(vertices, faces, voxel_size, min_bound, max_bound, return_occupancy)


def closest_on_mesh(grid, vertices, faces, vertex_colors=None):
    """Per occupied voxel of `grid` the closest triangle to its centre among the triangles listed in the 27 voxels around it
    (which hold the closest point of the whole mesh: the voxel's own triangle is within 0.866 voxel_size):
    dict(closest_tri int32 [nvox] (-1: no triangle with a finite distance), closest_uvw float64 [nvox,3] barycentric weights
    (1 - v - w, v, w), color float32 [nvox,3] = the vertex colours interpolated with them -- only with vertex_colors [V,3]
    float32).  Exact distance ties go to the lower triangle index.  vertices / faces: the mesh `grid` was made from."""
    if not isinstance(grid, VoxelGrid):
        raise TypeError(f"grid must be a VoxelGrid, got {type(grid).__name__}")
    dev = _mesh(vertices, faces, vertex_colors)
    same_device(dev, ref="vertices", grid=grid.voxel_index)
    v = vertices.detach().to(torch.float64).contiguous()
    f = faces.detach().to(torch.int32).contiguous()
    col = None if vertex_colors is None else vertex_colors.detach().contiguous()
    nvox = grid.num_voxels
    tri = torch.empty(nvox, dtype=torch.int32, device=dev)
    uvw = torch.empty((nvox, 3), dtype=torch.float64, device=dev)
    color = None if col is None else torch.empty((nvox, 3), dtype=torch.float32, device=dev)
    call("gsr_voxel_closest", dev, v, v.shape[0], f, f.shape[0], col, *_grid_args(grid.voxel_size, grid.origin, grid.shape),
         grid.voxel_index, grid.pair_start, grid.pair_tri, nvox, tri, uvw, color, what="closest_on_mesh",
         errors={-2: "{what}: bad argument"})
    out = dict(closest_tri=tri, closest_uvw=uvw)
    if color is not None:
        out["color"] = color
    return out


# ------------------------------------------------------------------------------------------------------ the initializer
def normalize_mesh(vertices):
    """_normalize_mesh (mesh.py:327-352) in float64 from float32 vertices: (vn float64 [V,3] on the device, scale, center
    float64 numpy [3]); vn = clip((v - center) / scale, -0.5 + 1e-6, 0.5 - 1e-6).  ValueError for a mesh without extent."""
    if not torch.is_tensor(vertices):
        raise TypeError("vertices must be a torch tensor")
    if vertices.dtype != torch.float32:
        raise TypeError(f"vertices must be float32, got {vertices.dtype}")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.shape[0] < 1:
        raise ValueError(f"vertices must have shape [V, 3] with V >= 1, got {list(vertices.shape)}")
    on_rocm(ValueError, vertices=vertices)
    v = vertices.detach().to(torch.float64)
    lo, hi = v.min(dim=0).values, v.max(dim=0).values
    center = (lo + hi) / 2
    scale = (hi - lo).max()                 # a device tensor: a true division below, not a multiplication by 1 / scale
    s = float(scale)
    if not math.isfinite(s):
        raise ValueError("a vertex coordinate is not finite")
    if not s > 0:
        raise ValueError("the mesh has no extent (scale == 0)")
    vn = torch.clamp((v - center) / scale, -0.5 + 1e-6, 0.5 - 1e-6)
    return vn, s, center.cpu().numpy()


def _seed_options(sh_degree, colors, rotations, opacity):
    if isinstance(sh_degree, bool) or int(sh_degree) != sh_degree or not 0 <= sh_degree <= 3:
        raise ValueError(f"sh_degree must be 0..3, got {sh_degree}")
    if colors not in ("closest", "gray"):
        raise ValueError(f"colors must be 'closest' or 'gray', got {colors!r}")
    if rotations not in ("random", "identity"):
        raise ValueError(f"rotations must be 'random' or 'identity', got {rotations!r}")
    if not 0.0 < float(opacity) <= 1.0:
        raise ValueError(f"opacity must lie in (0, 1], got {opacity}")


def voxel_init(vertices, faces, vertex_colors=None, voxel_size=1 / 256, sh_degree=3, colors="closest", rotations="random",
               generator=None, opacity=1.0):
    """VoxelInitializer.build_model (mesh.py:288-325) into VanillaPointCloud.create_from_attribute (models/vanilla_sg.py:69-97):
    (grid over the normalised mesh, formats.GaussianCloud with one Gaussian per occupied voxel, in the grid's order).

      xyz      float32(centre * scale + center), float64 before the cast
      scale    log(float32(voxel_size * scale * 0.8) + 1e-7) in float32, three times (raw: the renderer applies exp)
      opacity  inverse_sigmoid(opacity) raw; the reference's 1.0 gives +inf, whose sigmoid is 1
      rot      normalised torch.randn(P, 4, generator=generator) ('random', the reference) or (1, 0, 0, 0) ('identity')
      f_dc     RGB2SH(rgb) = (rgb - 0.5) / C0 in float32; rgb = ones without vertex_colors (create_from_attribute's default),
               with them the colour of the closest point of the mesh ('closest') or 0.5 ('gray': what the reference's colour
               loop yields in effect, its closest-point call raising for every point)
      f_rest   0 for sh_degree (0..3)

    vertices [V,3] float32, faces [F,3] int32 / int64, vertex_colors [V,3] float32 or None, on a ROCm device.
    ValueError("No voxels generated from mesh") for an empty result, as the reference."""
    _seed_options(sh_degree, colors, rotations, opacity)
    _bounds(voxel_size, UNIT_MIN, UNIT_MAX)
    if generator is not None and not isinstance(generator, torch.Generator):
        raise TypeError("generator must be a torch.Generator or None")
    dev = _mesh(vertices, faces, vertex_colors, vertex_dtypes=(torch.float32,))
    if vertices.shape[0] < 1:
        raise ValueError("No voxels generated from mesh")
    vn, scale, center = normalize_mesh(vertices)
    grid = voxelize_mesh(vn, faces, voxel_size, UNIT_MIN, UNIT_MAX)
    P = grid.num_voxels
    if P == 0:
        raise ValueError("No voxels generated from mesh")
    xyz = (grid.centers() * scale + torch.from_numpy(center).to(dev)).to(torch.float32)
    full = lambda shape, value: torch.full(shape, float(value), dtype=torch.float32, device=dev)
    raw_scale = np.log(np.float32(float(voxel_size) * scale * 0.8) + np.float32(1e-7))
    with np.errstate(divide="ignore"):
        raw_opacity = np.float32(np.log(np.float64(opacity) / (1.0 - np.float64(opacity))))
    if vertex_colors is None:
        rgb = full((P, 3), 1.0)
    elif colors == "gray":
        rgb = full((P, 3), 0.5)
    else:
        rgb = closest_on_mesh(grid, vn, faces, vertex_colors)["color"]
    # RGB2SH in float32, one rounding per operation: the float64 quotient of two float32 values, rounded, is the correctly
    # rounded float32 quotient, and dividing by a device tensor keeps torch from multiplying by a reciprocal
    c0 = torch.tensor(float(np.float32(C0)), dtype=torch.float64, device=dev)
    f_dc = ((rgb - 0.5).to(torch.float64) / c0).to(torch.float32).reshape(P, 1, 3)
    if rotations == "random":
        rot = torch.nn.functional.normalize(torch.randn((P, 4), dtype=torch.float32, device=dev, generator=generator), dim=-1)
    else:
        rot = full((P, 4), 0.0)
        rot[:, 0] = 1
    cloud = GaussianCloud(xyz=xyz.contiguous(), f_dc=f_dc.contiguous(), f_rest=full((P, (int(sh_degree) + 1) ** 2 - 1, 3), 0.0),
                          opacity=full((P, 1), raw_opacity), scale=full((P, 3), raw_scale), rot=rot)
    return grid, cloud


def voxel_seeds(vertices, faces, vertex_colors=None, voxel_size=1 / 256, sh_degree=3, colors="closest", rotations="random",
                generator=None, opacity=1.0):
    """The GaussianCloud of voxel_init (see there); feeds formats.export_gaussian_ply unchanged."""
    return voxel_init(vertices, faces, vertex_colors, voxel_size, sh_degree, colors, rotations, generator, opacity)[1]
