"""Per-triangle Gaussian seeds on the GPU (csrc/gsr_mesh_bake.hip gsr_mesh_seeds): the reference's `MeshInitializer`
(gaustudio/pipelines/initializers/mesh.py:74-250, the base class of its `tsdf` initializer) -- n flat Gaussians per triangle
at fixed barycentric positions, the rotation taken from the interpolated vertex normal, two scale axes from the shortest edge.

    cloud = mesh_seeds(vertices, faces, vertex_colors=None, vertex_normals=None, n_per_triangle=1)     # formats.GaussianCloud

Gaussian f * n + k is the k-th of face f.  Contract and the reference's quirks (the +inf raw opacity, the zero third scale axis
whose raw value is log(1e-7), the sign() cases of normal2rotation, the quaternion that is not normalised, torch.cross along the
last axis): INTEGRATION.md s21.  vertex_colors typically come from texture_bake.  ROCm tensors only, no CPU fallback.
"""
import torch

from ._abi import call, on_rocm, same_device
from .formats import GaussianCloud
from .mesh_raster import MeshRasterizer
from .voxelize import _mesh

N_PER_TRIANGLE = (1, 3, 4, 6)


def mesh_seeds(vertices, faces, vertex_colors=None, vertex_normals=None, n_per_triangle=1, sh_degree=3):
    """MeshInitializer.build_model into VanillaPointCloud.create_from_attribute: a formats.GaussianCloud of
    F * n_per_triangle Gaussians.

      xyz      the barycentric sum (b0 v0 + b1 v1) + b2 v2 of mesh.py:98-137's table for n_per_triangle (1, 3, 4 or 6)
      f_dc     RGB2SH of the same sum of vertex_colors; of rgb = 1 without them (create_from_attribute's default)
      scale    raw (log(2 s + 1e-7), same, log(1e-7)), s = shortest edge * surface_triangle_circle_radius
      opacity  raw +inf: inverse_sigmoid(1), whose sigmoid is 1
      rot      rotmat2quaternion(normal2rotation(N)), N the same sum of the vertex normals, normalised; (w, x, y, z), raw
      f_rest   0 for sh_degree (0..3)

    vertices [V,3] float32, faces [F,3] int32 / int64, vertex_colors / vertex_normals [V,3] float32 or None, on a ROCm device.
    Without vertex_normals, MeshRasterizer.vertex_normals() are used (area-weighted like Open3D's compute_vertex_normals, which
    the reference calls; agreement unpinned).  ValueError for a face index outside [0, V)."""
    if isinstance(n_per_triangle, bool) or n_per_triangle not in N_PER_TRIANGLE:
        raise ValueError(f"n_per_triangle must be one of {N_PER_TRIANGLE}, got {n_per_triangle!r}")
    if isinstance(sh_degree, bool) or int(sh_degree) != sh_degree or not 0 <= sh_degree <= 3:
        raise ValueError(f"sh_degree must be 0..3, got {sh_degree}")
    if vertex_normals is not None:
        if not torch.is_tensor(vertex_normals):
            raise TypeError("vertex_normals must be a torch tensor or None")
        if vertex_normals.dtype != torch.float32:
            raise TypeError(f"vertex_normals must be float32, got {vertex_normals.dtype}")
        if torch.is_tensor(vertices) and tuple(vertex_normals.shape) != tuple(vertices.shape):
            raise ValueError(f"vertex_normals must have shape {list(vertices.shape)} like vertices, got {list(vertex_normals.shape)}")
    dev = _mesh(vertices, faces, vertex_colors, vertex_dtypes=(torch.float32,))
    on_rocm(ValueError, vertex_normals=vertex_normals)
    same_device(dev, ref="vertices", vertex_normals=vertex_normals)
    n = int(n_per_triangle)
    v = vertices.detach().contiguous()
    f = faces.detach().to(torch.int32).contiguous()
    V, F = v.shape[0], f.shape[0]
    P = F * n
    if P >= 2 ** 31:
        raise ValueError("the mesh gives 2^31 Gaussians or more")
    if F > 0 and V == 0:
        raise ValueError("mesh_seeds: faces given without vertices")
    col = None if vertex_colors is None else vertex_colors.detach().contiguous()
    if P == 0:
        nrm = None
    elif vertex_normals is None:
        nrm = MeshRasterizer(v, f).vertex_normals()          # ValueError for a face index out of range
    else:
        nrm = vertex_normals.detach().contiguous()
    new = lambda c: torch.empty((P, c), dtype=torch.float32, device=dev)
    xyz, f_dc, scale, rot = new(3), new(3), new(3), new(4)
    call("gsr_mesh_seeds", dev, v, nrm, col, V, f, F, n, xyz, f_dc, scale, rot, workspace=True,
         errors={-2: "mesh_seeds: a face index lies outside [0, V)"})
    return GaussianCloud(xyz=xyz, f_dc=f_dc.reshape(P, 1, 3),
                         f_rest=torch.zeros((P, (int(sh_degree) + 1) ** 2 - 1, 3), dtype=torch.float32, device=dev),
                         opacity=torch.full((P, 1), float("inf"), dtype=torch.float32, device=dev), scale=scale, rot=rot)
