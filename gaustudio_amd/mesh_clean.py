"""Mesh cleaning on the GPU (csrc/gsr_mesh_clean.hip): the --clean stage of gaustudio/scripts/extract_mesh.py:149-186, i.e. the
Open3D pieces it uses, for the mesh that TSDFVolume.extract_triangle_mesh_device() leaves in HBM.

    clusters, n_triangles, area = cluster_connected_triangles(faces, vertices=vertices)     # o3d ...cluster_connected_triangles()
    vertices, faces, removed = remove_small_components(vertices, faces, ratio_threshold=0.5)  # extract_mesh.py:152-182
    v2, f2, vertex_index, face_index = remove_triangles_by_mask(vertices, faces, mask)      # + remove_unreferenced_vertices

Contract: INTEGRATION.md s16 (adjacency through shared undirected edges, clusters numbered by their lowest triangle index,
fp64 areas summed in a fixed order, compaction in the original order).  Deterministic.  ROCm tensors only, no CPU fallback.
Open3D parity is unpinned (tests/test_mesh_clean_open3d.py runs where Open3D is installed).
"""
import ctypes

import torch

from ._abi import call, check_mesh, on_rocm, same_device

last_rounds = 0
"""Hook-and-jump rounds of the most recent cluster_connected_triangles call (O(log F), not the mesh's diameter)."""

_ERRORS = {-2: "{what}: invalid argument (a face index out of range or a bad size)"}


def _mesh(vertices, faces):
    """(vertices float32 or None, faces int32), contiguous, checked to be one mesh on one ROCm device."""
    check_mesh(vertices, faces, vertex_dtypes=None, max_verts=(2 ** 31, "meshes are limited to V < 2^31 vertices"),
               max_faces=(2 ** 31 // 3, "meshes are limited to F < 2^31 / 3 faces"), device_exc=RuntimeError)
    f = faces.to(torch.int32).contiguous()
    if vertices is None:
        return None, f
    if not vertices.dtype.is_floating_point:
        raise TypeError(f"vertices must be a floating-point tensor, got {vertices.dtype}")
    if vertices.device != f.device:
        raise ValueError(f"vertices are on {vertices.device}, faces on {f.device}")
    return vertices.to(torch.float32).contiguous(), f


def cluster_connected_triangles(faces, num_verts=None, vertices=None):
    """Open3D TriangleMesh.cluster_connected_triangles(): (triangle_clusters [F] int32, cluster_n_triangles [C] int32,
    cluster_area [C] float64 or None).  Triangles that share an undirected edge are connected; clusters are numbered by their
    lowest triangle index.  The area needs `vertices` [V,3]; without them pass `num_verts` (default: the largest index + 1)."""
    global last_rounds
    v, f = _mesh(vertices, faces)
    dev = f.device
    F = f.shape[0]
    if num_verts is None:
        num_verts = v.shape[0] if v is not None else (int(f.max()) + 1 if F else 0)
    V = int(num_verts)
    if V < 0 or V >= 2 ** 31 or (v is not None and V != v.shape[0]):
        raise ValueError(f"num_verts = {V} does not fit the mesh")
    if F == 0:
        last_rounds = 0
        return (torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.float64, device=dev) if v is not None else None)
    clusters = torch.empty(F, dtype=torch.int32, device=dev)
    counts = torch.empty(F, dtype=torch.int32, device=dev)
    rounds = ctypes.c_int(0)
    with torch.cuda.device(dev):
        C = call("gsr_mesh_cluster_triangles", dev, f, F, V, clusters, counts, ctypes.byref(rounds), workspace=True, errors=_ERRORS)
        last_rounds = int(rounds.value)
        counts = counts[:C].clone()
        area = None
        if v is not None:
            area = torch.empty(C, dtype=torch.float64, device=dev)
            call("gsr_mesh_cluster_area", dev, v, V, f, F, clusters, C, area, workspace=True, errors=_ERRORS)
    return clusters, counts, area


def remove_triangles_by_mask(vertices, faces, remove_mask):
    """Open3D remove_triangles_by_mask(remove_mask) followed by remove_unreferenced_vertices(): (vertices' [V',3] float32,
    faces' [F',3] int32, vertex_index [V'] int32, face_index [F'] int32).  Kept faces and referenced vertices keep their
    order; the index maps (new -> old) carry per-vertex or per-face attributes across: colours[vertex_index.long()]."""
    if not torch.is_tensor(vertices) or not torch.is_tensor(faces):
        raise TypeError("vertices and faces must be torch tensors")
    v, f = _mesh(vertices, faces)
    dev = f.device
    F, V = f.shape[0], v.shape[0]
    if not torch.is_tensor(remove_mask):
        raise TypeError("remove_mask must be a torch tensor")
    if remove_mask.shape != (F,):
        raise ValueError(f"remove_mask must have shape [{F}], got {list(remove_mask.shape)}")
    if remove_mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"remove_mask must be bool or uint8, got {remove_mask.dtype}")
    on_rocm(remove_mask=remove_mask)
    same_device(dev, remove_mask=remove_mask)
    i32 = dict(dtype=torch.int32, device=dev)
    if F == 0:
        return torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), **i32), torch.zeros(0, **i32), torch.zeros(0, **i32)
    keep = (remove_mask == 0).to(torch.uint8).contiguous()
    out_v = torch.empty((V, 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((F, 3), **i32)
    vidx = torch.empty(V, **i32)
    fidx = torch.empty(F, **i32)
    nv = ctypes.c_int(0)
    nf = call("gsr_mesh_compact", dev, v, V, f, F, keep, out_v, out_f, vidx, fidx, ctypes.byref(nv), workspace=True, errors=_ERRORS)
    nv = int(nv.value)
    return out_v[:nv].clone(), out_f[:nf].clone(), vidx[:nv].clone(), fidx[:nf].clone()


def keep_clusters(cluster_n_triangles, ratio_threshold=0.5):
    """bool [C]: cluster i stays when n_i > ratio_threshold * n_largest (strict, in float64; extract_mesh.py:166-176)."""
    n = cluster_n_triangles.to(torch.float64)
    return n > float(ratio_threshold) * n[torch.argmax(n)]


def remove_small_components(vertices, faces, ratio_threshold=0.5, return_index=False):
    """extract_mesh.py:152-182 in one call: clusters the triangles, keeps the clusters with more than ratio_threshold times
    the triangles of the largest one, drops the other triangles and the vertices nothing references any more.
    Returns (vertices', faces', number of removed triangles), with return_index also (vertex_index, face_index)."""
    if not torch.is_tensor(vertices) or not torch.is_tensor(faces):
        raise TypeError("vertices and faces must be torch tensors")
    v, f = _mesh(vertices, faces)
    if f.shape[0] == 0:
        i32 = dict(dtype=torch.int32, device=f.device)
        out = (torch.zeros((0, 3), dtype=torch.float32, device=f.device), torch.zeros((0, 3), **i32), 0)
        return out + ((torch.zeros(0, **i32), torch.zeros(0, **i32)) if return_index else ())
    clusters, counts, _ = cluster_connected_triangles(f, num_verts=v.shape[0])
    remove = ~keep_clusters(counts, ratio_threshold)[clusters.long()]
    v2, f2, vidx, fidx = remove_triangles_by_mask(v, f, remove)
    removed = f.shape[0] - f2.shape[0]
    return (v2, f2, removed) + ((vidx, fidx) if return_index else ())
