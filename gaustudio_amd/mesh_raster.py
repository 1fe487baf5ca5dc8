"""Triangle mesh rendering on the GPU (csrc/gsr_mesh.hip): the PyTorch3D pieces that gaustudio/scripts/render_mesh.py and
texture_mesh.py use, for the mesh that TSDFVolume.extract_triangle_mesh_device() leaves in HBM.

    mr = MeshRasterizer(vertices, faces)                           # device tensors, e.g. straight from the TSDF volume
    frags = mr.rasterize(K, extrinsics, H, W)                      # MeshRasterizer(blur_radius=0, faces_per_pixel=1)
    mask = frags.pix_to_face >= 0                                  # render_mesh.py mask (SoftSilhouetteShader alpha > 0)
    depth = frags.zbuf                                             # render_mesh.py rendered_depth
    normal = mr.normal_map(frags, extrinsics)                      # render_mesh.py:348-353
    visible = mr.visible_faces(frags)                              # texture_mesh.py get_visible_faces, as a mask

Contract: INTEGRATION.md s15 (pixel rays at +0.5 centres, homogeneous coverage with an inclusive watertight edge test,
the least (z, face id) wins, background -1).  Forward only, deterministic.  ROCm tensors only, no CPU fallback.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _C

MAX_CHANNELS = 4

Fragments = namedtuple("Fragments", ["pix_to_face", "zbuf", "bary_coords"])
Fragments.__doc__ = """pix_to_face [H,W] int32, zbuf [H,W] float32 (camera-space z), bary_coords [H,W,3] float32; -1 on background.
(PyTorch3D's Fragments hold the same values with a batch and a faces_per_pixel axis of 1.)"""

_ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)


class _Workspace:
    """gsr_alloc_fn for the duration of one call: torch uint8 tensors (stream-ordered through torch's caching allocator),
    kept alive until the call has been enqueued."""

    def __init__(self, device):
        self.device = device
        self.bufs = []
        self.fn = _ALLOC_FN(self._alloc)

    def _alloc(self, ctx, nbytes):
        t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=self.device)
        self.bufs.append(t)
        return t.data_ptr()


def _host_f32(name, m, shape):
    a = np.asarray(m.detach().cpu().numpy() if torch.is_tensor(m) else m, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"{name} must have shape {list(shape)}, got {list(a.shape)}")
    a = a.astype(np.float32)
    return (ctypes.c_float * a.size)(*a.ravel().tolist())


def _on_rocm(**tensors):
    for name, t in tensors.items():
        if t.device.type != "cuda":
            raise RuntimeError(f"{name} is on '{t.device}': gaustudio_amd runs on ROCm devices only (no CPU fallback)")


def _check(name, rc):
    if rc == -2:
        raise ValueError(f"{name}: invalid argument (a face index out of range, a bad size or singular intrinsics)")
    if rc < 0:
        raise RuntimeError(f"{name} failed (rc={rc})")
    return rc


class MeshRasterizer:
    """Holds one device mesh: vertices [V,3] float32 (world space) and faces [F,3] int32 (int64 is converted; V, F < 2^31)."""

    def __init__(self, vertices, faces):
        if not torch.is_tensor(vertices) or not torch.is_tensor(faces):
            raise TypeError("vertices and faces must be torch tensors")
        if vertices.dim() != 2 or vertices.shape[1] != 3:
            raise ValueError(f"vertices must have shape [V, 3], got {list(vertices.shape)}")
        if faces.dim() != 2 or faces.shape[1] != 3:
            raise ValueError(f"faces must have shape [F, 3], got {list(faces.shape)}")
        if faces.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"faces must be int32 or int64, got {faces.dtype}")
        if vertices.shape[0] >= 2 ** 31 or faces.shape[0] >= 2 ** 31 // 3:
            raise ValueError("meshes are limited to V < 2^31 vertices and F < 2^31 / 3 faces")
        _on_rocm(vertices=vertices, faces=faces)
        if faces.dtype == torch.int64 and faces.numel():
            lo, hi = int(faces.min()), int(faces.max())
            if lo < -2 ** 31 or hi >= 2 ** 31:
                raise ValueError("face indices out of range")
        self.device = vertices.device
        self.verts = vertices.to(torch.float32).contiguous()
        self.faces = faces.to(device=self.device, dtype=torch.int32).contiguous()
        self._normals = None

    @property
    def num_verts(self):
        return self.verts.shape[0]

    @property
    def num_faces(self):
        return self.faces.shape[0]

    def rasterize(self, intrinsics, extrinsics, height, width, cull_backfaces=False, z_near=0.0):
        """intrinsics [3,3] (fx, fy, cx, cy), extrinsics [4,4] world-to-camera in OpenCV axes (Camera.extrinsics).
        Returns Fragments(pix_to_face, zbuf, bary_coords) of an height x width image."""
        K = _host_f32("intrinsics", intrinsics, (3, 3))
        E = _host_f32("extrinsics", extrinsics, (4, 4))
        H, W = int(height), int(width)
        if H <= 0 or W <= 0:
            raise ValueError(f"image size must be positive, got {H} x {W}")
        dev = self.device
        p2f = torch.empty((H, W), dtype=torch.int32, device=dev)
        zbuf = torch.empty((H, W), dtype=torch.float32, device=dev)
        bary = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        ws = _Workspace(dev)
        with torch.cuda.device(dev):
            rc = _C.lib().gsr_mesh_rasterize(ws.fn, None, _C._ptr(self.verts), ctypes.c_int(self.num_verts), _C._ptr(self.faces),
                                             ctypes.c_int(self.num_faces), K, E, ctypes.c_int(H), ctypes.c_int(W),
                                             ctypes.c_int(int(bool(cull_backfaces))), ctypes.c_float(float(z_near)),
                                             _C._ptr(p2f), _C._ptr(zbuf), _C._ptr(bary), _C._stream(dev))
        self.last_binned = _check("gsr_mesh_rasterize", rc)
        return Fragments(p2f, zbuf, bary)

    def _fragments(self, fragments, need_bary):
        """pix_to_face (int32) and bary_coords (float32 [..., 3]) of `fragments`, checked to be on this mesh's ROCm device."""
        p2f, bary = fragments.pix_to_face, fragments.bary_coords
        if not torch.is_tensor(p2f) or p2f.dtype != torch.int32:
            raise TypeError("fragments.pix_to_face must be an int32 tensor (MeshRasterizer.rasterize output)")
        if need_bary and (not torch.is_tensor(bary) or bary.dtype != torch.float32 or bary.shape != (*p2f.shape, 3)):
            raise TypeError(f"fragments.bary_coords must be a float32 tensor of shape {[*p2f.shape, 3]}")
        _on_rocm(pix_to_face=p2f, **({"bary_coords": bary} if need_bary else {}))
        for t in (p2f, bary) if need_bary else (p2f,):
            if t.device != self.device:
                raise ValueError(f"fragments are on {t.device}, the mesh on {self.device}")
        return p2f.contiguous(), (bary.contiguous() if need_bary else None)

    def interpolate(self, fragments, attr):
        """interpolate_face_attributes for per-vertex attributes attr [V,C] (C <= 4): [H,W,C] float32, 0 on background."""
        if not torch.is_tensor(attr) or attr.dim() != 2 or attr.shape[0] != self.num_verts:
            raise ValueError(f"attr must have shape [{self.num_verts}, C]")
        C = attr.shape[1]
        if not 1 <= C <= MAX_CHANNELS:
            raise ValueError(f"attr must have 1..{MAX_CHANNELS} channels, got {C}")
        _on_rocm(attr=attr)
        a = attr.to(device=self.device, dtype=torch.float32).contiguous()
        p2f, bary = self._fragments(fragments, need_bary=True)
        out = torch.empty((*p2f.shape, C), dtype=torch.float32, device=self.device)
        ws = _Workspace(self.device)
        with torch.cuda.device(self.device):
            rc = _C.lib().gsr_mesh_interpolate(ws.fn, None, _C._ptr(self.faces), ctypes.c_int(self.num_faces), _C._ptr(p2f),
                                               _C._ptr(bary), ctypes.c_int(p2f.numel()), _C._ptr(a), ctypes.c_int(self.num_verts),
                                               ctypes.c_int(C), _C._ptr(out), _C._stream(self.device))
        _check("gsr_mesh_interpolate", rc)
        return out

    def vertex_normals(self):
        """Meshes.verts_normals_packed: [V,3] float32, summed in a fixed order (cached)."""
        if self._normals is None:
            n = torch.empty((self.num_verts, 3), dtype=torch.float32, device=self.device)
            ws = _Workspace(self.device)
            with torch.cuda.device(self.device):
                rc = _C.lib().gsr_mesh_vertex_normals(ws.fn, None, _C._ptr(self.verts), ctypes.c_int(self.num_verts),
                                                      _C._ptr(self.faces), ctypes.c_int(self.num_faces), _C._ptr(n),
                                                      _C._stream(self.device))
            _check("gsr_mesh_vertex_normals", rc)
            self._normals = n
        return self._normals

    def normal_map(self, fragments, extrinsics):
        """render_mesh.py:348-353 over get_normals_from_fragments (:65-74): interpolate_face_attributes with barycentrics of
        ones, i.e. per pixel the SUM of the hit face's three vertex normals (one flat normal per face, not a smooth
        interpolation), normalised (F.normalize), rotated into the camera by the world-to-camera R, y and z negated:
        [H,W,3] float32, 0 on background."""
        p2f, bary = self._fragments(fragments, need_bary=True)
        ones = Fragments(p2f, fragments.zbuf, torch.ones_like(bary))
        n = self.interpolate(ones, self.vertex_normals())
        n = torch.nn.functional.normalize(n, 2.0, 2)
        E = torch.as_tensor(extrinsics, dtype=torch.float32).to(self.device)
        c2w_R = torch.linalg.inv(E)[:3, :3]
        n = n @ c2w_R
        return n * torch.tensor([1.0, -1.0, -1.0], device=self.device)

    def visible_faces(self, fragments):
        """bool [F]: the faces that appear in fragments.pix_to_face (texture_mesh.py get_visible_faces as a mask;
        mask.nonzero() gives its sorted list)."""
        p2f, _ = self._fragments(fragments, need_bary=False)
        vis = torch.empty(self.num_faces, dtype=torch.uint8, device=self.device)
        ws = _Workspace(self.device)
        with torch.cuda.device(self.device):
            rc = _C.lib().gsr_mesh_visible_faces(ws.fn, None, _C._ptr(p2f), ctypes.c_int(p2f.numel()), ctypes.c_int(self.num_faces),
                                                 _C._ptr(vis), _C._stream(self.device))
        _check("gsr_mesh_visible_faces", rc)
        return vis.bool()


def rasterize(vertices, faces, intrinsics, extrinsics, height, width, cull_backfaces=False, z_near=0.0):
    """One-shot MeshRasterizer(vertices, faces).rasterize(...)."""
    return MeshRasterizer(vertices, faces).rasterize(intrinsics, extrinsics, height, width, cull_backfaces, z_near)
