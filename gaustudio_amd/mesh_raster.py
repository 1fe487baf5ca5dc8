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

from ._abi import call, check_mesh, on_rocm

MAX_CHANNELS = 4

Fragments = namedtuple("Fragments", ["pix_to_face", "zbuf", "bary_coords"])
Fragments.__doc__ = """pix_to_face [H,W] int32, zbuf [H,W] float32 (camera-space z), bary_coords [H,W,3] float32; -1 on background.
(PyTorch3D's Fragments hold the same values with a batch and a faces_per_pixel axis of 1.)"""


def _host_f32(name, m, shape):
    a = np.asarray(m.detach().cpu().numpy() if torch.is_tensor(m) else m, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"{name} must have shape {list(shape)}, got {list(a.shape)}")
    a = a.astype(np.float32)
    return (ctypes.c_float * a.size)(*a.ravel().tolist())


_ERRORS = {-2: "{what}: invalid argument (a face index out of range, a bad size or singular intrinsics)"}
_LIMIT = "meshes are limited to V < 2^31 vertices and F < 2^31 / 3 faces"


class MeshRasterizer:
    """Holds one device mesh: vertices [V,3] float32 (world space) and faces [F,3] int32 (int64 is converted; V, F < 2^31)."""

    def __init__(self, vertices, faces):
        if not torch.is_tensor(vertices) or not torch.is_tensor(faces):
            raise TypeError("vertices and faces must be torch tensors")
        check_mesh(vertices, faces, vertex_dtypes=None, max_verts=(2 ** 31, _LIMIT), max_faces=(2 ** 31 // 3, _LIMIT),
                   device_exc=RuntimeError)
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
        self.last_binned = call("gsr_mesh_rasterize", dev, self.verts, self.num_verts, self.faces, self.num_faces, K, E, H, W,
                                bool(cull_backfaces), ctypes.c_float(float(z_near)), p2f, zbuf, bary, workspace=True, errors=_ERRORS)
        return Fragments(p2f, zbuf, bary)

    def _fragments(self, fragments, need_bary):
        """pix_to_face (int32) and bary_coords (float32 [..., 3]) of `fragments`, checked to be on this mesh's ROCm device."""
        p2f, bary = fragments.pix_to_face, fragments.bary_coords
        if not torch.is_tensor(p2f) or p2f.dtype != torch.int32:
            raise TypeError("fragments.pix_to_face must be an int32 tensor (MeshRasterizer.rasterize output)")
        if need_bary and (not torch.is_tensor(bary) or bary.dtype != torch.float32 or bary.shape != (*p2f.shape, 3)):
            raise TypeError(f"fragments.bary_coords must be a float32 tensor of shape {[*p2f.shape, 3]}")
        on_rocm(pix_to_face=p2f, **({"bary_coords": bary} if need_bary else {}))
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
        on_rocm(attr=attr)
        a = attr.to(device=self.device, dtype=torch.float32).contiguous()
        p2f, bary = self._fragments(fragments, need_bary=True)
        out = torch.empty((*p2f.shape, C), dtype=torch.float32, device=self.device)
        call("gsr_mesh_interpolate", self.device, self.faces, self.num_faces, p2f, bary, p2f.numel(), a, self.num_verts, C, out,
             workspace=True, errors=_ERRORS)
        return out

    def vertex_normals(self):
        """Meshes.verts_normals_packed: [V,3] float32, summed in a fixed order (cached)."""
        if self._normals is None:
            n = torch.empty((self.num_verts, 3), dtype=torch.float32, device=self.device)
            call("gsr_mesh_vertex_normals", self.device, self.verts, self.num_verts, self.faces, self.num_faces, n,
                 workspace=True, errors=_ERRORS)
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
        call("gsr_mesh_visible_faces", self.device, p2f, p2f.numel(), self.num_faces, vis, workspace=True, errors=_ERRORS)
        return vis.bool()


def rasterize(vertices, faces, intrinsics, extrinsics, height, width, cull_backfaces=False, z_near=0.0):
    """One-shot MeshRasterizer(vertices, faces).rasterize(...)."""
    return MeshRasterizer(vertices, faces).rasterize(intrinsics, extrinsics, height, width, cull_backfaces, z_near)
