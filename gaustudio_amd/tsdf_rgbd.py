"""Coloured TSDF fusion of posed RGB-D frames and coloured mesh extraction on the GPU.

Mirrors what the reference's `tsdf` initializer (gaustudio/pipelines/initializers/mesh.py:445-514) does with Open3D's
`ScalableTSDFVolume(voxel_length, sdf_trunc, color_type=RGB8)` on the CPU:

    vol = ColorTSDFVolume(voxel_length=0.02, sdf_trunc=0.04)
    vol.integrate(depth, color, intrinsic, extrinsic, depth_trunc=5.0)      # per frame; images stay on the GPU
    vertices, faces, colors = vol.extract_triangle_mesh_device()            # (+ normals with with_normals=True)

    vertices, faces, colors, normals = fuse_rgbd(frames)                    # TsdfInitializer._fuse_tsdf_mesh

The integration is voxel-projective (every voxel of every block a frame's depth touches projects into the depth image
and keeps a running average of tsdf and colour), unlike `TSDFVolume`, which walks the rays of a point cloud.  The volume
is a block-sparse grid in HBM owned by this object as torch tensors (hash keys + 10 KiB of float planes per hash slot);
the kernels are stateless (include/gsrast.h, csrc/gsr_tsdf_rgbd.hip).  Contract: INTEGRATION.md s18; every operation in
order: tests/tsdf_rgbd_model.py.  ROCm devices only, no CPU fallback.  Open3D parity is unpinned
(tests/test_tsdf_rgbd_open3d.py runs where Open3D is installed).
"""
import ctypes

import numpy as np
import torch

from ._abi import call
from ._block_volume import BlockVolume


def _intrinsic4(intrinsic):
    k = np.asarray(intrinsic.detach().cpu().numpy() if torch.is_tensor(intrinsic) else intrinsic, dtype=np.float64)
    if k.shape == (3, 3):
        k = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
    if k.shape != (4,):
        raise ValueError("intrinsic must be (fx, fy, cx, cy) or a 3x3 matrix")
    if not np.isfinite(k).all() or k[0] == 0 or k[1] == 0:
        raise ValueError("intrinsic must be finite with non-zero focal lengths")
    return k.astype(np.float32)


def _extrinsic_pair(extrinsic):
    """(world-to-camera, camera-to-world) as float32 [3,4]; the inverse is taken in float64."""
    E = np.asarray(extrinsic.detach().cpu().numpy() if torch.is_tensor(extrinsic) else extrinsic, dtype=np.float64)
    if E.shape != (4, 4):
        raise ValueError(f"extrinsic must be a 4x4 world-to-camera matrix, got shape {list(E.shape)}")
    if not np.isfinite(E).all() or abs(np.linalg.det(E)) < 1e-12:
        raise ValueError("extrinsic is singular (or not finite)")
    return E[:3].astype(np.float32), np.linalg.inv(E)[:3].astype(np.float32)


def _c_floats(a):
    return (ctypes.c_float * a.size)(*[float(v) for v in a.ravel()])


class ColorTSDFVolume(BlockVolume):
    def __init__(self, voxel_length=0.02, sdf_trunc=0.04, depth_sampling_stride=4, device="cuda", capacity_blocks=1 << 16):
        """capacity_blocks: hash slots (power of two).  Every slot reserves 5 planes x 512 voxels x 4 B = 10 KiB of HBM, so
        the default 2^16 slots = 640 MiB.  depth_sampling_stride: every stride-th pixel of a depth image allocates blocks
        (Open3D's depth_sampling_stride); every voxel of an allocated block is integrated."""
        self.voxel_length = float(voxel_length)
        self.sdf_trunc = float(sdf_trunc)
        self.depth_sampling_stride = int(depth_sampling_stride)
        super().__init__(device, capacity_blocks)
        if not self.voxel_length > 0 or not self.sdf_trunc > 0 or self.depth_sampling_stride < 1:
            raise ValueError("voxel_length and sdf_trunc must be positive, depth_sampling_stride at least 1")
        if self.sdf_trunc > 16 * self.voxel_length:
            raise ValueError("sdf_trunc is limited to 16 voxel lengths (a pixel then opens at most 5^3 blocks)")
        self._alloc(5, 512, dtype=torch.float32)
        self.device = self.keys.device   # "cuda" resolved to the current device's index: images are compared against it
        self.stamp = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
        self.frames = 0
        self.lane_filter = True          # tools/tsdf_rgbd_timing.py switches it off to measure it
        self.counters = None             # int64 [2] device tensor: the touch kernel counts its insertions there
        self.timings = None              # a dict: integrate() adds per-stage GPU milliseconds to it (one host wait per stage)

    # ------------------------------------------------------------------ integrate
    def _images(self, depth, color):
        if not torch.is_tensor(depth) or not torch.is_tensor(color):
            raise TypeError("depth and color must be torch tensors")
        for name, t in (("depth", depth), ("color", color)):
            if t.device.type != "cuda":
                raise RuntimeError(f"{name} is on '{t.device}': ColorTSDFVolume lives on a ROCm device (no CPU fallback)")
            if t.device != self.device:
                raise ValueError(f"{name} is on {t.device}, the volume on {self.device}")
        if depth.dim() == 3 and depth.shape[0] == 1:
            depth = depth[0]
        if depth.dim() != 2 or not depth.dtype.is_floating_point:
            raise ValueError(f"depth must be a floating-point image of shape [H,W], got {depth.dtype} {list(depth.shape)}")
        H, W = int(depth.shape[0]), int(depth.shape[1])
        if color.dtype == torch.uint8:
            if tuple(color.shape) != (H, W, 3):
                raise ValueError(f"uint8 color must have shape [{H}, {W}, 3] like depth, got {list(color.shape)}")
            mode = 0
        elif color.dtype.is_floating_point:
            if tuple(color.shape) == (H, W, 3):
                mode = 1
            elif tuple(color.shape) == (3, H, W):
                mode = 2
            else:
                raise ValueError(f"float color must have shape [{H}, {W}, 3] or [3, {H}, {W}] like depth, got {list(color.shape)}")
            color = color.to(torch.float32)
        else:
            raise TypeError(f"color must be uint8 or floating point, got {color.dtype}")
        return depth.to(torch.float32).contiguous(), color.contiguous(), mode, H, W

    def integrate(self, depth, color, intrinsic, extrinsic, depth_trunc=5.0):
        """ScalableTSDFVolume.integrate(rgbd, intrinsic, extrinsic) for one frame: depth [H,W] float in metres (non-finite,
        negative and > depth_trunc pixels are no observation), color uint8 [H,W,3] or float [H,W,3] / [3,H,W] in [0,1],
        intrinsic (fx, fy, cx, cy) or 3x3, extrinsic 4x4 world-to-camera."""
        depth, color, mode, H, W = self._images(depth, color)
        K = _intrinsic4(intrinsic)
        E, Einv = _extrinsic_pair(extrinsic)
        if H == 0 or W == 0:
            return
        self.frames += 1
        Kc, Ec, Eic = _c_floats(K), _c_floats(E), _c_floats(Einv)
        trunc, vl, st = ctypes.c_float(float(depth_trunc)), ctypes.c_float(self.voxel_length), ctypes.c_float(self.sdf_trunc)
        with torch.cuda.device(self.device):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if self.timings is not None else None
            if ev:
                ev[0].record()
            call("gsr_ctsdf_touch", self.device, depth, W, H, self.depth_sampling_stride, Kc, Eic, trunc, vl, st, self.keys,
                 ctypes.c_uint64(self.capacity), self.stamp, self.frames, self.status, int(self.lane_filter), self.counters)
            if ev:
                ev[1].record()
            touched = torch.nonzero(self.stamp == self.frames).flatten().to(torch.int32)
            self.last_touched = int(touched.shape[0])
            if ev:
                ev[2].record()
            call("gsr_ctsdf_integrate", self.device, depth, color, mode, W, H, Kc, Ec, trunc, vl, st, self.keys, touched,
                 self.last_touched, self.voxels)
            if ev:
                ev[3].record()
                torch.cuda.synchronize(self.device)
                for name, a, b in (("touch_ms", 0, 1), ("compact_ms", 1, 2), ("integrate_ms", 2, 3)):
                    self.timings[name] = self.timings.get(name, 0.0) + ev[a].elapsed_time(ev[b])

    def _check_overflow(self):
        if int(self.status.item()) & 1:
            raise RuntimeError(f"ColorTSDFVolume: the block hash ({self.capacity} slots) overflowed; "
                               "create the volume with a larger capacity_blocks")

    # ------------------------------------------------------------------ inspection
    def export_voxels(self):
        """All observed voxels (weight > 0) as (coords [m,3] int32, tsdf [m] f32, weight [m] f32, color [m,3] f32 in 0..255),
        sorted by (z, y, x).  Test / inspection helper."""
        slots, bcoords = self.occupied_blocks()
        n = slots.shape[0]
        tsdf = torch.empty((n, 512), dtype=torch.float32, device=self.device)
        weight = torch.empty((n, 512), dtype=torch.float32, device=self.device)
        color = torch.empty((n, 512, 3), dtype=torch.float32, device=self.device)
        if n:
            call("gsr_ctsdf_export_blocks", self.device, self.voxels, slots, n, tsdf, weight, color)
        return self._sorted_voxels(bcoords, weight > 0, tsdf, weight, color)

    # ------------------------------------------------------------------ mesh
    def extract_triangle_mesh(self, min_weight=0.0, clean_ratio=None, with_normals=False):
        """(vertices [nv,3] float64, triangles [nt,3] int32, colors [nv,3] float64 in [0,1]) as numpy arrays (what Open3D's
        TriangleMesh holds); with_normals also the vertex normals [nv,3] float64."""
        out = self.extract_triangle_mesh_device(min_weight, clean_ratio, with_normals)
        return tuple(t.cpu().numpy() if t.dtype == torch.int32 else t.double().cpu().numpy() for t in out)

    def extract_triangle_mesh_device(self, min_weight=0.0, clean_ratio=None, with_normals=False):
        """(vertices [nv,3] float32, triangles [nt,3] int32, colors [nv,3] float32 in [0,1]) as device tensors.
        clean_ratio (a float; extract_mesh.py --clean uses 0.5): mesh_clean.remove_small_components is applied, colours follow
        its vertex index map.  with_normals: also mesh_raster's fixed-order vertex normals of the returned mesh (what
        mesh.compute_vertex_normals() supplies at mesh.py:513)."""
        vertices, triangles, colors = self._extract_triangle_mesh_device(min_weight)
        if clean_ratio is not None:
            from .mesh_clean import remove_small_components
            vertices, triangles, _, vidx, _ = remove_small_components(vertices, triangles, float(clean_ratio), return_index=True)
            colors = colors[vidx.long()]
        if not with_normals:
            return vertices, triangles, colors
        from .mesh_raster import MeshRasterizer
        normals = (MeshRasterizer(vertices, triangles).vertex_normals() if vertices.shape[0]
                   else torch.zeros((0, 3), dtype=torch.float32, device=self.device))
        return vertices, triangles, colors, normals

    def _extract_triangle_mesh_device(self, min_weight, timings=None):
        return self._marching_cubes("gsr_ctsdf_mc_classify", (ctypes.c_float(float(min_weight)),),
                                    "gsr_ctsdf_mc_emit", (ctypes.c_float(self.voxel_length),), vertex_extras=1, timings=timings)


def _frame_parts(frame):
    """(depth, color, intrinsic, extrinsic) of one element of `frames`; None when it has no depth or no pose."""
    if len(frame) == 4:
        depth, color, intrinsic, extrinsic = frame
    elif len(frame) == 3:                                   # (CameraRecord, depth, color)
        from .formats import fov2focal
        rec, depth, color = frame
        if depth is None or rec is None or rec.R is None or rec.T is None:
            return None
        H, W = depth.shape[-2], depth.shape[-1]
        intrinsic = (fov2focal(rec.FoVx, W), fov2focal(rec.FoVy, H), W * 0.5, H * 0.5)
        extrinsic = np.eye(4)
        extrinsic[:3, :3] = np.asarray(rec.R, dtype=np.float64).transpose()
        extrinsic[:3, 3] = np.asarray(rec.T, dtype=np.float64)
    else:
        raise ValueError("a frame is (depth, color, intrinsic, extrinsic) or (CameraRecord, depth, color)")
    if depth is None or color is None or extrinsic is None:
        return None
    return depth, color, intrinsic, extrinsic


def fuse_rgbd(frames, voxel_size=0.02, sdf_trunc=0.04, max_depth=5.0, downsample_scale=1, device="cuda",
              capacity_blocks=1 << 16):
    """TsdfInitializer._fuse_tsdf_mesh (mesh.py:460-514): integrates every frame that has depth and a pose into a
    ColorTSDFVolume and extracts the coloured mesh with vertex normals: (vertices, triangles, colors, normals) as device
    tensors.  `frames` yields (depth, color, intrinsic, extrinsic) or (CameraRecord, depth, color); frames whose depth,
    colour or pose is None are skipped, as the reference skips them.  downsample_scale s > 1 takes every s-th pixel of both
    images and divides fx, fy, cx, cy by s (the reference resizes its images by interpolation there, Camera.downsample_scale;
    depth is not interpolated across silhouettes here)."""
    vol = ColorTSDFVolume(voxel_size, sdf_trunc, device=device, capacity_blocks=capacity_blocks)
    s = max(1, int(downsample_scale))
    for frame in frames:
        parts = _frame_parts(frame)
        if parts is None:
            continue
        depth, color, intrinsic, extrinsic = parts
        depth = torch.as_tensor(depth).to(vol.device)
        color = torch.as_tensor(color).to(vol.device)
        if depth.dim() == 3 and depth.shape[0] == 1:
            depth = depth[0]
        K = _intrinsic4(intrinsic).astype(np.float64)
        if s > 1:
            chw = color.dim() == 3 and color.shape[0] == 3 and color.shape[-1] != 3
            depth = depth[::s, ::s]
            color = color[:, ::s, ::s] if chw else color[::s, ::s]
            K = np.array([K[0] / s, K[1] / s, K[2] / s, K[3] / s])
        vol.integrate(depth, color, K, extrinsic, depth_trunc=max_depth)
    return vol.extract_triangle_mesh_device(with_normals=True)
