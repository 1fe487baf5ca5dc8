"""TSDF fusion and mesh extraction on the GPU.

Mirrors the part of `vdbfusion.VDBVolume` gs-extract-mesh uses (gaustudio/scripts/extract_mesh.py:86,115,145):

    vol = TSDFVolume(voxel_size=0.01, sdf_trunc=0.04, space_carving=False)
    vol.integrate(points_world, origin)                       # per rendered view, points stay on the GPU
    vertices, faces = vol.extract_triangle_mesh(min_weight=5)

The volume is a block-sparse grid in HBM owned by this object as torch tensors (hash keys + 4 KiB of voxels per
hash slot); the kernels are stateless (include/gsrast.h, csrc/gsr_tsdf.hip).  ROCm devices only, no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from ._abi import call
from ._block_volume import BlockVolume


class TSDFVolume(BlockVolume):
    def __init__(self, voxel_size, sdf_trunc, space_carving=False, device="cuda", capacity_blocks=1 << 18):
        """capacity_blocks: hash slots (power of two).  Every slot reserves 512 voxels x 8 B = 4 KiB of HBM, so the
        default 2^18 slots = 1 GiB holds scenes of ~130 k occupied 8^3 blocks at a load factor of 0.5."""
        self.voxel_size = float(voxel_size)
        self.sdf_trunc = float(sdf_trunc)
        self.space_carving = bool(space_carving)
        super().__init__(device, capacity_blocks)
        self._alloc(512, dtype=torch.int64)

    # ------------------------------------------------------------------ integrate
    def integrate(self, points, extrinsic=None, origin=None):
        """VDBVolume.integrate(points, extrinsic): `extrinsic` is the sensor origin [3] (what the reference passes,
        extract_mesh.py:115) or a 4x4 camera-to-world pose whose translation is the origin.
        `points`: [N,3], or an image-shaped point map [H,W,3] (what depth_to_points returns): the kernel then works in
        32 x 32 pixel patches, whose rays share voxels in both image directions -- same volume to the bit, fewer atomics."""
        o = origin if origin is not None else extrinsic
        if o is None:
            raise ValueError("integrate needs the sensor origin")
        o = np.asarray(o.detach().cpu().numpy() if torch.is_tensor(o) else o, dtype=np.float64)
        if o.shape == (4, 4):
            o = o[:3, 3]
        if o.shape != (3,):
            raise ValueError("origin must have shape [3] or [4,4]")
        pts = torch.as_tensor(points)
        row_w = 0
        if pts.dim() == 3 and pts.shape[2] == 3:
            row_w = int(pts.shape[1])
            pts = pts.reshape(-1, 3)
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError("points must have shape [N,3] or [H,W,3]")
        pts = pts.to(device=self.device, dtype=torch.float32).contiguous()
        if pts.shape[0] == 0:
            return
        origin_c = (ctypes.c_float * 3)(*[float(v) for v in o])
        call("gsr_tsdf_integrate_map", self.device, pts, pts.shape[0], row_w, origin_c, ctypes.c_float(self.voxel_size),
             ctypes.c_float(self.sdf_trunc), self.space_carving, self.keys, ctypes.c_uint64(self.capacity), self.voxels, self.status)

    def _check_overflow(self):
        st = int(self.status.item())
        if st & 1:
            raise RuntimeError(f"TSDFVolume: the block hash ({self.capacity} slots) overflowed; "
                               "create the volume with a larger capacity_blocks")
        if st & 2:
            raise RuntimeError("TSDFVolume: a voxel received more than 2^24 - 2^20 observations (the count field of the packed "
                               "voxel word is full); later observations of it were dropped")

    # ------------------------------------------------------------------ inspection
    def export_voxels(self):
        """All observed voxels as (coords [m,3] int32, tsdf [m] f32, weight [m] int32, sum_q [m] int64), sorted by
        (z, y, x).  Test / inspection helper."""
        slots, bcoords = self.occupied_blocks()
        n = slots.shape[0]
        counts = torch.empty((n, 512), dtype=torch.int32, device=self.device)
        tsdf = torch.empty((n, 512), dtype=torch.float32, device=self.device)
        sums = torch.empty((n, 512), dtype=torch.int64, device=self.device)
        if n:
            call("gsr_tsdf_export_blocks", self.device, self.voxels, slots, n, ctypes.c_float(self.sdf_trunc), counts, tsdf, sums)
        return self._sorted_voxels(bcoords, counts > 0, tsdf, counts, sums)

    # ------------------------------------------------------------------ mesh
    def extract_triangle_mesh(self, fill_holes=True, min_weight=0.5):
        """VDBVolume.extract_triangle_mesh(fill_holes, min_weight) -> (vertices [nv,3] float64, triangles [nt,3] int32)
        as numpy arrays (what trimesh.Trimesh(vertices, faces) at extract_mesh.py:146 takes)."""
        v, t = self.extract_triangle_mesh_device(fill_holes, min_weight)
        return v.double().cpu().numpy(), t.cpu().numpy()

    def extract_triangle_mesh_device(self, fill_holes=True, min_weight=0.5, clean_ratio=None):
        """(vertices [nv,3] float32, triangles [nt,3] int32) as device tensors.  clean_ratio (a float; extract_mesh.py --clean
        uses 0.5): mesh_clean.remove_small_components(vertices, triangles, clean_ratio) is applied before returning."""
        vertices, triangles = self._extract_triangle_mesh_device(fill_holes, min_weight)
        if clean_ratio is not None:
            from .mesh_clean import remove_small_components
            vertices, triangles, _ = remove_small_components(vertices, triangles, float(clean_ratio))
        return vertices, triangles

    def _extract_triangle_mesh_device(self, fill_holes, min_weight):
        return self._marching_cubes(
            "gsr_tsdf_mc_classify", (ctypes.c_float(self.sdf_trunc), ctypes.c_float(float(min_weight)), bool(fill_holes)),
            "gsr_tsdf_mc_emit", (ctypes.c_float(self.voxel_size), ctypes.c_float(self.sdf_trunc)))
