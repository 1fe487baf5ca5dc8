"""What TSDFVolume (tsdf.py) and ColorTSDFVolume (tsdf_rgbd.py) share: a block-sparse grid in HBM -- an open-addressing hash of
int64 block keys, one row of 8^3 voxels per hash slot, a status word -- and the two-pass marching cubes over its occupied
blocks.  The layout of a voxel row, integrate() and the overflow texts are the subclasses'."""
import ctypes

import torch

from ._abi import call

_EMPTY = -1          # all bits set, as int64


class BlockVolume:
    def __init__(self, device, capacity_blocks):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} lives on a ROCm device, got '{self.device}' (no CPU fallback)")
        if capacity_blocks & (capacity_blocks - 1) or capacity_blocks <= 0:
            raise ValueError("capacity_blocks must be a power of two")
        self.capacity = int(capacity_blocks)

    def _alloc(self, *voxel_shape, dtype):
        """keys, voxels [capacity, *voxel_shape] and status, once the subclass has checked its own arguments."""
        self.keys = torch.full((self.capacity,), _EMPTY, dtype=torch.int64, device=self.device)
        self.voxels = torch.zeros((self.capacity, *voxel_shape), dtype=dtype, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)

    # ------------------------------------------------------------------ inspection
    def occupied_blocks(self):
        """(slots [n] int32, block coordinates [n,3] int32), ordered by block key (deterministic)."""
        self._check_overflow()
        slots = torch.nonzero(self.keys != _EMPTY).flatten()
        k = self.keys[slots]
        k, order = torch.sort(k)
        slots = slots[order]
        B = 1 << 20
        coords = torch.stack([((k >> 42) & 0x1fffff) - B, ((k >> 21) & 0x1fffff) - B, (k & 0x1fffff) - B], dim=1)
        return slots.to(torch.int32).contiguous(), coords.to(torch.int32)

    def _sorted_voxels(self, bcoords, observed, *planes):
        """(coords [m,3] int32, *planes [m, ...]) of the voxels with observed[block, voxel], sorted by (z, y, x)."""
        local = torch.arange(512, device=self.device)
        lx, ly, lz = local & 7, (local >> 3) & 7, local >> 6
        coords = bcoords[:, None, :] * 8 + torch.stack([lx, ly, lz], dim=1)[None].to(torch.int32)
        coords, *planes = (t[observed] for t in (coords, *planes))
        key = (coords[:, 2].long() << 42) + (coords[:, 1].long() << 21) + coords[:, 0].long()
        order = torch.argsort(key)
        return (coords[order], *(p[order] for p in planes))

    # ------------------------------------------------------------------ mesh
    def _marching_cubes(self, classify, classify_args, emit, emit_args, vertex_extras=0, timings=None):
        """The two passes `classify` and `emit` (entry-point names) over the occupied blocks, with the volume's scalar
        arguments spliced in: (vertices [nv,3] float32, triangles [nt,3] int32, *vertex_extras further [nv,3] float32 outputs
        of emit).  timings: a dict that receives classify_ms and emit_ms (one host wait)."""
        slots, _ = self.occupied_blocks()
        n = slots.shape[0]
        dev = self.device
        if n == 0:
            z = lambda dt: torch.zeros((0, 3), dtype=dt, device=dev)
            return (z(torch.float32), z(torch.int32), *(z(torch.float32) for _ in range(vertex_extras)))
        slot_to_block = torch.zeros(self.capacity, dtype=torch.int32, device=dev)
        slot_to_block[slots.long()] = torch.arange(n, dtype=torch.int32, device=dev)
        cases = torch.empty((n, 512), dtype=torch.uint8, device=dev)
        flags = torch.empty((n, 512), dtype=torch.int32, device=dev)
        bnv = torch.empty(n, dtype=torch.int32, device=dev)
        bnt = torch.empty(n, dtype=torch.int32, device=dev)
        blocks = (self.keys, ctypes.c_uint64(self.capacity), self.voxels, slots, n, slot_to_block)
        with torch.cuda.device(dev):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timings is not None else None
            if ev:
                ev[0].record()
            call(classify, dev, *blocks, *classify_args, cases, flags, bnv, bnt)
            if ev:
                ev[1].record()
            voff = torch.cumsum(bnv.long(), 0)
            toff = torch.cumsum(bnt.long(), 0)
            nv, nt = int(voff[-1].item()), int(toff[-1].item())
            if nv >= 2 ** 31 or nt >= 2 ** 31:
                raise RuntimeError("mesh too large for 32-bit indices")
            voff = (voff - bnv).to(torch.int32).contiguous()
            toff = (toff - bnt).to(torch.int32).contiguous()
            vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
            extras = [torch.empty((nv, 3), dtype=torch.float32, device=dev) for _ in range(vertex_extras)]
            triangles = torch.empty((nt, 3), dtype=torch.int32, device=dev)
            vbase = torch.empty((n, 512), dtype=torch.int32, device=dev)
            if ev:
                ev[2].record()
            if nt:
                call(emit, dev, *blocks, *emit_args, cases, flags, voff, toff, vbase, vertices, *extras, triangles)
            if ev:
                ev[3].record()
                torch.cuda.synchronize(dev)
                timings["classify_ms"] = ev[0].elapsed_time(ev[1])
                timings["emit_ms"] = ev[2].elapsed_time(ev[3])
        return (vertices, triangles, *extras)
