"""Visual hull from silhouette masks on the GPU (csrc/gsr_hull.hip): what the reference's `VisualHull` initializer
(gaustudio/pipelines/initializers/mask.py) does before any Gaussian exists -- carve a voxel grid against every camera's
mask, mesh what is left, seed one Gaussian per mesh vertex.

    hull = carve(cameras, masks, resolution=128)            # construct_visual_hull, mask.py:38-71
    vertices, faces = hull.extract_mesh()                    # extract_mesh, mask.py:82-93 (sap.marching_cubes for mcubes)
    cloud = hull.seeds()                                     # build_model, mask.py:95-108 -> formats.GaussianCloud
    hull, (vertices, faces), cloud = visual_hull_init(cameras, masks, resolution=128)

The carve runs one thread per voxel over per-axis coordinate tables and bit-packed masks; no [R^3, 3] point array exists.
Contract and the reference's quirks (the 'xy' meshgrid order, the sign of `translate`, raw scale / opacity of the seeds):
INTEGRATION.md s19; every operation in order: tests/visual_hull_model.py.  ROCm tensors only, no CPU fallback.  PyMCubes
parity of the mesh is unpinned (tests/test_visual_hull_mcubes.py runs where it is installed).
"""
import ctypes
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from ._abi import call, on_rocm
from .formats import CameraRecord, GaussianCloud

MASK_DTYPES = (torch.uint8, torch.bool, torch.float32)


class _HullCamera(ctypes.Structure):
    """gsr_hull_camera of include/gsrast.h (96 bytes)."""
    _fields_ = [("m", ctypes.c_float * 16), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("word_offset", ctypes.c_uint32),
                ("row_stride", ctypes.c_int32), ("has_mask", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


def camera_normalization(cameras):
    """getNerfppNorm (gaustudio/datasets/utils.py:82-104), operation for operation and with the dtypes numpy gives the
    reference: getWorld2View2 returns a float32 matrix, so its inverse, the camera centres, their mean and the distances are
    float32; the factors 1.1 and 1.5 are applied in float32 too (numpy >= 2 keeps a float32 scalar times a Python float in
    float32).  Returned as float64: dict(translate = -mean(centres) [3], radius = 1.1 max|c - centre|,
    min_radius = 1.5 min|c - centre|).  cameras: formats.CameraRecord."""
    cameras = list(cameras)
    if not cameras:
        raise ValueError("camera_normalization needs at least one camera")
    centres = []
    for cam in cameras:
        if not isinstance(cam, CameraRecord):
            raise TypeError(f"camera_normalization takes formats.CameraRecord, got {type(cam).__name__}")
        Rt = np.zeros((4, 4))
        Rt[:3, :3] = np.asarray(cam.R, dtype=np.float64).transpose()
        Rt[:3, 3] = np.asarray(cam.T, dtype=np.float64)
        Rt[3, 3] = 1.0
        w2c = np.float32(np.linalg.inv(np.linalg.inv(Rt)))       # getWorld2View2 with translate 0, scale 1
        centres.append(np.linalg.inv(w2c)[:3, 3:4])              # float32
    centres = np.hstack(centres)
    centre = np.mean(centres, axis=1, keepdims=True)
    dist = np.linalg.norm(centres - centre, axis=0, keepdims=True)
    return {"translate": -centre.flatten().astype(np.float64), "radius": float(np.float32(np.max(dist)) * np.float32(1.1)),
            "min_radius": float(np.float32(np.min(dist)) * np.float32(1.5))}


def grid_axes(resolution, radius, translate):
    """The three per-axis float32 tables of the reference's grid (mask.py:43-56): lin = np.linspace(-radius, radius, R) in
    float64, minus translate in float64, then cast: (x [R], y [R], z [R]); voxel (i, j, k) sits at (x[j], y[i], z[k])."""
    lin = np.linspace(-float(radius), float(radius), int(resolution))
    t = np.asarray(translate, dtype=np.float64).reshape(3)
    return tuple((lin - t[a]).astype(np.float32) for a in range(3))


def _camera_triples(cameras):
    """[(full_proj_transform float32 [4,4] numpy, W, H)]."""
    try:
        cameras = list(cameras)
    except TypeError:
        raise TypeError("cameras must be a list of formats.CameraRecord or (full_proj_transform, W, H) triples") from None
    if not cameras:
        raise ValueError("the camera list is empty")
    out = []
    for n, cam in enumerate(cameras):
        if isinstance(cam, CameraRecord):
            M, W, H = cam.cam.projmatrix, cam.image_width, cam.image_height
        elif isinstance(cam, (tuple, list)) and len(cam) == 3:
            M, W, H = cam
        else:
            raise TypeError(f"camera {n}: expected a formats.CameraRecord or a (full_proj_transform, W, H) triple")
        M = np.asarray(M.detach().cpu().numpy() if torch.is_tensor(M) else M)
        if M.shape != (4, 4):
            raise ValueError(f"camera {n}: full_proj_transform must have shape [4, 4], got {list(M.shape)}")
        if int(W) != W or int(H) != H or not 1 <= int(W) <= 1 << 20 or not 1 <= int(H) <= 1 << 20:
            raise ValueError(f"camera {n}: image size must be integers in [1, 2^20], got {W} x {H}")
        out.append((np.ascontiguousarray(M, dtype=np.float32), int(W), int(H)))
    return out


def _check_masks(triples, masks):
    """The device of the masks (None when every entry is None)."""
    try:
        masks = list(masks)
    except TypeError:
        raise TypeError("masks must be a list of [H, W] tensors (None entries allowed)") from None
    if len(masks) != len(triples):
        raise ValueError(f"{len(triples)} cameras but {len(masks)} masks")
    dev = None
    for n, (m, (_, W, H)) in enumerate(zip(masks, triples)):
        if m is None:
            continue
        if not torch.is_tensor(m):
            raise TypeError(f"mask {n} must be a torch tensor or None")
        if m.dtype not in MASK_DTYPES:
            raise TypeError(f"mask {n} must be uint8, bool or float32, got {m.dtype}")
        if tuple(m.shape) != (H, W):
            raise ValueError(f"mask {n} must have shape [{H}, {W}] like its camera, got {list(m.shape)}")
    for n, m in enumerate(masks):
        if m is None:
            continue
        on_rocm(ValueError, **{f"mask {n}": m})
        if dev is not None and m.device != dev:
            raise ValueError(f"mask {n} is on {m.device}, an earlier mask on {dev}")
        dev = m.device
    return masks, dev


def pack_masks(masks, sizes=None, device=None):
    """One bit per pixel for every mask of the list: (words int32 [n] on the device, [(word offset, row stride in words) or
    None per view]).  Bit x & 31 of word offset + y * stride + (x >> 5) is pixel (y, x); a pixel is set iff its value is
    nonzero.  sizes: [(W, H)] to check the masks against."""
    masks = list(masks)
    triples = [(None, m.shape[1], m.shape[0]) if torch.is_tensor(m) and m.dim() == 2 else (None, 0, 0) for m in masks] \
        if sizes is None else [(None, int(W), int(H)) for W, H in sizes]
    masks, dev = _check_masks(triples, masks)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    layout, total = [], 0
    for m in masks:
        if m is None:
            layout.append(None)
            continue
        stride = (m.shape[1] + 31) // 32
        layout.append((total, stride))
        total += stride * m.shape[0]
    if total >= 2 ** 32:
        raise ValueError("the packed masks exceed 2^32 words")
    words = torch.empty(total, dtype=torch.int32, device=dev)
    for m, lay in zip(masks, layout):
        if lay is None or m.numel() == 0:
            continue
        call("gsr_hull_pack_masks", dev, m.contiguous(), m.dtype == torch.float32, m.shape[1], m.shape[0], words,
             ctypes.c_uint64(lay[0]), lay[1], ctypes.c_uint64(total))
    return words, layout


def carve_axes(cameras, masks, axes, return_carved_by=False, device=None, packed=None):
    """The carve over explicit per-axis tables: axes = (x [R1], y [R0], z [R2]) float32 (numpy or tensors); voxel (i, j, k) of
    the grid [R0, R1, R2] sits at (x[j], y[i], z[k]).  Returns (filled bool [R0,R1,R2], count, carved_by int32 [R0,R1,R2] or
    None).  packed: the result of pack_masks for these masks (the timing tool packs once and carves repeatedly)."""
    triples = _camera_triples(cameras)
    masks, dev = _check_masks(triples, masks)
    ax = []
    for name, a in zip("xyz", axes):
        a = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
        if a.ndim != 1 or a.shape[0] < 1:
            raise ValueError(f"axis table {name} must be a non-empty vector")
        ax.append(np.ascontiguousarray(a, dtype=np.float32))
    R1, R0, R2 = (a.shape[0] for a in ax)
    if R0 * R1 * R2 >= 2 ** 31:
        raise ValueError(f"the grid must have fewer than 2^31 voxels, got {R0} x {R1} x {R2}")
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"device '{dev}': gaustudio_amd runs on ROCm devices only (no CPU fallback)")
    words, layout = pack_masks(masks, [(W, H) for _, W, H in triples], dev) if packed is None else packed
    table = (_HullCamera * len(triples))()
    for rec, (M, W, H), lay in zip(table, triples, layout):
        rec.m[:] = [float(v) for v in M.ravel()]
        rec.width, rec.height = W, H
        rec.has_mask = 0 if lay is None else 1
        rec.word_offset, rec.row_stride = (0, 0) if lay is None else lay
    table_dev = torch.empty(len(triples) * ctypes.sizeof(_HullCamera), dtype=torch.uint8, device=dev)
    axd = [torch.from_numpy(a).to(dev) for a in ax]
    filled = torch.empty((R0, R1, R2), dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    carved_by = torch.empty((R0, R1, R2), dtype=torch.int32, device=dev) if return_carved_by else None
    call("gsr_hull_carve", dev, *axd, R0, R1, R2, table, table_dev, len(triples), words, ctypes.c_uint64(words.numel()), filled,
         count, carved_by)
    return filled.bool(), int(count.item()), carved_by


@dataclass
class VisualHull:
    filled: torch.Tensor                     # bool [R,R,R]; voxel (i, j, k) sits at (axes[0][j], axes[1][i], axes[2][k])
    axes: Tuple[np.ndarray, np.ndarray, np.ndarray]
    translate: np.ndarray                    # float64 [3], the reference's dataset.cameras_center (= -centre of the cameras)
    radius: float                            # half the grid's edge
    count: int                               # number of filled voxels
    carved_by: Optional[torch.Tensor] = None  # int32 [R,R,R]: first camera (list order) that carved the voxel, -1 = filled

    @property
    def resolution(self):
        return int(self.filled.shape[0])

    def extract_mesh(self, threshold=0.5):
        """extract_mesh (mask.py:82-93): marching cubes of the binary volume at `threshold`, the first two vertex coordinates
        swapped (the grid's 'xy' indexing), face winding reversed, vertices mapped to world units by
        v / (R - 1) * 2 radius - radius - translate (float64, stored as float32).  (vertices [nv,3] float32, faces [nf,3] int32)
        on the device; face normals point away from the filled region.  An empty hull gives (0, 3) tensors."""
        from .sap import marching_cubes
        if not 0.0 < float(threshold) < 1.0:
            raise ValueError(f"threshold must lie in (0, 1) for a binary volume, got {threshold}")
        dev = self.filled.device
        if self.count == 0:
            return torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev)
        # sap.marching_cubes: inside iff value < level, normals towards increasing value.  On 1 - filled at 1 - threshold the
        # filled voxels are inside and the normals leave them: the orientation of mcubes on the volume itself.
        empty = (~self.filled).to(torch.float32)
        verts, faces = marching_cubes(empty, 1.0 - float(threshold))
        faces = torch.flip(faces, dims=(1,)).contiguous()
        R = self.resolution
        v = verts.double()[:, [1, 0, 2]]
        v = v / (R - 1) * (2 * self.radius) - self.radius
        v = v - torch.from_numpy(np.asarray(self.translate, dtype=np.float64)).to(dev)
        return v.float().contiguous(), faces

    def seeds(self, sh_degree=3, vertices=None):
        """build_model (mask.py:95-108) into VanillaPointCloud.create_from_attribute (models/vanilla_sg.py:69-97): one Gaussian
        per mesh vertex, f_dc = RGB2SH(0.5) = 0, f_rest = 0, rot = (1,0,0,0), and RAW scale = 0.01, RAW opacity = 0.1 -- the
        reference stores both without the log / inverse sigmoid its activations undo."""
        if int(sh_degree) != sh_degree or not 0 <= sh_degree <= 3:
            raise ValueError(f"sh_degree must be 0..3, got {sh_degree}")
        xyz = self.extract_mesh()[0] if vertices is None else vertices
        P, dev = xyz.shape[0], xyz.device
        full = lambda shape, v: torch.full(shape, v, dtype=torch.float32, device=dev)
        rot = full((P, 4), 0.0)
        rot[:, 0] = 1
        return GaussianCloud(xyz=xyz, f_dc=full((P, 1, 3), 0.0), f_rest=full((P, (int(sh_degree) + 1) ** 2 - 1, 3), 0.0),
                             opacity=full((P, 1), 0.1), scale=full((P, 3), 0.01), rot=rot)


def carve(cameras, masks, resolution=128, radius_scale=1.2, translate=None, radius=None, return_carved_by=False):
    """construct_visual_hull (mask.py:38-71).  cameras: formats.CameraRecord, or raw (full_proj_transform [4,4], W, H) triples;
    masks: [H,W] uint8 / bool / float32 tensors on a ROCm device (nonzero = object), None = a camera that only restricts the
    hull to its view.  translate (the reference's dataset.cameras_center) and radius (half the grid's edge; radius_scale is
    not applied to a radius that is given) default to camera_normalization's translate and min_radius * radius_scale, which
    needs CameraRecords.  A voxel outside one camera's view is carved, as in the reference."""
    if int(resolution) != resolution:
        raise TypeError("resolution must be an int")
    if resolution < 2:
        raise ValueError(f"resolution must be at least 2, got {resolution}")
    if int(resolution) ** 3 >= 2 ** 31:
        raise ValueError(f"resolution must stay below 2^31 voxels, got {resolution}^3")
    try:
        cameras = list(cameras)
    except TypeError:
        raise TypeError("cameras must be a list of formats.CameraRecord or (full_proj_transform, W, H) triples") from None
    triples = _camera_triples(cameras)
    masks, _ = _check_masks(triples, masks)
    if translate is None or radius is None:
        if not all(isinstance(c, CameraRecord) for c in cameras):
            raise ValueError("translate and radius must be given with raw (full_proj_transform, W, H) cameras")
        norm = camera_normalization(cameras)
        translate = norm["translate"] if translate is None else translate
        radius = norm["min_radius"] * float(radius_scale) if radius is None else radius
    translate = np.asarray(translate, dtype=np.float64).reshape(-1)
    if translate.shape != (3,) or not np.isfinite(translate).all():
        raise ValueError("translate must be three finite numbers")
    radius = float(radius)
    if not (radius > 0 and np.isfinite(radius)):
        raise ValueError(f"radius must be positive and finite, got {radius}")
    axes = grid_axes(int(resolution), radius, translate)
    filled, count, carved_by = carve_axes(triples, masks, axes, return_carved_by)
    return VisualHull(filled, axes, translate, radius, count, carved_by)


def visual_hull_init(cameras, masks, sh_degree=3, threshold=0.5, **conf):
    """VisualHullInitializer.__call__: carve, mesh, seeds.  conf: the arguments of carve (resolution, radius_scale, translate,
    radius).  Returns (hull, (vertices, faces), cloud)."""
    hull = carve(cameras, masks, **conf)
    vertices, faces = hull.extract_mesh(threshold)
    return hull, (vertices, faces), hull.seeds(sh_degree, vertices=vertices)
