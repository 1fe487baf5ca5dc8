"""Gaussian seeds from a point cloud on the GPU: what every point-cloud initializer of the reference ends in,
VanillaPointCloud.create_from_attribute (gaustudio/models/vanilla_sg.py:69-97), with the 3-nearest-neighbour mean squared
distance it takes from simple-knn's distCUDA2 (or scipy's KDTree, :9-14) when no scale is given.

    d2 = mean_dist2(points)                                     # [N] float32 (csrc/gsr_knn.hip gsr_mean_dist3)
    cloud = point_seeds(xyz, rgb, scale, rot, normals, opacity) # create_from_attribute (csrc/gsr_mesh_bake.hip gsr_point_seeds)
    cloud = pcd_init(points, colors, normals)                   # PcdInitializer.build_model (initializers/pcd.py:58-77)
    cloud = pcd_init_from_ply(path, device)
    cloud = sky_seeds(resolution, radius)                       # GaussianSky / MultiGaussianSky (initializers/gaussiansky.py)
    cloud = depth_seeds(frames)                                 # DepthInitializer (initializers/depth.py) without its files

Every function returns a formats.GaussianCloud of raw (pre-activation) float32 parameters.  Contract and the reference's
quirks: INTEGRATION.md s22.  ROCm tensors only, no CPU fallback; every call runs on the current stream of the tensors' device.
"""
import ctypes
import math

import numpy as np
import torch

from ._abi import call, on_rocm, same_device
from .formats import GaussianCloud, read_ply_vertices
from .pcd_fusion import _ERRORS
from .postprocess import depth_to_points


def _f32(name, t, last, optional=True):
    """[N, last] float32 tensor (or None)."""
    if t is None and optional:
        return None
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch tensor" + (" or None" if optional else ""))
    if t.dim() != 2 or t.shape[1] != last:
        raise ValueError(f"{name} must have shape [N, {last}], got {list(t.shape)}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t


def _sh_degree(sh_degree):
    if isinstance(sh_degree, bool) or int(sh_degree) != sh_degree or not 0 <= sh_degree <= 3:
        raise ValueError(f"sh_degree must be 0..3, got {sh_degree}")
    return int(sh_degree)


def _ready(t):
    return None if t is None else t.detach().contiguous()


# ------------------------------------------------------------------------------------------------------------- 3-NN
def mean_dist2(points, return_stats=False, cell_target=None):
    """distCUDA2 / calculate_dist2_python: for each of points [N,3] (float32) the mean of the squared distances to its three
    nearest OTHER points (a duplicate coordinate counts, at distance 0), [N] float32.  Each squared distance is
    dx*dx + dy*dy + dz*dz in float64 from the float32 coordinates and the mean is ((d1 + d2) + d3) / 3.0 in float64, cast
    once: only values enter, so the result is fully determined and bit-identical from run to run.  N >= 4 (the reference
    yields inf or garbage below); a NaN or infinite coordinate raises ValueError.

    return_stats: also a dict -- `occupied_cells` of the hashed grid, `shell2_lanes` (points whose three neighbours were not
    settled by the 27 cells around them), `leftovers` (points answered by the wave-per-query kNN instead: far outliers, sparse
    regions, N near 4) and the GPU milliseconds `grid_ms`, `query_ms`, `fallback_ms`.  cell_target: points per occupied grid
    cell the build aims at (1..64; None = the library's measured default); the result does not depend on it."""
    pts = _f32("points", points, 3, optional=False)
    n = pts.shape[0]
    if n < 4:
        raise ValueError(f"mean_dist2 needs at least 4 points (three neighbours each), got {n}")
    if n >= 2 ** 31:
        raise ValueError("mean_dist2 takes fewer than 2^31 points")
    if cell_target is not None and (isinstance(cell_target, bool) or int(cell_target) != cell_target or not 1 <= cell_target <= 64):
        raise ValueError(f"cell_target must be in [1, 64], got {cell_target!r}")
    on_rocm(points=pts)
    pts = _ready(pts)
    out = torch.empty(n, dtype=torch.float32, device=pts.device)
    stats = (ctypes.c_int * 3)()
    ms = (ctypes.c_float * 3)() if return_stats else None
    call("gsr_mean_dist3_ex", pts.device, pts, n, out, int(cell_target or 0), stats, ms, workspace=True, what="mean_dist2",
         errors=_ERRORS)
    if not return_stats:
        return out
    return out, dict(occupied_cells=int(stats[0]), shell2_lanes=int(stats[1]), leftovers=int(stats[2]),
                     grid_ms=float(ms[0]), query_ms=float(ms[1]), fallback_ms=float(ms[2]))


# ------------------------------------------------------------------------------------------------------------- seeds
_DEFAULT_OPACITY = None


def default_opacity():
    """inverse_sigmoid(0.1) as create_from_attribute evaluates it (vanilla_sg.py:95): torch CPU float32 ops, once."""
    global _DEFAULT_OPACITY
    if _DEFAULT_OPACITY is None:
        x = 0.1 * torch.ones((1, 1), dtype=torch.float32)
        _DEFAULT_OPACITY = float(torch.log(x / (1 - x)).item())
    return _DEFAULT_OPACITY


def point_seeds(xyz, rgb=None, scale=None, rot=None, normals=None, opacity=None, sh_degree=3, dist2=None):
    """VanillaPointCloud.create_from_attribute(xyz, rgb, scale, rot, opacity) in one kernel, float32 throughout:

      xyz      copied
      f_dc     (rgb - 0.5) / C0; rgb = 1 when None.  f_rest = 0 for sh_degree (0..3)
      scale    copied when given; otherwise log(sqrt(mean_dist2(xyz) + 1e-7)) on all three axes (the logarithm correctly
               rounded from float64), which needs N >= 4
      rot      copied when given; from `normals` [N,3] the initializers' normal2rotation (its sign() cases and its quaternion
               that is not normalised as in mesh_init); otherwise (1, 0, 0, 0).  Both given: ValueError
      opacity  a [N,1] tensor, or a Python float for every point; None = the reference's float32 inverse_sigmoid(0.1)

    dist2 (not in the reference): a mean_dist2(xyz) the caller already has ([N] float32), used instead of a second search when
    no scale is given.  N = 0 gives an empty cloud when a scale is supplied."""
    xyz = _f32("xyz", xyz, 3, optional=False)
    rgb, scale, normals = _f32("rgb", rgb, 3), _f32("scale", scale, 3), _f32("normals", normals, 3)
    rot = _f32("rot", rot, 4)
    if dist2 is not None:
        if not torch.is_tensor(dist2) or dist2.dtype != torch.float32 or tuple(dist2.shape) != (xyz.shape[0],):
            raise ValueError(f"dist2 must be a float32 tensor of shape [{xyz.shape[0]}]")
        if scale is not None:
            raise ValueError("give scale or dist2, not both")
    if rot is not None and normals is not None:
        raise ValueError("give rot or normals, not both")
    op_t = None
    if torch.is_tensor(opacity):
        op_t = _f32("opacity", opacity, 1)
    elif opacity is not None and (isinstance(opacity, bool) or not isinstance(opacity, (int, float))):
        raise TypeError("opacity must be a [N,1] float32 tensor, a float or None")
    n = xyz.shape[0]
    for name, t in (("rgb", rgb), ("scale", scale), ("rot", rot), ("normals", normals), ("opacity", op_t)):
        if t is not None and t.shape[0] != n:
            raise ValueError(f"{name} must have one row per point ({n}), got {t.shape[0]}")
    deg = _sh_degree(sh_degree)
    if n >= 2 ** 31:
        raise ValueError("point_seeds takes fewer than 2^31 points")
    if scale is None and dist2 is None and n < 4:
        raise ValueError(f"point_seeds without a scale needs at least 4 points (three neighbours each), got {n}")
    on_rocm(xyz=xyz, rgb=rgb, scale=scale, rot=rot, normals=normals, opacity=op_t, dist2=dist2)
    dev = xyz.device
    same_device(dev, ref="the points", rgb=rgb, scale=scale, rot=rot, normals=normals, opacity=op_t, dist2=dist2)
    xyz, rgb, scale, rot, normals, op_t, dist2 = (_ready(t) for t in (xyz, rgb, scale, rot, normals, op_t, dist2))
    if scale is None and dist2 is None:
        dist2 = mean_dist2(xyz)
    op = default_opacity() if opacity is None else (0.0 if op_t is not None else float(opacity))
    new = lambda c: torch.empty((n, c), dtype=torch.float32, device=dev)
    o_xyz, f_dc, o_scale, o_rot, o_op = new(3), new(3), new(3), new(4), new(1)
    call("gsr_point_seeds", dev, xyz, rgb, dist2, scale, rot, normals, op_t, ctypes.c_float(op), n, o_xyz, f_dc, o_scale, o_rot, o_op)
    return GaussianCloud(xyz=o_xyz, f_dc=f_dc.reshape(n, 1, 3),
                         f_rest=torch.zeros((n, (deg + 1) ** 2 - 1, 3), dtype=torch.float32, device=dev),
                         opacity=o_op, scale=o_scale, rot=o_rot)


# ------------------------------------------------------------------------------------------------------------- pcd
PCD_OPACITY = float(np.float32(np.log(0.1 / (1 - 0.1))))      # pcd.py:74 inverse_sigmoid(0.1) in float64, stored float32


def pcd_init(points, colors=None, normals=None, sh_degree=3):
    """PcdInitializer.build_model (initializers/pcd.py:58-77): points [N,3], colors [N,3] in [0, 1] or None (white), normals
    [N,3] or None, float32 on a ROCm device.  Rotations from the normals when there are any, scales from mean_dist2, raw
    opacity float32(log(0.1 / 0.9))."""
    return point_seeds(points, rgb=colors, normals=normals, opacity=PCD_OPACITY, sh_degree=sh_degree)


def ply_point_cloud(path):
    """(points, colors or None, normals or None) float32 arrays of a PLY file's vertex element: x, y, z; red, green, blue
    (integer properties divided by 255 in float64, as Open3D reads them, then cast) and nx, ny, nz when all three are there."""
    v = read_ply_vertices(path)
    names = v.dtype.names
    for a in "xyz":
        if a not in names:
            raise ValueError(f"{path}: the vertex element has no property {a!r}")
    col = lambda keys: np.stack([np.asarray(v[k], dtype=np.float64) for k in keys], axis=1)
    points = col("xyz").astype(np.float32)
    colors = normals = None
    if all(k in names for k in ("red", "green", "blue")):
        colors = col(("red", "green", "blue"))
        if v.dtype["red"].kind in "iu":
            colors = colors / 255.0
        colors = colors.astype(np.float32)
    if all(k in names for k in ("nx", "ny", "nz")):
        normals = col(("nx", "ny", "nz")).astype(np.float32)
    return points, colors, normals


def pcd_init_from_ply(path, device="cuda", sh_degree=3):
    """pcd_init of a PLY point cloud (formats.read_ply_vertices; agreement with Open3D's reader is unpinned)."""
    dev = torch.device(device)
    points, colors, normals = ply_point_cloud(path)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return pcd_init(up(points), up(colors), up(normals), sh_degree=sh_degree)


# ------------------------------------------------------------------------------------------------------------- sky
def fibonacci_sphere(samples):
    """gaussiansky.py:13-36 point by point in Python float64 with `math`: (points [S,3], inward unit normals [S,3]) float64."""
    points, normals = [], []
    phi = math.pi * (3. - math.sqrt(5.))
    for i in range(samples):
        y = 1 - (i / float(samples - 1)) * 2
        radius = math.sqrt(1 - y ** 2)
        theta = phi * i
        x = math.cos(theta) * radius
        z = math.sin(theta) * radius
        points.append((x, y, z))
        normal = (-x, -y, -z)
        magnitude = math.sqrt(sum(n ** 2 for n in normal))
        normals.append(tuple(n / magnitude for n in normal))
    return np.array(points), np.array(normals)


def sky_points(resolution=100, radius=100.0):
    """The PLY that GaussianSkyInitializer / MultiGaussianSkyInitializer cache, as float32 arrays (its f4 properties):
    (points, normals) of resolution^2 Fibonacci points per radius, the shells concatenated in the order of `radius`."""
    if isinstance(resolution, bool) or int(resolution) != resolution:
        raise TypeError("resolution must be an int")
    if resolution < 2:
        raise ValueError(f"resolution must be at least 2 (the reference divides by zero below), got {resolution}")
    radii = [float(r) for r in (radius if isinstance(radius, (list, tuple, range, np.ndarray)) else [radius])]
    if not radii:
        raise ValueError("radius must not be empty")
    if int(resolution) ** 2 * len(radii) >= 2 ** 31:
        raise ValueError("sky_seeds: 2^31 points or more")
    p, nrm = fibonacci_sphere(int(resolution) ** 2)
    xyz = np.concatenate([p * r for r in radii], axis=0)
    return xyz.astype(np.float32), np.concatenate([nrm] * len(radii), axis=0).astype(np.float32)


def sky_seeds(resolution=100, radius=100.0, device="cuda", sh_degree=3):
    """GaussianSkyInitializer (radius a number) / MultiGaussianSkyInitializer (radius a sequence: one shell each): white
    Gaussians on Fibonacci spheres, rotations from the inward normals, then as pcd_init."""
    deg = _sh_degree(sh_degree)
    xyz, nrm = sky_points(resolution, radius)
    dev = torch.device(device)
    points = torch.from_numpy(xyz).to(dev)
    return pcd_init(points, torch.ones_like(points), torch.from_numpy(nrm).to(dev), sh_degree=deg)


# ------------------------------------------------------------------------------------------------------------- depth
def _focal(intrinsics):
    k = np.asarray(intrinsics.detach().cpu() if torch.is_tensor(intrinsics) else intrinsics, dtype=np.float32).reshape(3, 3)
    return float((k[0, 0] + k[1, 1]) / np.float32(2))


def depth_seeds(frames, sh_degree=3):
    """DepthInitializer without its disk round trip.  frames: (depth [H,W], image [H,W,3], intrinsics [3,3], extrinsics [4,4]
    world-to-camera) per view, depth and image float32 on a ROCm device, already downsampled by the caller
    (Camera.downsample_scale(4) in the reference).  Per pixel, frames in order, pixels row-major:

      xyz      depth_to_points(depth, 'world') rounded through float16 (the reference's cache file)
      rgb      half(image) * 255 in half, truncated to uint8, / 255 in float32; the image's values lie in [0, 1] -- negative
               or NaN colours are outside the contract (the reference's uint8 cast of them is undefined)
      scale    s = half(depth / ((fx + fy) / 2)); raw scale half(log(s)) on all three axes: -inf for a depth of 0, which the
               reference keeps too (it filters nothing)
      opacity  0.0 = inverse_sigmoid(0.5); rot (1, 0, 0, 0)"""
    deg = _sh_degree(sh_degree)
    frames = list(frames)
    if not frames:
        raise ValueError("depth_seeds needs at least one frame")
    checked = []
    for j, fr in enumerate(frames):
        if len(fr) != 4:
            raise ValueError(f"frame {j}: expected (depth, image, intrinsics, extrinsics)")
        depth, image, K, E = fr
        for name, t in (("depth", depth), ("image", image)):
            if not torch.is_tensor(t):
                raise TypeError(f"frame {j}: {name} must be a torch tensor")
            if t.dtype != torch.float32:
                raise TypeError(f"frame {j}: {name} must be float32, got {t.dtype}")
        if depth.dim() != 2:
            raise ValueError(f"frame {j}: depth must have shape [H, W], got {list(depth.shape)}")
        if tuple(image.shape) != (depth.shape[0], depth.shape[1], 3):
            raise ValueError(f"frame {j}: image must have shape [{depth.shape[0]}, {depth.shape[1]}, 3], got {list(image.shape)}")
        checked.append((depth, image, K, E))
    total = sum(d.numel() for d, _, _, _ in checked)
    if total >= 2 ** 31:
        raise ValueError("depth_seeds: 2^31 pixels or more")
    for j, (depth, image, _, _) in enumerate(checked):
        on_rocm(**{f"frame {j}: depth": depth, f"frame {j}: image": image})
    dev = checked[0][0].device
    new = lambda: torch.empty((total, 3), dtype=torch.float32, device=dev)
    xyz, rgb, scale = new(), new(), new()
    off = 0
    for j, (depth, image, K, E) in enumerate(checked):
        same_device(dev, ref="the points", **{f"frame {j}: depth": depth, f"frame {j}: image": image})
        n = depth.numel()
        if n == 0:
            continue
        depth, image = _ready(depth), _ready(image)
        pts = depth_to_points(depth, K, E, "world")
        call("gsr_depth_seed_pack", dev, pts, image, depth, n, ctypes.c_float(_focal(K)), xyz[off:], rgb[off:], scale[off:])
        off += n
    return point_seeds(xyz, rgb=rgb, scale=scale, opacity=0.0, sh_degree=deg)
