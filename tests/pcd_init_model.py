"""The numpy model of gaustudio_amd.pcd_init (csrc/gsr_knn.hip gsr_mean_dist3, csrc/gsr_mesh_bake.hip
gsr_point_seeds / gsr_depth_seed_pack): the contracts restated operation for operation.  The GPU tests compare with it exactly;
tests/test_pcd_init_model.py compares it with the reference's own functions (tests/golden/pcd_init_ref.npz).  CPU only."""
import math

import numpy as np

import mesh_init_model as mi
import pcd_fusion_model as pm

F32 = np.float32
DEFAULT_OPACITY = F32(-2.1972246170043945)       # torch float32 log(x / (1 - x)) of x = float32(0.1) (vanilla_sg.py:95)
PCD_OPACITY = F32(np.log(0.1 / (1 - 0.1)))       # pcd.py:74, float64, stored float32


def fold3(d2):
    """[N, >=4] ascending squared distances, entry 0 the point itself (or a duplicate of it) -> float32 mean of entries 1..3."""
    d2 = np.asarray(d2, dtype=np.float64)
    return (((d2[:, 1] + d2[:, 2]) + d2[:, 3]) / 3.0).astype(F32)


def mean_dist2(points):
    """Brute force: knn_exact with k = 4; the first entry is the self distance 0, the minimum."""
    p = np.asarray(points, dtype=F32).reshape(-1, 3)
    if len(p) < 4:
        raise ValueError("mean_dist2 needs at least 4 points")
    return fold3(pm.knn_exact(p, 4)[0])


def mean_dist2_candidates(points, cand):
    """The same from candidate lists cand [N, c] (indices, the point itself among them, a superset of its 4 nearest): the
    float64 distances are recomputed by the contract's formula and the four smallest values taken."""
    p = np.asarray(points, dtype=F32).astype(np.float64).reshape(-1, 3)
    d = p[np.asarray(cand)] - p[:, None, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    return fold3(np.sort(d2, axis=1))


def scale_from_dist2(dist2):
    """log(sqrtf(dist2 + 1e-7f)), the logarithm correctly rounded from float64; [N,3]."""
    with np.errstate(all="ignore"):
        ls = mi.log32(np.sqrt(np.asarray(dist2, dtype=F32) + F32(1e-7)))
    return np.repeat(ls[:, None], 3, axis=1).astype(F32)


def point_seeds(xyz, rgb=None, scale=None, rot=None, normals=None, opacity=None, sh_degree=3):
    """create_from_attribute: dict(xyz, f_dc [N,1,3], f_rest, opacity [N,1], scale, rot)."""
    xyz = np.asarray(xyz, dtype=F32).reshape(-1, 3)
    n = len(xyz)
    if rot is not None and normals is not None:
        raise ValueError("rot and normals")
    rgb = np.ones((n, 3), dtype=F32) if rgb is None else np.asarray(rgb, dtype=F32)
    scale = scale_from_dist2(mean_dist2(xyz)) if scale is None else np.asarray(scale, dtype=F32)
    if rot is None:
        if normals is None:
            rot = np.zeros((n, 4), dtype=F32)
            rot[:, 0] = 1
        else:
            rot = mi.normal2rotation(normals)
    if opacity is None:
        opacity = DEFAULT_OPACITY
    op = np.broadcast_to(np.asarray(opacity, dtype=F32).reshape(-1, 1), (n, 1)).copy()
    return dict(xyz=xyz.copy(), f_dc=mi.rgb2sh(rgb).reshape(n, 1, 3), f_rest=np.zeros((n, (sh_degree + 1) ** 2 - 1, 3), dtype=F32),
                opacity=op, scale=scale, rot=np.asarray(rot, dtype=F32))


def pcd_init(points, colors=None, normals=None, sh_degree=3):
    return point_seeds(points, rgb=colors, normals=normals, opacity=PCD_OPACITY, sh_degree=sh_degree)


def fibonacci_sphere(samples):
    """gaussiansky.py:13-36 with Python's math, point by point: float64 (points, inward normals)."""
    pts, nrm = [], []
    phi = math.pi * (3. - math.sqrt(5.))
    for i in range(samples):
        y = 1 - (i / float(samples - 1)) * 2
        radius = math.sqrt(1 - y ** 2)
        theta = phi * i
        x, z = math.cos(theta) * radius, math.sin(theta) * radius
        pts.append((x, y, z))
        normal = (-x, -y, -z)
        mag = math.sqrt(sum(c ** 2 for c in normal))
        nrm.append(tuple(c / mag for c in normal))
    return np.array(pts), np.array(nrm)


def sky_points(resolution, radius):
    radii = list(radius) if isinstance(radius, (list, tuple, range)) else [radius]
    p, nrm = fibonacci_sphere(resolution ** 2)
    return (np.concatenate([p * float(r) for r in radii]).astype(F32), np.concatenate([nrm] * len(radii)).astype(F32))


def sky_seeds(resolution, radius, sh_degree=3):
    xyz, nrm = sky_points(resolution, radius)
    return pcd_init(xyz, np.ones_like(xyz), nrm, sh_degree)


def half_log(h):
    """float16 log in two roundings: half(float32(log(float64(h))))."""
    with np.errstate(all="ignore"):
        return np.log(np.asarray(h, dtype=np.float16).astype(np.float64)).astype(F32).astype(np.float16)


def depth_pack(world_points, image, depth, fx, fy):
    """One frame of depth_seeds from its world points [H,W,3]: (xyz, rgb, raw scale), [H*W,3] float32 each."""
    with np.errstate(all="ignore"):
        xyz = np.asarray(world_points, dtype=F32).reshape(-1, 3).astype(np.float16).astype(F32)
        c = np.asarray(image, dtype=F32).reshape(-1, 3).astype(np.float16)
        c255 = (c.astype(F32) * F32(255)).astype(np.float16)              # the float16 product, rounded once
        rgb = c255.astype(np.int32).astype(np.uint8).astype(F32) / F32(255)
        focal = (F32(fx) + F32(fy)) / F32(2)
        s = (np.asarray(depth, dtype=F32).reshape(-1) / focal).astype(np.float16)
        ls = half_log(s).astype(F32)
    return xyz, rgb, np.repeat(ls[:, None], 3, axis=1)


def depth_seeds(packs, sh_degree=3):
    """packs: depth_pack outputs per frame, concatenated in order."""
    xyz, rgb, scale = (np.concatenate([p[j] for p in packs]) for j in range(3))
    return point_seeds(xyz, rgb=rgb, scale=scale, opacity=F32(0.0), sh_degree=sh_degree)
