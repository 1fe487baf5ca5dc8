"""Normal fusion and point-cloud cleaning of gs-extract-pcd on the GPU, over an exact HIP kNN (csrc/gsr_knn.hip).

Mirrors what gaustudio/scripts/extract_pcd.py does after its render loop, which the reference runs on the CPU
(scipy cKDTree with a Python loop per fused point, Open3D):

    records = view_records(median_map, final_opacity, world_normals, radius)      # :330-337, per view
    fusion = NormalFusion(xyz); fusion.add_view(*records, extrinsics[:3, 3])     # :108-183 normal_fusion
    unique_ids, normals = fusion.finalize()
    keep = clean_point_cloud(xyz[unique_ids], normals)                            # :45-51

Contract and quirks: INTEGRATION.md "gs-extract-pcd".  ROCm tensors only, no CPU fallback; every call runs on the
current stream of the tensors' device.
"""
import ctypes
import math

import torch

from ._abi import call, on_rocm

MAX_K = 64


def _device_tensor(name, t, shape_last=None, dtypes=(torch.float32,)):
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch tensor")
    if shape_last is not None and (t.dim() != 2 or t.shape[1] != shape_last):
        raise ValueError(f"{name} must have shape [N, {shape_last}], got {list(t.shape)}")
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must be one of {[str(d) for d in dtypes]}, got {t.dtype}")
    return t


def _check_k(k, n, what="k"):
    if not isinstance(k, int) or isinstance(k, bool):
        raise TypeError(f"{what} must be an int")
    if k < 1 or k > MAX_K:
        raise ValueError(f"{what} must be in [1, {MAX_K}], got {k}")
    if k > n:
        raise ValueError(f"{what} = {k} needs at least {k} points, got {n}")


def _points(name, p):
    return _device_tensor(name, p, 3, (torch.float32, torch.float64))


# GSR_ERR_NONFINITE, GSR_ERR_NONFINITE_QUERY (include/gsrast.h)
_ERRORS = {-5: "{what}: a point coordinate is not finite", -6: "{what}: a coordinate of the queries is not finite"}


# ------------------------------------------------------------------------------------------------------------- kNN
def knn(points, k, queries=None):
    """Exact k nearest neighbours of each query (default: each point) among `points` [N,3] (float32, or float64 holding
    float32 values): (dist2 [Q,k] float64, idx [Q,k] int64) in ascending (squared distance, index) order, the distances in
    float64 from the float32 coordinates (what cKDTree computes on the same values).  1 <= k <= 64, k <= N.  Ties are
    broken by the index, so the output is fully determined.  Empty queries ([0,3]) give empty [0,k] outputs; a NaN or
    infinite coordinate, of the points or of the queries, raises ValueError."""
    pts = _points("points", points)
    q = None if queries is None else _points("queries", queries)
    _check_k(k, pts.shape[0])
    on_rocm(points=pts, queries=q)
    pts = pts.to(torch.float32).contiguous()
    if q is not None:
        if q.device != pts.device:
            raise ValueError("queries and points must be on the same device")
        q = q.to(torch.float32).contiguous()
    nq = pts.shape[0] if q is None else q.shape[0]
    dist2 = torch.empty((nq, k), dtype=torch.float64, device=pts.device)
    idx = torch.empty((nq, k), dtype=torch.int64, device=pts.device)
    # an empty `queries` has no address to pass (a NULL pointer means "the points themselves"): the points' address
    # stands in for it, and with num_queries = 0 nothing is read through it
    call("gsr_knn", pts.device, pts, pts.shape[0], pts if q is not None and nq == 0 else q, nq, k, dist2, idx,
         workspace=True, what="knn", errors=_ERRORS)
    return dist2, idx


# ------------------------------------------------------------------------------------------------------------- records
def scene_radius(camera_centres):
    """getNerfppNorm(cameras)["radius"] (datasets/utils.py:82-104): 1.1 * max_i |c_i - mean(c)| over the camera centres
    [N,3] (tensor or array-like).  Returns a Python float (float64)."""
    c = torch.as_tensor(camera_centres, dtype=torch.float64).reshape(-1, 3)
    if c.shape[0] == 0:
        raise ValueError("scene_radius needs at least one camera centre")
    return float((c - c.mean(dim=0, keepdim=True)).norm(dim=1).max()) * 1.1


def view_records(median_map, final_opacity, world_normals, scene_radius):
    """The records of one view (extract_pcd.py:330-337): pixels with median depth < 0.8 * scene_radius, final opacity
    > 0.5 and world_normals.sum(-1) > -3 (the -1 marker of masked normals is rotated first, so most masked pixels pass).
    median_map: the operator's [3,H,W] median output (channel 0 median depth, channel 2 median Gaussian id);
    final_opacity: [1,H,W] or [H,W]; world_normals: [H,W,3] (camera normals @ inverse(R).T).
    Returns (ids int32 [n], normals float32 [n,3] = -world_normals, confidences float32 [n] = final opacity)."""
    median_map = _device_tensor("median_map", median_map)
    if median_map.dim() != 3 or median_map.shape[0] < 3:
        raise ValueError("median_map must have shape [3, H, W]")
    H, W = median_map.shape[1:]
    op = _device_tensor("final_opacity", final_opacity).reshape(H, W)
    wn = _device_tensor("world_normals", world_normals)
    if wn.shape != (H, W, 3):
        raise ValueError(f"world_normals must have shape [{H}, {W}, 3]")
    on_rocm(median_map=median_map, final_opacity=op, world_normals=wn)
    valid = (median_map[0] < scene_radius * 0.8) & (op > 0.5)
    valid = (wn.sum(dim=-1) > -3) & valid
    return median_map[2].int()[valid], (-wn[valid]).contiguous(), op[valid].contiguous()


# ------------------------------------------------------------------------------------------------------------- fusion
class NormalFusion:
    """normal_fusion (extract_pcd.py:108-183) with the records kept on the device: add_view() computes each record's
    weight and appends {id, normal, weight} (20 B) to one growable buffer; finalize() groups by id (stable radix sort),
    runs the two per-id reductions in record order in fp64 and the 10-NN exponential smoothing.  Bit-identical from run
    to run."""

    def __init__(self, xyz):
        xyz = _device_tensor("xyz", xyz, 3)
        on_rocm(xyz=xyz)
        self.xyz = xyz.contiguous()
        self.device = xyz.device
        self.num_records = 0
        self.records = torch.empty((1 << 16, 5), dtype=torch.int32, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)

    def add_view(self, ids, normals, confidences, w2c_translation):
        """One view's records and the translation extrinsics[:3, 3] of its WORLD-TO-CAMERA matrix (the reference's
        quirk: not the camera centre)."""
        ids = _device_tensor("ids", ids, None, (torch.int32, torch.int64)).reshape(-1)
        normals = _device_tensor("normals", normals, 3)
        conf = _device_tensor("confidences", confidences).reshape(-1)
        n = ids.shape[0]
        if normals.shape[0] != n or conf.shape[0] != n:
            raise ValueError("ids, normals and confidences must have the same length")
        on_rocm(ids=ids, normals=normals, confidences=conf)
        if ids.device != self.device or normals.device != self.device or conf.device != self.device:
            raise ValueError("records must be on the device of xyz")
        t = torch.as_tensor(w2c_translation, dtype=torch.float32).detach().cpu().reshape(-1)
        if t.shape[0] != 3:
            raise ValueError("w2c_translation must have 3 elements")
        if n == 0:
            return
        need = self.num_records + n
        if need >= 2 ** 31:
            raise ValueError("NormalFusion holds at most 2^31 - 1 records")
        if need > self.records.shape[0]:
            grown = torch.empty((max(need, 2 * self.records.shape[0]), 5), dtype=torch.int32, device=self.device)
            grown[:self.num_records] = self.records[:self.num_records]
            self.records = grown
        ids = ids.to(torch.int32).contiguous()
        normals = normals.contiguous()
        conf = conf.contiguous()
        tc = (ctypes.c_float * 3)(*[float(v) for v in t.tolist()])
        call("gsr_fusion_records", self.device, self.xyz, self.xyz.shape[0], ids, normals, conf, n, tc,
             self.records[self.num_records:], self.status, errors=_ERRORS)
        self.num_records = need

    def finalize(self, k=10, sigma=0.1, consistency=0.8):
        """-> (unique_ids int32 [U] ascending, normals float32 [U,3]).  Raises ValueError with fewer than k fused points
        (the reference's cKDTree query fails there)."""
        if not isinstance(k, int) or k < 1 or k > MAX_K:
            raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
        if int(self.status.item()) & 1:
            raise ValueError(f"a record's id lies outside [0, {self.xyz.shape[0]})")
        n = self.num_records
        cap = max(min(n, self.xyz.shape[0]), 1)
        uids = torch.empty(cap, dtype=torch.int32, device=self.device)
        mean = torch.empty((cap, 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            U = call("gsr_fusion_group", self.device, self.records, n, self.xyz.shape[0], ctypes.c_float(consistency), uids, mean,
                     workspace=True, errors=_ERRORS)
            if U < k:
                raise ValueError(f"normal fusion needs at least k = {k} fused points for the smoothing, got {U}")
            uids, mean = uids[:U], mean[:U]
            out = torch.empty((U, 3), dtype=torch.float32, device=self.device)
            call("gsr_fusion_smooth", self.device, self.xyz, uids, mean, U, k, ctypes.c_float(sigma), out, workspace=True,
                 errors=_ERRORS)
        return uids, out


def normal_fusion(xyz, all_ids_list, all_normals_list, all_confidences_list, translations, k=10, sigma=0.1, consistency=0.8):
    """The reference's normal_fusion(pcd, ids, normals, confidences, cameras) in one call, with `translations` the
    per-view extrinsics[:3, 3] (world-to-camera translations) in place of the cameras."""
    f = NormalFusion(xyz)
    for ids, nrm, conf, t in zip(all_ids_list, all_normals_list, all_confidences_list, translations):
        f.add_view(ids, nrm, conf, t)
    return f.finalize(k=k, sigma=sigma, consistency=consistency)


# ------------------------------------------------------------------------------------------------------------- cleaning
def statistical_outlier_mask(points, nb_neighbors=50, std_ratio=2.0, return_distances=False):
    """Open3D remove_statistical_outlier(nb_neighbors, std_ratio) as a keep mask (bool [N]); with return_distances also
    the per-point mean kNN distance (float64 [N])."""
    pts = _points("points", points)
    n = pts.shape[0]
    if not isinstance(nb_neighbors, int) or nb_neighbors < 1 or nb_neighbors > MAX_K:
        raise ValueError(f"nb_neighbors must be in [1, {MAX_K}], got {nb_neighbors}")
    on_rocm(points=pts)
    pts = pts.to(torch.float32).contiguous()
    keep = torch.zeros(n, dtype=torch.uint8, device=pts.device)
    dist = torch.empty(n, dtype=torch.float64, device=pts.device) if return_distances else None
    if n:
        call("gsr_outlier_statistical", pts.device, pts, n, nb_neighbors, ctypes.c_double(std_ratio), keep, dist,
             workspace=True, what="statistical_outlier_mask", errors=_ERRORS)
    return (keep.bool(), dist) if return_distances else keep.bool()


def normal_outlier_mask(points, normals, nb_neighbors=20, angle_threshold=math.pi / 4):
    """remove_normal_outliers (extract_pcd.py:30-43) as a keep mask (bool [N]): neighbour 0 is dropped as the point
    itself; keep where mean(acos(|n_j . n_i|)) < angle_threshold, in float64."""
    pts = _points("points", points)
    nrm = _device_tensor("normals", normals, 3, (torch.float32, torch.float64))
    n = pts.shape[0]
    if nrm.shape[0] != n:
        raise ValueError("normals must have one row per point")
    if not isinstance(nb_neighbors, int) or nb_neighbors < 1 or nb_neighbors > MAX_K:
        raise ValueError(f"nb_neighbors must be in [1, {MAX_K}], got {nb_neighbors}")
    on_rocm(points=pts, normals=nrm)
    pts = pts.to(torch.float32).contiguous()
    keep = torch.zeros(n, dtype=torch.uint8, device=pts.device)
    if n:
        nrm = nrm.to(torch.float64).contiguous()
        call("gsr_outlier_normal", pts.device, pts, nrm, n, nb_neighbors, ctypes.c_double(angle_threshold), keep,
             workspace=True, what="normal_outlier_mask", errors=_ERRORS)
    return keep.bool()


def clean_point_cloud(points, normals, nb_neighbors=50, std_ratio=2.0, normal_neighbors=20, angle_threshold=math.pi / 4):
    """clean_point_cloud (extract_pcd.py:45-51): the statistical test, then the normal test on the points it kept (the
    kNN rebuilt over that subset).  Returns the kept indices into `points` (int64, ascending)."""
    pts = _points("points", points)
    nrm = _device_tensor("normals", normals, 3, (torch.float32, torch.float64))
    if nrm.shape[0] != pts.shape[0]:
        raise ValueError("normals must have one row per point")
    on_rocm(points=pts, normals=nrm)
    first = torch.nonzero(statistical_outlier_mask(pts, nb_neighbors, std_ratio)).flatten()
    if first.numel() == 0:
        return first
    second = normal_outlier_mask(pts[first], nrm[first], normal_neighbors, angle_threshold)
    return first[second]
