"""Float64 numpy / scipy restatement of gs-extract-pcd's normal fusion and point-cloud cleaning (the contract of
INTEGRATION.md "gs-extract-pcd"; extract_pcd.py:30-51 and :108-183).  kNN from scipy.spatial.cKDTree by default, or from
knn_exact (brute force, ties broken by the index) through the `knn=` argument.  CPU only."""
import numpy as np
from scipy.spatial import cKDTree


def _normalize(v, eps=1e-12):
    n = np.sqrt((v * v).sum(axis=1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.maximum(n, eps)


def knn(points, k, queries=None):
    """(dist2 [Q,k], idx [Q,k]) from cKDTree, float64."""
    p = np.asarray(points, dtype=np.float64)
    q = p if queries is None else np.asarray(queries, dtype=np.float64)
    d, i = cKDTree(p).query(q, k=k)
    d, i = d.reshape(len(q), k), i.reshape(len(q), k)
    return d * d, i


def knn_exact(points, k, queries=None):
    """(dist2 [Q,k] float64, idx [Q,k] int64) by brute force, in ascending (dist2, index) order: the fully determined
    result that include/gsrast.h promises of gsr_knn.  dist2 = dx*dx + dy*dy + dz*dz in float64 from the float32 values
    of the coordinates, summed in that order.  Chunked over the queries (about 2^22 distances at a time)."""
    p = np.asarray(points).astype(np.float32).astype(np.float64).reshape(-1, 3)
    q = p if queries is None else np.asarray(queries).astype(np.float32).astype(np.float64).reshape(-1, 3)
    n = len(p)
    if not 1 <= k <= n:
        raise ValueError(f"k = {k} needs 1 <= k <= {n} points")
    dist2 = np.empty((len(q), k), dtype=np.float64)
    idx = np.empty((len(q), k), dtype=np.int64)
    step = max(1, (1 << 22) // n)
    for b in range(0, len(q), step):
        d = p[None, :, :] - q[b:b + step, None, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        # every entry up to the k-th distance, ties included, then ordered by (row, dist2, index); the first k of a row
        kth = np.partition(d2, k - 1, axis=1)[:, k - 1:k]
        r, c = np.nonzero(d2 <= kth)
        v = d2[r, c]
        o = np.lexsort((c, v, r))
        r, c, v = r[o], c[o], v[o]
        first = np.searchsorted(r, np.arange(d2.shape[0]))
        keep = np.arange(len(r)) - first[r] < k
        dist2[b:b + step] = v[keep].reshape(-1, k)
        idx[b:b + step] = c[keep].reshape(-1, k)
    return dist2, idx


def record_weights(xyz, ids, normals, conf, t):
    xyz = np.asarray(xyz, dtype=np.float64)
    v = np.asarray(t, dtype=np.float64)[None, :] - xyz[np.asarray(ids, dtype=np.int64)]
    d = np.sqrt((v * v).sum(axis=1))
    vw = np.abs(((v / d[:, None]) * np.asarray(normals, dtype=np.float64)).sum(axis=1))
    return np.asarray(conf, dtype=np.float64) * vw * (1.0 / (d + 1e-6))


def fused_means(xyz, ids_list, normals_list, conf_list, translations, consistency=0.8):
    """Steps 1-3: (unique_ids, mean1 [U,3], mean2 [U,3], stats) with stats the per-id |S|/W of the second pass and the
    distance of every record to its id's first mean (for the threshold-event accounting of the GPU tests)."""
    ids = np.concatenate([np.asarray(i, dtype=np.int64).reshape(-1) for i in ids_list])
    nrm = np.concatenate([np.asarray(n, dtype=np.float64).reshape(-1, 3) for n in normals_list])
    w = np.concatenate([record_weights(xyz, i, n, c, t)
                        for i, n, c, t in zip(ids_list, normals_list, conf_list, translations)])
    uids, inv = np.unique(ids, return_inverse=True)
    U = len(uids)

    def reduce(mask):
        S = np.zeros((U, 3))
        W = np.zeros(U)
        np.add.at(S, inv[mask], nrm[mask] * w[mask, None])
        np.add.at(W, inv[mask], w[mask])
        with np.errstate(invalid="ignore", divide="ignore"):
            return S / W[:, None], S, W

    m1, _, _ = reduce(np.ones(len(ids), dtype=bool))
    m1 = _normalize(m1)
    diff = np.sqrt(((nrm - m1[inv]) ** 2).sum(axis=1))
    m2, S2, W2 = reduce(diff < consistency)
    m2 = _normalize(m2)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.sqrt((S2 * S2).sum(axis=1)) / W2
    return uids, m1, m2, {"record_diff": diff, "sum_ratio": ratio, "inverse": inv}


def normal_fusion(xyz, ids_list, normals_list, conf_list, translations, k=10, sigma=0.1, consistency=0.8, knn=knn):
    """-> (unique_ids int64 [U], normals float64 [U,3]).  knn: the neighbour search of this and of the functions below
    (points, k) -> (dist2, idx); cKDTree unless given."""
    uids, _, m2, _ = fused_means(xyz, ids_list, normals_list, conf_list, translations, consistency)
    if len(uids) < k:
        raise ValueError("fewer fused points than k")
    q = np.asarray(xyz, dtype=np.float64)[uids]
    d2, idx = knn(q, k)
    wts = np.exp(-np.sqrt(d2) / sigma)
    s = (m2[idx] * wts[:, :, None]).sum(axis=1)
    return uids, _normalize(s)


def statistical_outlier_mask(points, nb_neighbors=50, std_ratio=2.0, knn=knn):
    """-> (keep bool [N], a [N], threshold)."""
    p = np.asarray(points, dtype=np.float64)
    k = min(nb_neighbors, len(p))
    d2, _ = knn(p, k)
    a = np.sqrt(d2).sum(axis=1) / k
    pos = a[a > 0]
    mean = pos.mean() if len(pos) else np.nan
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(((pos - mean) ** 2).sum() / (len(pos) - 1)) if len(pos) else np.nan
    thr = mean + std_ratio * std
    return (a > 0) & (a < thr), a, thr


def normal_outlier_mask(points, normals, nb_neighbors=20, angle_threshold=np.pi / 4, knn=knn):
    """-> (keep bool [N], mean angle [N])."""
    p = np.asarray(points, dtype=np.float64)
    n = np.asarray(normals, dtype=np.float64)
    k = min(nb_neighbors, len(p))
    _, idx = knn(p, k)
    dots = (n[idx[:, 1:]] * n[:, None, :]).sum(axis=2)
    with np.errstate(invalid="ignore"):
        ang = np.arccos(np.abs(dots)).mean(axis=1) if k > 1 else np.full(len(p), np.nan)
    return ang < angle_threshold, ang


def clean_point_cloud(points, normals, nb_neighbors=50, std_ratio=2.0, normal_neighbors=20, angle_threshold=np.pi / 4, knn=knn):
    """-> ascending kept indices."""
    keep1, _, _ = statistical_outlier_mask(points, nb_neighbors, std_ratio, knn)
    first = np.nonzero(keep1)[0]
    if len(first) == 0:
        return first
    keep2, _ = normal_outlier_mask(np.asarray(points)[first], np.asarray(normals)[first], normal_neighbors, angle_threshold, knn)
    return first[keep2]


def view_records(median_map, final_opacity, world_normals, scene_radius):
    """extract_pcd.py:330-337 on numpy arrays."""
    H, W = median_map.shape[1:]
    op = np.asarray(final_opacity).reshape(H, W)
    valid = (median_map[0] < scene_radius * 0.8) & (op > 0.5) & (world_normals.sum(axis=-1) > -3)
    return median_map[2].astype(np.int32)[valid], -world_normals[valid], op[valid]
