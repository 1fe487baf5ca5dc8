"""Float64 numpy / scipy restatement of gs-extract-pcd's normal fusion and point-cloud cleaning (the contract of
INTEGRATION.md "gs-extract-pcd"; extract_pcd.py:30-51 and :108-183).  kNN from scipy.spatial.cKDTree.  CPU only."""
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


def normal_fusion(xyz, ids_list, normals_list, conf_list, translations, k=10, sigma=0.1, consistency=0.8):
    """-> (unique_ids int64 [U], normals float64 [U,3])."""
    uids, _, m2, _ = fused_means(xyz, ids_list, normals_list, conf_list, translations, consistency)
    if len(uids) < k:
        raise ValueError("fewer fused points than k")
    q = np.asarray(xyz, dtype=np.float64)[uids]
    d2, idx = knn(q, k)
    wts = np.exp(-np.sqrt(d2) / sigma)
    s = (m2[idx] * wts[:, :, None]).sum(axis=1)
    return uids, _normalize(s)


def statistical_outlier_mask(points, nb_neighbors=50, std_ratio=2.0):
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


def normal_outlier_mask(points, normals, nb_neighbors=20, angle_threshold=np.pi / 4):
    """-> (keep bool [N], mean angle [N])."""
    p = np.asarray(points, dtype=np.float64)
    n = np.asarray(normals, dtype=np.float64)
    k = min(nb_neighbors, len(p))
    _, idx = knn(p, k)
    dots = (n[idx[:, 1:]] * n[:, None, :]).sum(axis=2)
    with np.errstate(invalid="ignore"):
        ang = np.arccos(np.abs(dots)).mean(axis=1) if k > 1 else np.full(len(p), np.nan)
    return ang < angle_threshold, ang


def clean_point_cloud(points, normals, nb_neighbors=50, std_ratio=2.0, normal_neighbors=20, angle_threshold=np.pi / 4):
    """-> ascending kept indices."""
    keep1, _, _ = statistical_outlier_mask(points, nb_neighbors, std_ratio)
    first = np.nonzero(keep1)[0]
    if len(first) == 0:
        return first
    keep2, _ = normal_outlier_mask(np.asarray(points)[first], np.asarray(normals)[first], normal_neighbors, angle_threshold)
    return first[keep2]


def view_records(median_map, final_opacity, world_normals, scene_radius):
    """extract_pcd.py:330-337 on numpy arrays."""
    H, W = median_map.shape[1:]
    op = np.asarray(final_opacity).reshape(H, W)
    valid = (median_map[0] < scene_radius * 0.8) & (op > 0.5) & (world_normals.sum(axis=-1) > -3)
    return median_map[2].astype(np.int32)[valid], -world_normals[valid], op[valid]
