"""gs-extract-pcd normal fusion / cleaning: the float64 model against the reference's own normal_fusion (fixture), the
exact (dist2, index)-ordered kNN of the model against cKDTree, the small cleaning inputs of the GPU edge tests (none may
sit at a threshold), and the argument checks of gaustudio_amd.pcd_fusion that need no device."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pcd_edge_cases as edge  # noqa: E402
import pcd_fusion_model as model  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "py_pcd_fusion.npz")


def fixture_case(name):
    z = np.load(FIXTURE)
    sizes = z[f"{name}_view_sizes"]
    cuts = np.cumsum(sizes)[:-1]
    return dict(xyz=z[f"{name}_xyz"], ids=np.split(z[f"{name}_ids"], cuts), normals=np.split(z[f"{name}_normals"], cuts),
                conf=np.split(z[f"{name}_conf"], cuts), t=[w[:3, 3] for w in z[f"{name}_w2c"]],
                unique_ids=z[f"{name}_unique_ids"], fused=z[f"{name}_fused_normals"])


@pytest.mark.parametrize("name", ["coherent", "scattered"])
def test_model_reproduces_reference_normal_fusion(name):
    c = fixture_case(name)
    uids, normals = model.normal_fusion(c["xyz"], c["ids"], c["normals"], c["conf"], c["t"])
    assert np.array_equal(uids, c["unique_ids"])
    nan_ref = np.isnan(c["fused"]).any(axis=1)
    assert np.array_equal(np.isnan(normals).any(axis=1), nan_ref)
    assert (name == "scattered") == bool(nan_ref.any())
    assert np.abs(normals[~nan_ref] - c["fused"][~nan_ref]).max() <= 1e-6


def test_model_statistical_mask_semantics():
    rng = np.random.default_rng(0)
    p = rng.uniform(size=(400, 3))
    p[10] = [50.0, 50.0, 50.0]        # far outlier
    p[20:30] = p[20]                   # ten duplicates: a == 0 at k <= 10
    keep, a, thr = model.statistical_outlier_mask(p, nb_neighbors=8)
    assert not keep[10] and not keep[20:30].any()
    assert np.all(keep == ((a > 0) & (a < thr)))


def test_model_normal_mask_drops_nan_and_keeps_flat():
    rng = np.random.default_rng(1)
    p = np.c_[rng.uniform(size=(300, 2)), np.zeros(300)]
    n = np.tile([0.0, 0.0, 1.0], (300, 1))
    n[5] = [1.0, 0.0, 0.0]
    n[7] = np.nan
    keep, _ = model.normal_outlier_mask(p, n)
    assert not keep[7]
    assert keep.sum() >= 300 - 2 - 2 * 20      # the NaN normal drops every point that has it among its neighbours


def test_open3d_statistical_parity():
    o3d = pytest.importorskip("open3d")
    rng = np.random.default_rng(3)
    p = rng.normal(size=(2000, 3))
    pc = o3d.geometry.PointCloud()
    pc.points = o3d.utility.Vector3dVector(p)
    _, ind = pc.remove_statistical_outlier(nb_neighbors=50, std_ratio=2.0)
    keep, _, _ = model.statistical_outlier_mask(p)
    assert np.array_equal(np.nonzero(keep)[0], np.asarray(ind))


# ---------------------------------------------------------------------------------------------------- the exact kNN
@pytest.mark.parametrize("k", [1, 10, 64])
def test_knn_exact_equals_ckdtree_without_ties(k):
    rng = np.random.default_rng(k)
    p = rng.uniform(-1, 1, size=(3000, 3)).astype(np.float32)
    q = rng.uniform(-1.5, 1.5, size=(700, 3)).astype(np.float32)
    for queries in (None, q):
        d2, idx = model.knn_exact(p, k, queries)
        rd2, ridx = model.knn(p, k, queries)
        assert d2.dtype == np.float64 and idx.dtype == np.int64 and d2.shape == idx.shape == (len(rd2), k)
        assert (np.diff(d2, axis=1) > 0).all(), "the cloud was meant to be tie-free"
        assert np.array_equal(idx, ridx)
        assert np.all(np.abs(d2 - rd2) <= 1e-14 * rd2)      # cKDTree squares a rounded square root


@functools.lru_cache(maxsize=None)
def lattice_reference():
    return model.knn_exact(edge.cloud("lattice"), 64)


@pytest.mark.parametrize("k", [1, 10, 20, 50, 64])
def test_knn_exact_orders_lattice_ties_by_index(k):
    p = edge.cloud("lattice")
    d2, idx = model.knn_exact(p, k)
    d64, idx64 = lattice_reference()
    assert np.array_equal(d2, d64[:, :k]) and np.array_equal(idx, idx64[:, :k]), "a smaller k is a prefix: the order is total"
    rd2, ridx = model.knn(p, k)
    assert np.array_equal(d2, np.round(rd2)), "integer squared distances: the k nearest distances are cKDTree's"
    pd = p.astype(np.float64)
    assert np.array_equal(d2, ((pd[idx] - pd[:, None, :]) ** 2).sum(axis=2))
    lexicographic = (d2[:, 1:] > d2[:, :-1]) | ((d2[:, 1:] == d2[:, :-1]) & (idx[:, 1:] > idx[:, :-1]))
    assert lexicographic.all()
    # no lower index was passed over: every point tied with the k-th distance and left out has a higher index than
    # every tied point that was taken
    for i in range(0, len(p), 97):
        full = ((pd - pd[i]) ** 2).sum(axis=1)
        tied = np.nonzero(full == d2[i, -1])[0]
        taken = idx[i][d2[i] == d2[i, -1]]
        assert np.array_equal(taken, tied[:len(taken)])
        assert (full < d2[i, -1]).sum() == (d2[i] < d2[i, -1]).sum()
    if k >= 10:
        assert not np.array_equal(np.sort(idx, axis=1), np.sort(ridx, axis=1)), "cKDTree's ties were meant to differ"


def test_knn_exact_chunks_queries_and_rejects_bad_k():
    p = edge.cloud("duplicates")
    d2, idx = model.knn_exact(p, 10)                        # 4000 queries: several chunks
    assert (d2 == 0).all()
    groups = {}
    for i, row in enumerate(map(bytes, p)):
        groups.setdefault(row, []).append(i)
    for i in (0, 1, 1234, 3999):
        assert idx[i].tolist() == groups[bytes(p[i])][:10]  # the group's ten lowest indices, the query itself or not
    with pytest.raises(ValueError):
        model.knn_exact(p[:5], 6)
    with pytest.raises(ValueError):
        model.knn_exact(p, 0)


# ------------------------------------------------------------------- the cleaning inputs of the GPU edge tests
def cleaning_events(name, nb):
    """Near-threshold events of the model (knn_exact) on one cleaning input, by the definitions of the large GPU tests:
    |a - thr| <= 1e-9 thr in the statistical test, |angle - pi/4| <= 1e-9 pi/4 in the normal test, the latter on the whole
    cloud and on what the statistical test kept (clean_point_cloud)."""
    p, n = edge.cleaning_cloud(name)
    keep, a, thr = model.statistical_outlier_mask(p, nb, 2.0, knn=model.knn_exact)
    stat = int((np.abs(a - thr) <= 1e-9 * thr).sum())
    _, ang = model.normal_outlier_mask(p, n, nb, knn=model.knn_exact)
    near = int((np.abs(ang - math.pi / 4) <= 1e-9 * math.pi / 4).sum())
    if keep.any():
        _, ang = model.normal_outlier_mask(p[keep], n[keep], 20, knn=model.knn_exact)
        near += int((np.abs(ang - math.pi / 4) <= 1e-9 * math.pi / 4).sum())
    return stat, near, (keep, a, thr)


@pytest.mark.parametrize("name,nb", edge.cleaning_inputs())
def test_cleaning_edge_inputs_have_no_threshold_events(name, nb):
    stat, near, (keep, a, thr) = cleaning_events(name, nb)
    assert near == 0
    if name == "n2" and nb >= 2:
        # two points are each other's only neighbour: a_0 = a_1 = d / 2, their mean (a + a) / 2 = a and every deviation
        # a - a = 0 without any rounding, so thr = a + 2 * 0 = a_i exactly and `a_i < thr` is false in any IEEE
        # arithmetic.  The definition counts both points as events; nothing here depends on a rounding.
        assert stat == 2 and a[0] == a[1] == thr and not keep.any()
    else:
        assert stat == 0


def test_cleaning_edge_inputs_exercise_both_outcomes():
    for name, nb in (("n255", 20), ("n256", 50), ("n257", 20), ("n513", 50)):
        p, n = edge.cleaning_cloud(name)
        keep, _, _ = model.statistical_outlier_mask(p, nb, knn=model.knn_exact)
        assert 0 < keep.sum() < len(p)
        keep, _ = model.normal_outlier_mask(p, n, nb, knn=model.knn_exact)
        assert 0 < keep.sum() < len(p)
    for name in ("identical", "pairs_and_one"):
        p, _ = edge.cleaning_cloud(name)
        keep, a, thr = model.statistical_outlier_mask(p, 2, knn=model.knn_exact)
        assert not keep.any() and math.isnan(thr) and (a > 0).sum() == (name == "pairs_and_one")
    p, n = edge.cleaning_cloud("duplicated_fifth")
    _, idx = model.knn_exact(p, 20)
    assert 150 <= (idx[:, 0] != np.arange(len(p))).sum() <= 200, "the higher index of a pair does not find itself first"
    exact, _ = model.normal_outlier_mask(p, n, 20, knn=model.knn_exact)
    assert 0 < exact.sum() < len(p)
    assert not model.normal_outlier_mask(p, n, 1, knn=model.knn_exact)[0].any()      # k = 1: the mean of nothing


# ---------------------------------------------------------------------------------- argument checks, no device needed
def test_module_rejects_cpu_tensors():
    from gaustudio_amd import pcd_fusion
    with pytest.raises(RuntimeError, match="ROCm"):
        pcd_fusion.knn(torch.zeros(20, 3), 4)
    with pytest.raises(RuntimeError, match="ROCm"):
        pcd_fusion.NormalFusion(torch.zeros(20, 3))
    with pytest.raises(RuntimeError, match="ROCm"):
        pcd_fusion.statistical_outlier_mask(torch.zeros(20, 3))
    with pytest.raises(RuntimeError, match="ROCm"):
        pcd_fusion.clean_point_cloud(torch.zeros(20, 3), torch.zeros(20, 3))


def test_module_shape_dtype_and_k_checks():
    from gaustudio_amd import pcd_fusion
    with pytest.raises(ValueError, match="shape"):
        pcd_fusion.knn(torch.zeros(20, 2), 4)
    with pytest.raises(TypeError):
        pcd_fusion.knn(torch.zeros(20, 3, dtype=torch.int32), 4)
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        pcd_fusion.knn(torch.zeros(20, 3), 0)
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        pcd_fusion.knn(torch.zeros(100, 3), 65)
    with pytest.raises(ValueError, match="at least 10 points"):
        pcd_fusion.knn(torch.zeros(5, 3), 10)
    with pytest.raises(ValueError, match="shape"):
        pcd_fusion.NormalFusion(torch.zeros(20, 4))
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        pcd_fusion.statistical_outlier_mask(torch.zeros(100, 3), nb_neighbors=0)
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        pcd_fusion.normal_outlier_mask(torch.zeros(100, 3), torch.zeros(100, 3), nb_neighbors=65)
    with pytest.raises(ValueError, match="one row per point"):
        pcd_fusion.normal_outlier_mask(torch.zeros(100, 3), torch.zeros(99, 3))
    with pytest.raises(ValueError, match="one row per point"):
        pcd_fusion.clean_point_cloud(torch.zeros(100, 3), torch.zeros(99, 3))


def test_scene_radius_matches_getnerfppnorm():
    from gaustudio_amd import pcd_fusion
    c = np.array([[0.0, 0, 0], [2.0, 0, 0], [0, 2.0, 0]])
    expect = 1.1 * np.max(np.linalg.norm(c - c.mean(axis=0), axis=1))
    assert math.isclose(pcd_fusion.scene_radius(c), expect, rel_tol=1e-15)
