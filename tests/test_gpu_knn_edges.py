"""The HIP kNN and the cleaning masks of gaustudio_amd.pcd_fusion (csrc/gsr_knn.hip) where the hashed grid, the wave-wide
sorted insert, the shell stop rule and the full-scan fallback can go wrong: ties, degenerate clouds, far points, query
edges.  The reference is tests/pcd_fusion_model.knn_exact, brute force in (dist2, index) order: include/gsrast.h promises
that order, so dist2 and idx are compared ARRAY-EQUAL, ties included (cKDTree breaks ties its own way and cannot be the
reference here).  The inputs are those of tests/pcd_edge_cases.py; test_pcd_fusion_model.py shows on the CPU that the
cleaning inputs have no near-threshold event, so the masks are compared for equality as well."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pcd_edge_cases as edge  # noqa: E402
import pcd_fusion_model as model  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KS = (1, 10, 20, 50, 64)


def pcd():
    from gaustudio_amd import pcd_fusion
    return pcd_fusion


def dev(a):
    return torch.from_numpy(a).to(DEV)


@functools.lru_cache(maxsize=None)
def reference(cloud, queries=None):
    """knn_exact at the largest k the cloud allows; a smaller k is a prefix, the order being total."""
    p = edge.cloud(cloud)
    return model.knn_exact(p, min(64, len(p)), None if queries is None else edge.lattice_queries(queries))


def check_exact(cloud, k, queries=None, rows=None):
    p = edge.cloud(cloud)
    q = None if queries is None else edge.lattice_queries(queries)
    rd2, ridx = reference(cloud, queries)
    rd2, ridx = rd2[:, :k], ridx[:, :k]
    if rows is not None:
        q, rd2, ridx = q[rows], rd2[rows], ridx[rows]
    dist2, idx = pcd().knn(dev(p), k, None if q is None else dev(q))
    assert dist2.dtype == torch.float64 and idx.dtype == torch.int64 and dist2.shape == idx.shape == rd2.shape
    D, I = dist2.cpu().numpy(), idx.cpu().numpy()
    wrong = np.nonzero((I != ridx).any(axis=1))[0]
    assert len(wrong) == 0, f"{len(wrong)} queries with other indices, first {wrong[0]}: {I[wrong[0]]} for {ridx[wrong[0]]}"
    assert np.array_equal(D, rd2), "dist2 is not dx*dx + dy*dy + dz*dz in float64, bit for bit"
    return dist2, idx


# ------------------------------------------------------------------------------------------------------------ clouds
@pytest.mark.parametrize("cloud,k", [(c, k) for c in edge.CLOUDS for k in KS if k <= len(edge.cloud(c))])
def test_knn_exact_on_edge_clouds(cloud, k):
    check_exact(cloud, k)


def test_knn_ties_between_the_cell_and_its_neighbours():
    """lattice17_holes at k <= 16 (cell size 2): for a site with odd coordinates the tied candidates at squared distance
    1 lie half inside its cell and half outside, at exactly the distance of the cell's faces.  The k of the parametrised
    test do not stop there: 4 and 7 do."""
    for k in (2, 4, 7):
        check_exact("lattice17_holes", k)


def test_knn_duplicates_return_the_lowest_indices():
    p = edge.cloud("duplicates")
    dist2, idx = check_exact("duplicates", 10)
    assert not bool(dist2.any())
    I = idx.cpu().numpy()
    same = (p[I] == p[:, None, :]).all(axis=2)
    assert same.all()
    assert (I != np.arange(len(p))[:, None]).all(axis=1).sum() > 3000, "most queries are not among their group's lowest ten"
    dist2, _ = check_exact("duplicates", 64)
    D = dist2.cpu().numpy()
    assert (D[:, :50] == 0).all() and (D[:, 50:] > 0).all(), "k = 64 crosses into the next group"


# ----------------------------------------------------------------------------------------------------------- queries
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("queries", edge.LATTICE_QUERIES)
def test_knn_separate_queries_against_the_lattice(queries, k):
    check_exact("lattice", k, queries)


@pytest.mark.parametrize("nq", [1, 3, 4, 5])
def test_knn_query_counts_around_a_block(nq):
    for queries in ("midpoints", "at_1e30"):
        check_exact("lattice", 20, queries, rows=slice(7, 7 + nq))


def test_knn_empty_queries():
    p = dev(edge.cloud("n65"))
    for q in (torch.empty(0, 3, device=DEV), torch.empty(0, 3, device=DEV, dtype=torch.float64), p[:0]):
        dist2, idx = pcd().knn(p, 7, q)
        assert dist2.shape == idx.shape == (0, 7) and dist2.dtype == torch.float64 and idx.dtype == torch.int64
        assert dist2.device == idx.device == p.device
    bad = p.clone()
    bad[5, 0] = float("inf")
    with pytest.raises(ValueError, match="point coordinate is not finite"):     # the points are still checked
        pcd().knn(bad, 7, torch.empty(0, 3, device=DEV))


def test_knn_k_above_n_raises():
    p = dev(edge.cloud("n65"))
    for q in (None, p[:3].clone(), torch.empty(0, 3, device=DEV)):
        with pytest.raises(ValueError, match="at least 64 points"):
            pcd().knn(p[:63], 64, q)
    with pytest.raises(ValueError, match="at least 2 points"):
        pcd().knn(dev(edge.cloud("single")), 2)


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("row,col,nq", [(0, 0, 1), (2, 1, 4), (8, 2, 9)])
def test_knn_rejects_non_finite_queries(value, row, col, nq):
    p = dev(edge.cloud("lattice"))
    q = dev(edge.lattice_queries("midpoints"))[:nq].clone()
    q[row, col] = value
    with pytest.raises(ValueError, match="queries is not finite"):
        pcd().knn(p, 10, q)
    # and the device is left usable: the same call with the coordinate restored
    q[row, col] = 0.5
    dist2, idx = pcd().knn(p, 10, q)
    rd2, ridx = model.knn_exact(edge.cloud("lattice"), 10, q.cpu().numpy())
    assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(dist2.cpu().numpy(), rd2)


def test_knn_error_codes_are_told_apart():
    """The C entry: an invalid argument, a non-finite point and a non-finite query have return codes of their own, and
    the wrapper says "not finite" for the last two only."""
    from gaustudio_amd import _C, _abi, pcd_fusion
    ws = _abi.Workspace(DEV)
    p = dev(edge.cloud("n65"))
    q = p[:5].clone()
    d2 = torch.empty(65 * 4, dtype=torch.float64, device=DEV)
    idx = torch.empty(65 * 4, dtype=torch.int64, device=DEV)

    def call(points, n, queries, nq, k, out=True):
        null = ctypes.c_void_p(0)
        with torch.cuda.device(DEV):
            return _C.lib().gsr_knn(ws.fn, None, _C._ptr(points), ctypes.c_int(n), null if queries is None else _C._ptr(queries),
                                    ctypes.c_int(nq), ctypes.c_int(k), _C._ptr(d2) if out else null,
                                    _C._ptr(idx) if out else null, _C._stream(DEV))

    assert call(p, 65, None, 0, 4) == 0 and call(p, 65, q, 5, 4) == 0 and call(p, 65, q, 0, 4, out=False) == 0
    for args in ((p, 65, q, 5, 0), (p, 65, q, 5, 65), (p, 3, q, 5, 4), (p, 0, q, 5, 1), (p, 65, q, -1, 4)):
        assert call(*args) == -2                             # GSR_ERR_ARG
    assert call(p, 65, q, 5, 4, out=False) == -2             # no outputs for five queries
    bad = p.clone()
    bad[64, 2] = float("nan")
    assert call(bad, 65, None, 0, 4) == -5 and call(bad, 65, q, 5, 4) == -5      # GSR_ERR_NONFINITE
    q[4, 1] = float("nan")
    assert call(p, 65, q, 5, 4) == -6                        # GSR_ERR_NONFINITE_QUERY
    assert call(p, 65, q, 4, 4) == 0                         # the fifth query is not read
    with pytest.raises(RuntimeError, match=r"rc=-2") as e:
        _abi.raise_status(-2, "knn", pcd_fusion._ERRORS)
    assert "finite" not in str(e.value)


# ------------------------------------------------------------------------------------------------------------ layout
def test_knn_layouts_and_streams_give_the_same_tensors():
    p = edge.cloud("lattice_offset")
    q = edge.lattice_queries("midpoints") * np.float32(2.0 ** -7) + np.array([1024.0, -1024.0, 0.5], dtype=np.float32)
    plain = pcd().knn(dev(p), 20, dev(q))
    rd2, ridx = model.knn_exact(p, 20, q)
    assert np.array_equal(plain[1].cpu().numpy(), ridx) and np.array_equal(plain[0].cpu().numpy(), rd2)

    def padded(a):                                           # a [N,4][:, :3] slice
        t = torch.full((len(a), 4), float("nan"), device=DEV)
        t[:, :3] = dev(a)
        return t[:, :3]

    def transposed(a):                                       # a [3,N].T view
        return dev(np.ascontiguousarray(a.T)).t()

    for name, f in (("slice", padded), ("transposed", transposed), ("float64", lambda a: dev(a.astype(np.float64)))):
        assert name == "float64" or not f(p).is_contiguous()
        got = pcd().knn(f(p), 20, f(q))
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]), name
    self_plain = pcd().knn(dev(p), 20)
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        pts, qs = dev(p), dev(q)
        got = pcd().knn(pts, 20, qs)
        got_self = pcd().knn(pts, 20)
    stream.synchronize()
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    assert torch.equal(got_self[0], self_plain[0]) and torch.equal(got_self[1], self_plain[1])


@pytest.mark.parametrize("cloud", ["lattice", "duplicates"])
def test_knn_is_bit_identical_from_run_to_run(cloud):
    p = dev(edge.cloud(cloud))
    a = pcd().knn(p, 64)
    b = pcd().knn(p.clone(), 64)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))


# ---------------------------------------------------------------------------------------------------------- cleaning
@pytest.mark.parametrize("name,nb", edge.cleaning_inputs())
def test_cleaning_masks_equal_the_model(name, nb):
    p, n = edge.cleaning_cloud(name)
    P = pcd()
    keep, a = P.statistical_outlier_mask(dev(p), nb, 2.0, return_distances=True)
    mk, ma, thr = model.statistical_outlier_mask(p, nb, 2.0, knn=model.knn_exact)
    assert np.allclose(a.cpu().numpy(), ma, rtol=1e-12, atol=0)
    assert np.array_equal(keep.cpu().numpy(), mk), "statistical mask"
    if name in ("n1", "n2", "identical", "pairs_and_one") or nb == 1:
        assert not mk.any()                                  # a_i = 0, a NaN threshold, or two points at the threshold
    keep = P.normal_outlier_mask(dev(p), dev(n), nb)
    mk, _ = model.normal_outlier_mask(p, n, nb, knn=model.knn_exact)
    assert np.array_equal(keep.cpu().numpy(), mk), "normal mask"
    if nb == 1 or len(p) == 1:
        assert not mk.any()                                  # k = 1: the mean of no angle is NaN
    kept = P.clean_point_cloud(dev(p), dev(n), nb_neighbors=nb)
    ref = model.clean_point_cloud(p, n, nb_neighbors=nb, knn=model.knn_exact)
    assert kept.dtype == torch.int64 and np.array_equal(kept.cpu().numpy(), ref)


def test_normal_mask_with_duplicates_needs_the_index_order():
    """The duplicated cloud at the default k = 20: the copy with the higher index has the other copy in slot 0, not
    itself, so the mask depends on the tie order."""
    p, n = edge.cleaning_cloud("duplicated_fifth")
    keep = pcd().normal_outlier_mask(dev(p), dev(n)).cpu().numpy()
    exact, _ = model.normal_outlier_mask(p, n, knn=model.knn_exact)
    assert np.array_equal(keep, exact) and 0 < exact.sum() < len(p)
    kept = pcd().clean_point_cloud(dev(p), dev(n), nb_neighbors=20, normal_neighbors=20).cpu().numpy()
    assert np.array_equal(kept, model.clean_point_cloud(p, n, 20, normal_neighbors=20, knn=model.knn_exact))
