"""gs-extract-pcd on the GPU (gaustudio_amd.pcd_fusion over csrc/gsr_knn.hip): exact kNN against scipy's cKDTree,
normal fusion against the reference's own output (tests/golden/py_pcd_fusion.npz) and the float64 model, run-to-run
bit-identity, the grouping's edges (radix passes, sort tiles, the record buffer's growth, degenerate ids, record order),
the outlier masks against the model, and the whole per-view chain on frames rendered by the operator.  The kNN's and the
masks' edge cases, compared exactly: tests/test_gpu_knn_edges.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pcd_fusion_model as model  # noqa: E402
from test_pcd_fusion_model import fixture_case  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def pcd():
    from gaustudio_amd import pcd_fusion
    return pcd_fusion


def exact_d2(p, q, idx):
    """dx*dx + dy*dy + dz*dz in float64 from the float32 coordinates, the kernel's order."""
    nb = p.astype(np.float64)[idx]
    d = nb - q.astype(np.float64)[:, None, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def check_knn(p, k, q=None):
    """Ours against cKDTree: distances within 1e-14 relative; the index sets equal below the k-th distance; the entries
    tied with the k-th distance are free (cKDTree breaks ties its own way)."""
    dist2, idx = pcd().knn(torch.from_numpy(p).to(DEV), k, None if q is None else torch.from_numpy(q).to(DEV))
    D, I = dist2.cpu().numpy(), idx.cpu().numpy()
    qq = p if q is None else q
    rd, ri = cKDTree(p.astype(np.float64)).query(qq.astype(np.float64), k=k)
    rd, ri = rd.reshape(len(qq), k), ri.reshape(len(qq), k)
    assert I.min() >= 0 and I.max() < len(p)
    assert np.array_equal(D, exact_d2(p, qq, I)), "dist2 is not the float64 distance of the returned index"
    assert np.all(np.abs(D - rd * rd) <= 1e-14 * rd * rd), "k-nearest distances differ from cKDTree"
    ordered = (D[:, 1:] > D[:, :-1]) | ((D[:, 1:] == D[:, :-1]) & (I[:, 1:] > I[:, :-1]))
    assert ordered.all(), "not in ascending (dist2, index) order"
    kth = D[:, -1:]
    ours = np.where(D < kth, I, -1)
    theirs = np.where(exact_d2(p, qq, ri) < kth, ri, -1)
    assert np.array_equal(np.sort(ours, axis=1), np.sort(theirs, axis=1)), "index sets differ below the k-th distance"
    return D, I


def point_sets():
    rng = np.random.default_rng(0)
    sets = {"uniform": rng.uniform(size=(20000, 3))}
    d = rng.normal(size=(20000, 3))
    sets["shell"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    c = rng.uniform(size=(50, 3))
    sets["clustered"] = (c[:, None, :] + 1e-4 * rng.normal(size=(50, 400, 3))).reshape(-1, 3)
    dup = rng.uniform(size=(3000, 3))
    sets["duplicates"] = np.concatenate([dup, np.repeat(dup[:1], 5000, axis=0), np.repeat(dup[1:2], 500, axis=0)])
    far = rng.uniform(size=(20000, 3))
    far[123] = [1e4, 1e4, 1e4]
    sets["far_outlier"] = far
    return {n: v.astype(np.float32) for n, v in sets.items()}


@pytest.mark.parametrize("name", ["uniform", "shell", "clustered", "duplicates", "far_outlier"])
@pytest.mark.parametrize("k", [1, 10, 20, 50, 64])
def test_knn_matches_ckdtree(name, k):
    check_knn(point_sets()[name], k)


@pytest.mark.parametrize("n", [1, 10, 64])
def test_knn_n_equals_k(n):
    rng = np.random.default_rng(n)
    check_knn(rng.uniform(size=(n, 3)).astype(np.float32), n)


def test_knn_separate_queries():
    rng = np.random.default_rng(5)
    p = point_sets()["shell"]
    q = rng.uniform(-1.5, 1.5, size=(5000, 3)).astype(np.float32)
    q[0] = [3e3, -2e3, 1e3]            # far from every point
    for k in (1, 10, 50):
        check_knn(p, k, q)


def test_knn_one_million_surface_points():
    rng = np.random.default_rng(6)
    d = rng.normal(size=(1_000_000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = (d * (1.0 + 0.05 * np.sin(5 * d[:, :1]))).astype(np.float32)
    check_knn(p, 10)


def test_knn_rejects_non_finite_points():
    p = torch.zeros(100, 3, device=DEV)
    p[3, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        pcd().knn(p, 4)


# ------------------------------------------------------------------------------------------------------------ fusion
def run_gpu_fusion(c, k=10, consistency=0.8):
    xyz = torch.from_numpy(c["xyz"]).to(DEV)
    return pcd().normal_fusion(xyz, [torch.from_numpy(i).to(DEV) for i in c["ids"]],
                               [torch.from_numpy(n).to(DEV) for n in c["normals"]],
                               [torch.from_numpy(f).to(DEV) for f in c["conf"]], c["t"], k=k, consistency=consistency)


def events(c, consistency=0.8, knn=model.knn, k=10):
    """Unique ids whose fused normal may legitimately differ from a float32 / float64 restatement by more than the
    tolerance, and every fused point that has one of them among its k (10) smoothing neighbours:
      * a record within 1e-5 of the 0.8 consistency threshold (the record is in or out depending on rounding);
      * an id whose consistent records nearly cancel, |S| / W < 1e-3 (normalising amplifies the rounding)."""
    uids, _, _, st = model.fused_means(c["xyz"], c["ids"], c["normals"], c["conf"], c["t"], consistency)
    flagged = np.zeros(len(uids), dtype=bool)
    near = np.abs(st["record_diff"] - consistency) < 1e-5
    flagged[st["inverse"][near]] = True
    flagged |= st["sum_ratio"] < 1e-3
    _, nbr = knn(c["xyz"].astype(np.float64)[uids], k)
    return flagged[nbr].any(axis=1)


def compare_fused(uids, normals, ref_uids, ref_normals, allowed, tol=1e-5, cap=0.01):
    assert np.array_equal(uids.cpu().numpy().astype(np.int64), ref_uids.astype(np.int64))
    n = normals.cpu().numpy()
    nan_ref = np.isnan(ref_normals).any(axis=1)
    assert np.array_equal(np.isnan(n).any(axis=1), nan_ref), "NaN in different places"
    err = np.abs(n - ref_normals).max(axis=1)
    bad = (err > tol) & ~nan_ref
    assert allowed.sum() <= max(5, cap * len(n)), f"{allowed.sum()} threshold events: more than the cap"
    assert not (bad & ~allowed).any(), f"{int((bad & ~allowed).sum())} normals off by > {tol} outside the named events"


@pytest.mark.parametrize("name", ["coherent", "scattered"])
def test_fusion_matches_reference_fixture(name):
    c = fixture_case(name)
    uids, normals = run_gpu_fusion(c)
    compare_fused(uids, normals, c["unique_ids"], c["fused"], events(c))


def big_case(seed=7, P=200_000, views=50, per_view=100_000):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(P, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    xyz = (d * (1.0 + 0.05 * np.sin(4 * d[:, :1]))).astype(np.float32)
    ids, nrm, conf, t = [], [], [], []
    for v in range(views):
        i = rng.integers(0, P, size=per_view).astype(np.int32)
        n = d[i] + 0.3 * rng.normal(size=(per_view, 3))
        scatter = rng.uniform(size=per_view) < 0.05
        n[scatter] = rng.normal(size=(int(scatter.sum()), 3))
        ids.append(i)
        nrm.append((n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32))
        conf.append(rng.uniform(0.5, 1.0, size=per_view).astype(np.float32))
        a = 2 * math.pi * v / views
        t.append(np.array([3 * math.cos(a), 0.5 * math.sin(3 * a), 3 * math.sin(a)], dtype=np.float32))
    return dict(xyz=xyz, ids=ids, normals=nrm, conf=conf, t=t)


def test_fusion_matches_model_at_scale_and_is_bit_identical():
    c = big_case()
    u1, n1 = run_gpu_fusion(c)
    u2, n2 = run_gpu_fusion(c)
    assert torch.equal(u1, u2)
    assert torch.equal(n1.view(torch.int32), n2.view(torch.int32)), "two runs differ"
    ref_u, ref_n = model.normal_fusion(c["xyz"], c["ids"], c["normals"], c["conf"], c["t"])
    assert len(ref_u) > 150_000
    compare_fused(u1, n1, ref_u, ref_n, events(c))


def test_fusion_errors():
    P = pcd()
    xyz = torch.rand(100, 3, device=DEV)
    f = P.NormalFusion(xyz)
    f.add_view(torch.arange(5, device=DEV, dtype=torch.int32), torch.rand(5, 3, device=DEV), torch.ones(5, device=DEV), [3, 0, 0])
    with pytest.raises(ValueError, match="at least k = 10"):
        f.finalize()
    f.add_view(torch.tensor([100], device=DEV, dtype=torch.int32), torch.rand(1, 3, device=DEV), torch.ones(1, device=DEV), [3, 0, 0])
    with pytest.raises(ValueError, match="outside"):
        f.finalize(k=2)


# ------------------------------------------------------------------------------------------- fusion: grouping edges
def small_case(P, counts, seed, distinct=400, int64=False):
    """`counts` records per view over at most `distinct` ids of [0, P), ids 0 and P - 1 among them, and 20 ids with a
    single record; every id has a direction of its own, its records scatter around it (a few far enough to fail the
    consistency test)."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1, 1, size=(P, 3)).astype(np.float32)
    pool = np.unique(np.concatenate([[0, P - 1], rng.integers(0, P, size=min(distinct, P))]))
    singles = rng.permutation(np.setdiff1d(np.arange(min(P, 1 << 17)), pool))[:20]     # ids with exactly one record
    axis = rng.normal(size=(P, 3)) if P <= 1 << 12 else None
    ids, nrm, conf, t = [], [], [], []
    for v, m in enumerate(counts):
        i = rng.choice(pool, size=m)
        if v == 0:                                                     # every id of the pool at least once
            first = np.concatenate([rng.permutation(pool), singles])[:m]
            i[:len(first)] = first
            i = rng.permutation(i)
        base = axis[i] if axis is not None else np.stack([np.sin(i * 0.7), np.cos(i * 1.3), np.sin(i * 0.37 + 1)], axis=1)
        n = base / np.linalg.norm(base, axis=1, keepdims=True) + 0.25 * rng.normal(size=(m, 3))
        wild = rng.uniform(size=m) < 0.05
        n[wild] = rng.normal(size=(int(wild.sum()), 3))
        ids.append(i.astype(np.int64 if int64 else np.int32))
        nrm.append((n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32))
        conf.append(rng.uniform(0.5, 1.0, size=m).astype(np.float32))
        t.append(np.array([3.0 * math.cos(v), 0.5, 3.0 * math.sin(v)], dtype=np.float32))
    return dict(xyz=xyz, ids=ids, normals=nrm, conf=conf, t=t)


def check_small_case(c, k=10):
    uids, normals = run_gpu_fusion(c, k=k)
    ref_u, ref_n = model.normal_fusion(c["xyz"], c["ids"], c["normals"], c["conf"], c["t"], k=k, knn=model.knn_exact)
    compare_fused(uids, normals, ref_u, ref_n, events(c, knn=model.knn_exact, k=k))
    return uids, normals, ref_n


# the radix sort runs ceil(bits(num_gaussians - 1) / 8) passes over 4096-key tiles: both sides of 2^8 and 2^16 Gaussians,
# and of one tile of records
@pytest.mark.parametrize("P,records,k", [(2, 300, 2), (256, 4095, 10), (257, 4096, 10), (65536, 4097, 10), (65537, 4096, 10),
                                         (257, 1, 1)])
def test_fusion_grouping_sizes(P, records, k):
    c = small_case(P, [records], seed=P + records + (1000 if P == 257 and records == 4096 else 0))   # seeds without events
    uids, _, _ = check_small_case(c, k)
    u = uids.cpu().numpy()
    if records > 1:
        assert u[0] == 0 and u[-1] == P - 1
    counts = np.bincount(c["ids"][0], minlength=P)
    assert records == 1 or P == 2 or ((counts == 1).any() and (counts > 8).any()), "ids with one record and with many"


def test_fusion_record_buffer_grows_across_views():
    """Three views carry the record buffer across its first 65536 records (and the second one across a tile edge), with
    int64 ids."""
    c = small_case(5000, [40000, 25536 + 1, 30000], seed=3, distinct=1500, int64=True)
    f = pcd().NormalFusion(torch.from_numpy(c["xyz"]).to(DEV))
    sizes = []
    for i, n, w, t in zip(c["ids"], c["normals"], c["conf"], c["t"]):
        f.add_view(torch.from_numpy(i).to(DEV), torch.from_numpy(n).to(DEV), torch.from_numpy(w).to(DEV), t)
        sizes.append(f.records.shape[0])
    assert sizes[0] == 1 << 16 and sizes[1] > 1 << 16 and f.num_records == 95537
    uids, normals = f.finalize()
    ref_u, ref_n = model.normal_fusion(c["xyz"], c["ids"], c["normals"], c["conf"], c["t"], knn=model.knn_exact)
    compare_fused(uids, normals, ref_u, ref_n, events(c, knn=model.knn_exact))
    assert uids.dtype == torch.int32


def test_fusion_degenerate_ids_poison_their_neighbours_only():
    """An id whose weights are all zero (0 / 0 in the first mean) and an id with two opposite normals of equal weight
    (mean 0, no record within 0.8 of it) fuse to NaN; the smoothing spreads the NaN to exactly the points that have
    one of them among their 10 nearest, as the model says."""
    c = small_case(3000, [4000, 3000], seed=5, distinct=600)
    pool = np.unique(np.concatenate(c["ids"]))
    zero_w, opposite = int(pool[len(pool) // 3]), int(pool[2 * len(pool) // 3])
    for v in range(2):
        c["conf"][v][c["ids"][v] == zero_w] = 0.0
        keep = c["ids"][v] != opposite
        c["ids"][v], c["normals"][v], c["conf"][v] = c["ids"][v][keep], c["normals"][v][keep], c["conf"][v][keep]
    n = np.array([[0.6, 0.0, 0.8]], dtype=np.float32)
    c["ids"][1] = np.concatenate([c["ids"][1][:1000], [opposite], c["ids"][1][1000:], [opposite]]).astype(np.int32)
    c["normals"][1] = np.concatenate([c["normals"][1][:1000], n, c["normals"][1][1000:], -n])
    c["conf"][1] = np.concatenate([c["conf"][1][:1000], [0.75], c["conf"][1][1000:], [0.75]]).astype(np.float32)
    uids, normals, ref_n = check_small_case(c)              # compare_fused: NaN in the same places
    u = uids.cpu().numpy()
    nan = np.isnan(normals.cpu().numpy()).any(axis=1)
    sources = np.isin(u, [zero_w, opposite])
    _, nbr = model.knn_exact(c["xyz"][u], 10)
    assert sources.sum() == 2 and nan[sources].all()
    assert np.array_equal(nan, sources[nbr].any(axis=1)) and 2 < nan.sum() <= 40
    assert np.array_equal(nan, np.isnan(ref_n).any(axis=1))


def sequential_fusion(records, consistency):
    """extract_pcd.py:130-181 for one id at k = 1, its records [(normal, weight)] summed one after the other in float64
    (the 1e-12 floor under both means' norms included: with weights of 2^60 it is what the means are divided by)."""
    def mean(rs):
        s, w = np.zeros(3), 0.0
        for n, wt in rs:
            s = s + np.asarray(n, dtype=np.float64) * wt
            w = w + wt
        with np.errstate(invalid="ignore", divide="ignore"):
            m = s / w
        return m / max(math.sqrt(float((m * m).sum())), 1e-12)
    m1 = mean(records)
    m2 = mean([(n, w) for n, w in records if math.sqrt(float(((np.asarray(n, dtype=np.float64) - m1) ** 2).sum())) < consistency])
    f = m2.astype(np.float32)                                # k = 1 smoothing: the mean itself, F.normalize in float32
    return f / max(np.sqrt((f * f).sum(dtype=np.float32)), np.float32(1e-12))


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (0, 2, 1, 3), (1, 0, 2, 3), (3, 2, 1, 0), (2, 3, 0, 1)])
def test_fusion_sums_an_ids_records_in_record_order(order):
    """The stable sort, observed: four records of one id whose float64 sum depends on the order (2^60 + 1 - 2^60 is 0 or
    1), spread over four 4096-key tiles among 13000 records of other ids.  In the order r1 r2 r3 r4 the x-sum is exactly
    0 and the result (0, 1, 0); with r2 after r3 it is (0.707, 0.707, 0)."""
    big = 2.0 ** 60
    four = [((1.0, 0.0, 0.0), big), ((1.0, 0.0, 0.0), 1.0), ((-1.0, 0.0, 0.0), big), ((0.0, 1.0, 0.0), 1.0)]
    four = [four[j] for j in order]
    rng = np.random.default_rng(8)
    P, special, n = 1000, 517, 13000
    ids = rng.integers(0, P, size=n).astype(np.int32)
    ids[ids == special] = special + 1
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    w = rng.uniform(0.1, 1.0, size=n).astype(np.float32)
    at = [5, 4100, 8200, 12300]                              # one position in each of the four tiles
    for pos, (normal, weight) in zip(at, four):
        ids[pos], nrm[pos], w[pos] = special, normal, weight
    rec = np.empty((n, 5), dtype=np.int32)
    rec[:, 0] = ids
    rec[:, 1:4] = nrm.view(np.int32)
    rec[:, 4] = w.view(np.int32)
    f = pcd().NormalFusion(torch.from_numpy(rng.uniform(size=(P, 3)).astype(np.float32)).to(DEV))
    f.records[:n] = torch.from_numpy(rec).to(DEV)
    f.num_records = n
    uids, normals = f.finalize(k=1, consistency=10.0)       # k = 1: the smoothing returns the id's own mean
    u = uids.cpu().numpy()
    assert np.array_equal(u, np.unique(ids))
    got = normals.cpu().numpy()
    expect = sequential_fusion(four, 10.0)
    assert np.abs(expect).max() > 0.7 and (order != (0, 1, 2, 3) or np.array_equal(expect, [0.0, 1.0, 0.0]))
    # float32 output of a float64 computation: 2^-24 relative per component, twice (mean, then the smoothing's normalize)
    assert np.abs(got[u == special][0] - expect).max() <= 4 * 2.0 ** -24, (got[u == special][0], expect)
    for j in (0, 1, len(u) - 1):                             # and three other ids, their records in record order as well
        sel = ids == u[j]
        e = sequential_fusion(list(zip(nrm[sel].astype(np.float64), w[sel].astype(np.float64))), 10.0)
        assert np.abs(got[j] - e).max() <= 4 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------ cleaning
def cloud(seed=11, n=60_000):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = d * (1.0 + 0.003 * rng.normal(size=(n, 1)))
    out = rng.uniform(size=n) < 0.02
    p[out] += 0.2 * rng.normal(size=(int(out.sum()), 3))
    nrm = d + 0.2 * rng.normal(size=(n, 3))
    flip = rng.uniform(size=n) < 0.05
    nrm[flip] = rng.normal(size=(int(flip.sum()), 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return p.astype(np.float32), nrm.astype(np.float32)


def test_statistical_mask_matches_model():
    p, _ = cloud()
    for k, ratio in ((50, 2.0), (20, 1.0)):
        keep, a = pcd().statistical_outlier_mask(torch.from_numpy(p).to(DEV), k, ratio, return_distances=True)
        mk, ma, thr = model.statistical_outlier_mask(p, k, ratio)
        assert np.allclose(a.cpu().numpy(), ma, rtol=1e-12, atol=0)
        near = np.abs(ma - thr) <= 1e-9 * thr
        diff = keep.cpu().numpy() != mk
        assert near.sum() <= 5 and not (diff & ~near).any(), (int(diff.sum()), int(near.sum()))
        assert 0 < (~mk).sum() < 0.2 * len(p)


def test_normal_mask_matches_model():
    p, n = cloud(12)
    keep = pcd().normal_outlier_mask(torch.from_numpy(p).to(DEV), torch.from_numpy(n).to(DEV))
    mk, ang = model.normal_outlier_mask(p, n)
    near = np.abs(ang - math.pi / 4) <= 1e-9 * math.pi / 4
    diff = keep.cpu().numpy() != mk
    assert near.sum() <= 5 and not (diff & ~near).any(), (int(diff.sum()), int(near.sum()))
    assert 0 < (~mk).sum() < len(p)


def test_clean_point_cloud_matches_model():
    p, n = cloud(13, 30_000)
    kept = pcd().clean_point_cloud(torch.from_numpy(p).to(DEV), torch.from_numpy(n).to(DEV)).cpu().numpy()
    ref = model.clean_point_cloud(p, n)
    assert np.all(np.diff(kept) > 0)
    assert len(np.setxor1d(kept, ref)) <= 5


# ------------------------------------------------------------------------------------------------------------ end to end
def render_views(P=30_000, views=8, W=192, H=144):
    from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, scenes
    from gaustudio_amd import postprocess as pp
    g = torch.Generator().manual_seed(3)
    d = torch.randn(P, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    xyz = (d * (1.0 + 0.08 * torch.sin(5 * d[:, 0:1]))).to(DEV)
    shs = torch.zeros(P, 16, 3, device=DEV)
    out = []
    for cam in scenes.ring_cameras(views, W, H, radius=3.2, elevation=0.35):
        rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0,
                                           cam.viewmatrix.to(DEV), cam.projmatrix.to(DEV), 0, cam.campos.to(DEV), False, False)
        with torch.no_grad():
            _, _, depth, median, opacity = GaussianRasterizer(rs)(
                means3D=xyz, means2D=torch.zeros_like(xyz), opacities=torch.full((P, 1), 0.95, device=DEV), shs=shs,
                scales=torch.full((P, 3), 0.012, device=DEV), rotations=torch.tensor([[1.0, 0, 0, 0]], device=DEV).repeat(P, 1))
        f = cam.width / (2 * cam.tanfovx)
        K = torch.tensor([[f, 0, cam.width / 2], [0, f, cam.height / 2], [0, 0, 1]])
        w2c = cam.viewmatrix.t().contiguous()
        filtered, fg = pp.masked_bilateral_filter(depth[0], opacity[0] > 0.1)
        cam_n = pp.depth_to_normals(filtered, K)
        cam_n[~fg] = -1
        world_n = cam_n @ w2c[:3, :3].to(DEV).inverse().t()
        out.append((median, opacity, world_n, w2c, cam.campos))
    return xyz, out


def test_end_to_end_rendered_views_match_model():
    P = pcd()
    xyz, views = render_views()
    radius = P.scene_radius(torch.stack([v[4] for v in views]))
    fusion = P.NormalFusion(xyz)
    m_ids, m_nrm, m_conf, m_t = [], [], [], []
    for median, opacity, world_n, w2c, _ in views:
        ids, nrm, conf = P.view_records(median, opacity, world_n, radius)
        fusion.add_view(ids, nrm, conf, w2c[:3, 3])
        a, b, c = model.view_records(median.cpu().numpy(), opacity.cpu().numpy(), world_n.cpu().numpy(), radius)
        assert np.array_equal(a, ids.cpu().numpy()) and np.array_equal(b, nrm.cpu().numpy())
        m_ids.append(a); m_nrm.append(b); m_conf.append(c); m_t.append(w2c[:3, 3].numpy())
    uids, normals = fusion.finalize()
    c = dict(xyz=xyz.cpu().numpy(), ids=m_ids, normals=m_nrm, conf=m_conf, t=m_t)
    ref_u, ref_n = model.normal_fusion(c["xyz"], m_ids, m_nrm, m_conf, m_t)
    compare_fused(uids, normals, ref_u, ref_n, events(c))
    pts = xyz[uids.long()]
    ok = ~torch.isnan(normals).any(dim=1)
    outward = (normals[ok] * pts[ok]).sum(dim=1) > 0
    assert outward.float().mean() > 0.9, "fused normals do not point outward on the shell"
    kept = P.clean_point_cloud(pts, normals).cpu().numpy()
    # the same cleaning of the same fused cloud: differences only at the thresholds
    same = model.clean_point_cloud(pts.cpu().numpy(), normals.cpu().numpy().astype(np.float64))
    assert len(np.setxor1d(kept, same)) <= 5
    # the model's whole chain: its fused normals differ by <= 1e-5, which moves points that sit at the pi/4 angle test
    ref_kept = model.clean_point_cloud(pts.cpu().numpy(), ref_n)
    assert len(np.setxor1d(kept, ref_kept)) <= max(5, len(ref_kept) // 200)
