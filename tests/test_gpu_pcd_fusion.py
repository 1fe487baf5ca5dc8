"""gs-extract-pcd on the GPU (gaustudio_amd.pcd_fusion over csrc/gsr_knn.hip): exact kNN against scipy's cKDTree,
normal fusion against the reference's own output (tests/golden/py_pcd_fusion.npz) and the float64 model, run-to-run
bit-identity, the outlier masks against the model, and the whole per-view chain on frames rendered by the operator."""
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
def run_gpu_fusion(c, k=10):
    xyz = torch.from_numpy(c["xyz"]).to(DEV)
    return pcd().normal_fusion(xyz, [torch.from_numpy(i).to(DEV) for i in c["ids"]],
                               [torch.from_numpy(n).to(DEV) for n in c["normals"]],
                               [torch.from_numpy(f).to(DEV) for f in c["conf"]], c["t"], k=k)


def events(c, consistency=0.8):
    """Unique ids whose fused normal may legitimately differ from a float32 / float64 restatement by more than the
    tolerance, and every fused point that has one of them among its 10 smoothing neighbours:
      * a record within 1e-5 of the 0.8 consistency threshold (the record is in or out depending on rounding);
      * an id whose consistent records nearly cancel, |S| / W < 1e-3 (normalising amplifies the rounding)."""
    uids, _, _, st = model.fused_means(c["xyz"], c["ids"], c["normals"], c["conf"], c["t"], consistency)
    flagged = np.zeros(len(uids), dtype=bool)
    near = np.abs(st["record_diff"] - consistency) < 1e-5
    flagged[st["inverse"][near]] = True
    flagged |= st["sum_ratio"] < 1e-3
    _, nbr = model.knn(c["xyz"].astype(np.float64)[uids], 10)
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
