"""gs-extract-pcd normal fusion / cleaning: the float64 model against the reference's own normal_fusion (fixture), and
the argument checks of gaustudio_amd.pcd_fusion that need no device."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
