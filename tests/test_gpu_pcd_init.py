"""GPU tests of gaustudio_amd.pcd_init (csrc/gsr_knn.hip gsr_mean_dist3, csrc/gsr_mesh_bake.hip gsr_point_seeds /
gsr_depth_seed_pack) against the numpy model tests/pcd_init_model.py: every comparison is exact (np.array_equal, -inf and NaN
positions included).  Nothing outside the repository is read."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mesh_init_model as mi  # noqa: E402
import pcd_init_model as pim  # noqa: E402
from gaustudio_amd import formats, postprocess  # noqa: E402
from gaustudio_amd import pcd_init as pi  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
FIELDS = ("xyz", "f_dc", "f_rest", "opacity", "scale", "rot")


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(points, **kw):
    """(dist2 float32 numpy, stats) of the device."""
    out, stats = pi.mean_dist2(dev(np.asarray(points, dtype=F32)), return_stats=True, **kw)
    got = out.cpu().numpy()
    assert got.dtype == F32 and got.shape == (len(points),)
    return got, stats


def check(points, **kw):
    got, stats = run(points, **kw)
    want = pim.mean_dist2(points)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {len(want)} values differ from the model"
    assert 0 <= stats["leftovers"] <= len(points) and stats["occupied_cells"] >= 1
    return got, stats


def noisy_sphere(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * (1 + rng.normal(0, 0.01, (n, 1)))).astype(F32)


# ------------------------------------------------------------------------------------------------------------- mean_dist2
@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 255, 256, 257, 4097])
def test_sizes(n):
    """N = 4 and 5 (every point's three neighbours are all or nearly all the others), wave and block tails."""
    check(np.random.default_rng(n).uniform(-1, 1, (n, 3)).astype(F32))


@pytest.mark.parametrize("target", [1, 2, 8, 64])
def test_cell_target_does_not_change_the_result(target):
    check(np.random.default_rng(77).uniform(-1, 1, (1500, 3)).astype(F32), cell_target=target)


def test_all_points_identical():
    """ext == 0: one cell of size 1 with every point on its corner; d3 = 0 is below the distance to the faces of the 27-cell
    cube (one cell), so every lane settles."""
    got, stats = check(np.repeat(F32([[0.5, -2.0, 3.25]]), 70, axis=0))
    assert (got == 0).all() and stats["leftovers"] == 0 and stats["occupied_cells"] == 1


def test_duplicates_fill_one_cell():
    """1000 copies of one point inside a 3000-point cloud: a cell with more than 64 points."""
    rng = np.random.default_rng(5)
    p = rng.uniform(-1, 1, (3000, 3)).astype(F32)
    where = rng.permutation(3000)[:1000]
    p[where] = F32([0.125, 0.25, -0.5])
    got, _ = check(p)
    assert (got[where] == 0).all()


def test_integer_lattice_all_ties():
    g = np.arange(8, dtype=F32)
    got, _ = check(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))
    assert (got == 1).all()


def test_line_and_plane():
    rng = np.random.default_rng(6)
    t = rng.uniform(0, 1, 300).astype(F32)
    check(np.stack([t, F32(2) * t, F32(-1) * t], axis=1))
    uv = rng.uniform(-1, 1, (700, 2)).astype(F32)
    check(np.concatenate([uv, np.full((700, 1), F32(0.75))], axis=1))


def test_large_offset_small_spread():
    rng = np.random.default_rng(7)
    check((1e4 + rng.uniform(0, 1e-3, (1000, 3))).astype(F32))


def test_outlier_goes_through_the_fallback():
    rng = np.random.default_rng(8)
    p = np.concatenate([rng.normal(0, 0.05, (400, 3)), rng.normal(0, 0.05, (400, 3)) + [3, 0, 0], [[400.0, -250.0, 90.0]]]).astype(F32)
    _, stats = check(p)
    assert stats["leftovers"] >= 1


def test_uniform_cloud_settles_in_the_lane_kernel():
    _, stats = check(np.random.default_rng(9).uniform(0, 1, (4096, 3)).astype(F32))
    assert stats["leftovers"] < 4096
    assert stats["shell2_lanes"] >= stats["leftovers"]


def test_50k_noisy_sphere_against_ckdtree_candidates():
    """cKDTree only proposes 8 candidates per point; their float64 distances are recomputed by the contract's formula."""
    from scipy.spatial import cKDTree
    p = noisy_sphere(50000, 10)
    _, cand = cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=8)
    assert (cand == np.arange(len(p))[:, None]).any(axis=1).all()
    want = pim.mean_dist2_candidates(p, cand)
    got, stats = run(p)
    assert np.array_equal(got, want)
    assert stats["leftovers"] < len(p) // 10
    again, _ = run(p)                                     # bit-identical from run to run
    assert np.array_equal(again.view(np.int32), got.view(np.int32))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_raises(bad):
    p = np.random.default_rng(11).uniform(-1, 1, (300, 3)).astype(F32)
    p[123, 1] = bad
    with pytest.raises(ValueError, match="not finite"):
        pi.mean_dist2(dev(p))
    with pytest.raises(ValueError, match="not finite"):
        pi.point_seeds(dev(p))


# ------------------------------------------------------------------------------------------------------------- seeds
def same(cloud, want):
    for k in FIELDS:
        got = getattr(cloud, k).cpu().numpy()
        assert got.dtype == F32 and got.shape == want[k].shape, k
        assert np.array_equal(got, want[k], equal_nan=True), f"{k} differs from the model"


@pytest.fixture(scope="module")
def cloud_inputs():
    rng = np.random.default_rng(12)
    n = 700
    nrm = rng.normal(size=(n, 3)).astype(F32)
    nrm[:6] = F32([[1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 1, 0], [0, 0, -1], [0, 0, 0]])      # the sign() cases, a zero normal
    return dict(xyz=rng.uniform(-1, 1, (n, 3)).astype(F32), rgb=rng.uniform(0, 1, (n, 3)).astype(F32), normals=nrm,
                scale=rng.normal(size=(n, 3)).astype(F32), rot=rng.normal(size=(n, 4)).astype(F32),
                opacity=rng.normal(size=(n, 1)).astype(F32))


def test_point_seeds_defaults_and_normals(cloud_inputs):
    c = cloud_inputs
    same(pi.point_seeds(dev(c["xyz"])), pim.point_seeds(c["xyz"]))
    same(pi.point_seeds(dev(c["xyz"]), rgb=dev(c["rgb"]), normals=dev(c["normals"]), opacity=0.25, sh_degree=1),
         pim.point_seeds(c["xyz"], rgb=c["rgb"], normals=c["normals"], opacity=0.25, sh_degree=1))


def test_point_seeds_takes_a_distance_the_caller_has(cloud_inputs):
    c = cloud_inputs
    d2 = pi.mean_dist2(dev(c["xyz"]))
    assert np.array_equal(d2.cpu().numpy(), pim.mean_dist2(c["xyz"]))
    same(pi.point_seeds(dev(c["xyz"]), normals=dev(c["normals"]), dist2=d2), pim.point_seeds(c["xyz"], normals=c["normals"]))


def test_point_seeds_given_paths_copy_bit_for_bit(cloud_inputs):
    c = dict(cloud_inputs)
    scale, rot, op = c["scale"].copy(), c["rot"].copy(), c["opacity"].copy()
    scale[0], rot[1], op[2] = [-np.inf, np.nan, np.inf], np.nan, -np.inf
    xyz = c["xyz"].copy()
    xyz[3, 0] = np.nan                                    # no kNN with a scale given: the position is only copied
    cloud = pi.point_seeds(dev(xyz), rgb=dev(c["rgb"]), scale=dev(scale), rot=dev(rot), opacity=dev(op), sh_degree=0)
    same(cloud, pim.point_seeds(xyz, rgb=c["rgb"], scale=scale, rot=rot, opacity=op, sh_degree=0))
    for k, a in (("xyz", xyz), ("scale", scale), ("rot", rot), ("opacity", op)):
        assert np.array_equal(getattr(cloud, k).cpu().numpy().view(np.int32), a.view(np.int32)), k
    assert cloud.f_rest.shape == (700, 0, 3)


def test_pcd_init(cloud_inputs, tmp_path):
    c = cloud_inputs
    cloud = pi.pcd_init(dev(c["xyz"]), dev(c["rgb"]), dev(c["normals"]))
    want = pim.pcd_init(c["xyz"], c["rgb"], c["normals"])
    same(cloud, want)
    assert (cloud.opacity.cpu().numpy() == F32(np.log(0.1 / 0.9))).all()
    same(pi.pcd_init(dev(c["xyz"])), pim.pcd_init(c["xyz"]))
    rec = np.zeros(700, dtype=[(k, "f4") for k in ("x", "y", "z", "nx", "ny", "nz")] + [(k, "u1") for k in ("red", "green", "blue")])
    for j, a in enumerate("xyz"):
        rec[a], rec["n" + a] = c["xyz"][:, j], c["normals"][:, j]
    u8 = np.random.default_rng(13).integers(0, 256, (700, 3)).astype(np.uint8)
    rec["red"], rec["green"], rec["blue"] = u8[:, 0], u8[:, 1], u8[:, 2]
    path = str(tmp_path / "cloud.ply")
    formats.write_ply_vertices(path, rec)
    same(pi.pcd_init_from_ply(path, "cuda"), pim.pcd_init(c["xyz"], (u8.astype(np.float64) / 255).astype(F32), c["normals"]))
    out = str(tmp_path / "seeds.ply")
    formats.export_gaussian_ply(out, cloud)
    back = formats.load_gaussian_ply(out)
    for k in ("xyz", "opacity", "scale", "rot"):
        assert np.array_equal(getattr(back, k).numpy(), want[k], equal_nan=True), k


@pytest.mark.parametrize("resolution,radius", [(3, 100.0), (4, [50, 55])])
def test_sky_seeds(resolution, radius):
    cloud = pi.sky_seeds(resolution, radius)
    want = pim.sky_seeds(resolution, radius)
    same(cloud, want)
    shells = len(radius) if isinstance(radius, list) else 1
    assert cloud.num_points == resolution ** 2 * shells
    assert (cloud.f_dc.cpu().numpy() == F32(0.5) / F32(mi.C0)).all() and np.isfinite(cloud.scale.cpu().numpy()).all()


def test_depth_seeds():
    import torch
    rng = np.random.default_rng(14)
    H, W = 7, 5
    frames, packs = [], []
    for j in range(2):
        depth = rng.uniform(0.5, 4, (H, W)).astype(F32)
        depth[2 + j, 3] = 0.0
        img = rng.uniform(0, 1, (H, W, 3)).astype(F32)
        img[0, 0], img[0, 1] = 0.0, 1.0
        fx, fy = 61.5 + j, 60.25
        K = np.array([[fx, 0, W / 2], [0, fy, H / 2], [0, 0, 1]], dtype=F32)
        a = 0.3 + j
        E = np.array([[np.cos(a), 0, np.sin(a), 0.1], [0, 1, 0, -0.2], [-np.sin(a), 0, np.cos(a), 0.5 * j], [0, 0, 0, 1]], dtype=F32)
        frames.append((dev(depth), dev(img), torch.from_numpy(K), torch.from_numpy(E)))
        world = postprocess.depth_to_points(dev(depth), torch.from_numpy(K), torch.from_numpy(E), "world").cpu().numpy()
        packs.append(pim.depth_pack(world, img, depth, fx, fy))
    cloud = pi.depth_seeds(frames)
    want = pim.depth_seeds(packs)
    same(cloud, want)
    scale = cloud.scale.cpu().numpy()
    assert cloud.num_points == 2 * H * W and np.isneginf(scale[2 * W + 3]).all() and np.isneginf(scale[H * W + 3 * W + 3]).all()
    assert np.isneginf(scale).sum() == 6 and (cloud.opacity.cpu().numpy() == 0).all()
    same(pi.depth_seeds(frames[1:], sh_degree=0), pim.depth_seeds(packs[1:], sh_degree=0))


def test_empty_clouds():
    import torch
    e = lambda c: torch.zeros((0, c), dtype=torch.float32, device="cuda")
    cloud = pi.point_seeds(e(3), scale=e(3), sh_degree=2)
    assert cloud.num_points == 0 and cloud.rot.shape == (0, 4) and cloud.f_rest.shape == (0, 8, 3) and cloud.f_dc.shape == (0, 1, 3)
    cloud = pi.point_seeds(e(3), rgb=e(3), scale=e(3), rot=e(4), opacity=e(1))
    assert cloud.num_points == 0 and cloud.opacity.shape == (0, 1)
    d = pi.depth_seeds([(torch.zeros((0, 5), device="cuda"), torch.zeros((0, 5, 3), device="cuda"), np.eye(3), np.eye(4))])
    assert d.num_points == 0 and d.scale.shape == (0, 3)
