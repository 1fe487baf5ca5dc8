"""GPU tests of gaustudio_amd.visual_hull (csrc/gsr_hull.hip) against the float32 model tests/visual_hull_model.py.  Every
comparison with the model is exact (np.array_equal): packed mask words, filled, count and carved_by -- the library is built
without contraction and with a correctly rounded divide, and the model performs the kernel's operations in their order."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import visual_hull_model as vm  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def _torch():
    import torch
    return torch


def to_dev(masks, dtype=None):
    t = _torch()
    return [None if m is None else t.from_numpy(np.ascontiguousarray(m if dtype is None else m.astype(dtype))).cuda() for m in masks]


def gpu_carve(axes, cameras, masks, dtype=None):
    from gaustudio_amd import visual_hull as vh
    filled, count, carved_by = vh.carve_axes(cameras, to_dev(masks, dtype), axes, return_carved_by=True)
    assert filled.dtype == _torch().bool and carved_by.dtype == _torch().int32
    return filled.cpu().numpy(), count, carved_by.cpu().numpy()


def assert_same_carve(axes, cameras, masks, dtype=None):
    got = gpu_carve(axes, cameras, masks, dtype)
    want = vm.carve(axes, cameras, masks)
    assert got[0].shape == want[0].shape
    assert np.array_equal(got[0], want[0]), f"filled differs on {(got[0] != want[0]).sum()} voxels"
    assert got[1] == want[1] == int(want[0].sum())
    assert np.array_equal(got[2], want[2]), "carved_by differs"
    return want


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "py_visual_hull.npz")))


def fixture_scene(fx):
    W, H = (int(v) for v in fx["size"])
    cameras = [(M, W, H) for M in fx["matrices"]]
    masks = [m if h else None for m, h in zip(fx["masks"], fx["has_mask"])]
    return (fx["axis_x"], fx["axis_y"], fx["axis_z"]), cameras, masks


@pytest.fixture(scope="module")
def ring():
    """6 ring cameras, 64 x 48, disc masks of a sphere of radius 0.5 around the origin."""
    return vm.ring_scene(6, 64, 48, distance=3.0, fov_deg=40.0, disc=0.5, seed=1)


def lin_axes(r0, r1, r2, half=0.8):
    """(x [r1], y [r0], z [r2]) with slightly different, non-symmetric extents per axis."""
    return (np.linspace(-half, half * 1.05, r1).astype(F), np.linspace(-half * 0.9, half, r0).astype(F),
            np.linspace(-half * 1.1, half * 0.95, r2).astype(F))


# ---------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("shape", [(29, 37), (1, 64), (70, 1)], ids=["37x29", "64x1", "1x70"])      # [H, W]
@pytest.mark.parametrize("dtype", ["uint8", "bool", "float32"])
def test_pack_masks_equals_model(shape, dtype):
    from gaustudio_amd import visual_hull as vh
    t = _torch()
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    a = rng.random(shape) < 0.5
    b = rng.random(shape) < 0.3
    if dtype == "float32":
        ma, mb = (a * rng.uniform(-2, 2, shape)).astype(F), b.astype(F)
        ma[0, 0] = np.nan                                               # nonzero, like .bool()
        ma[-1, -1] = -0.0
    else:
        ma, mb = a.astype(dtype), b.astype(dtype)
        if dtype == "uint8":
            ma = ma * np.uint8(200)
    words, layout = vh.pack_masks([t.from_numpy(ma).cuda(), None, t.from_numpy(mb).cuda()])
    wa, sa = vm.pack_bits(ma)
    wb, sb = vm.pack_bits(mb)
    assert layout == [(0, sa), None, (len(wa), sb)] and words.dtype == t.int32 and words.numel() == len(wa) + len(wb)
    got = words.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:len(wa)], wa) and np.array_equal(got[len(wa):], wb)


# ---------------------------------------------------------------------------------------------- carve against the model
def test_fixture_scene_equals_model_and_reference(fx):
    axes, cameras, masks = fixture_scene(fx)
    filled, count, _ = assert_same_carve(axes, cameras, masks)
    # the model equals the reference on this fixture (tests/test_visual_hull_model.py; fixture meta: 0 differing decisions)
    assert np.array_equal(filled.ravel(), fx["filled"]) and count == int(fx["filled"].sum()) > 0


def test_carve_through_camera_records(fx):
    """The public entry: CameraRecords, default translate / radius from camera_normalization, float masks."""
    from gaustudio_amd import carve, formats
    W, H = (int(v) for v in fx["size"])
    recs = [formats.CameraRecord(id=n, image_name=str(n), image_width=W, image_height=H, R=R, T=T, FoVx=float(f[0]), FoVy=float(f[1]))
            for n, (R, T, f) in enumerate(zip(fx["cam_R"], fx["cam_T"], fx["cam_fov"]))]
    masks = [m if h else None for m, h in zip(fx["masks"], fx["has_mask"])]
    hull = carve(recs, to_dev(masks, F), resolution=int(fx["resolution"]), return_carved_by=True)
    assert hull.filled.shape == (24, 24, 24) and np.array_equal(hull.filled.cpu().numpy().ravel(), fx["filled"])
    assert hull.count == int(fx["filled"].sum()) and hull.radius == float(fx["radius"])
    assert all(np.array_equal(a, fx[n]) for a, n in zip(hull.axes, ("axis_x", "axis_y", "axis_z")))
    assert np.array_equal((hull.carved_by == -1).cpu().numpy(), hull.filled.cpu().numpy())


@pytest.mark.parametrize("res", [(5, 7, 67), (33, 33, 33)], ids=["5x7x67", "33^3"])
def test_wave_tails_on_every_axis(ring, res):
    cameras, masks = ring
    filled, count, _ = assert_same_carve(lin_axes(*res), cameras, masks)
    assert 0 < count < filled.size


@pytest.mark.parametrize("ncam", [1, 70])
def test_camera_counts(ncam):
    cameras, masks = vm.ring_scene(ncam, 40, 30, distance=3.0, fov_deg=40.0, disc=0.5, seed=ncam)
    filled, count, carved_by = assert_same_carve(lin_axes(20, 21, 22), cameras, masks)
    assert 0 < count < filled.size
    if ncam == 70:
        assert carved_by.max() > 32                                     # late cameras of the table decide voxels too


def test_all_carved_by_the_first_camera(ring):
    """Early exit: a mask of zeros carves every voxel at camera 0; no wave walks the rest of the table."""
    cameras, masks = ring
    masks = [np.zeros_like(masks[0])] + list(masks[1:])
    filled, count, carved_by = assert_same_carve(lin_axes(17, 18, 19), cameras, masks)
    assert count == 0 and not filled.any() and (carved_by == 0).all()


def test_all_kept_and_no_mask(ring):
    cameras, masks = ring
    axes = lin_axes(9, 10, 70, half=0.2)                                # well inside every view
    full = [np.ones_like(m) for m in masks]
    filled, count, carved_by = assert_same_carve(axes, cameras, full)
    assert filled.all() and count == filled.size and (carved_by == -1).all()
    filled2, count2, _ = assert_same_carve(axes, cameras, [None] * len(cameras))     # no mask at all: no packed words
    assert filled2.all()
    mixed = [masks[0], None, masks[2], None, None, masks[5]]
    filled3, count3, _ = assert_same_carve(lin_axes(12, 13, 14), cameras, mixed)
    assert 0 < count3 < filled3.size


def test_identity_boundary_cases():
    """ndc = 1 reads pixel W - 1, ndc = -1 pixel 0, z = 0 is not in front, w < 0, w = 0 (tests/test_visual_hull_model.py)."""
    t = np.array([-1.0, 0.0, 1.0], dtype=F)
    axes = (t, t, t)
    rng = np.random.default_rng(3)
    col, row = [0, 2, 3], [0, 1, 2]
    for M in (np.eye(4, dtype=F), np.diag([1, 1, 1, -1]).astype(F), np.diag([1, 1, 1, 0]).astype(F)):
        for trial in range(3):
            mask = rng.integers(0, 2, (3, 4)).astype(np.uint8)
            filled, _, _ = assert_same_carve(axes, [(M, 4, 3)], [mask])
            assert not filled[:, :, :2].any()
            if M[3, 3] == 1:
                assert all(filled[i, j, 2] == bool(mask[row[i], col[j]]) for i in range(3) for j in range(3))
            if M[3, 3] == 0:
                assert not filled.any()


def test_permutation_and_repeat_are_bit_identical(ring):
    cameras, masks = ring
    axes = lin_axes(21, 22, 23)
    a = gpu_carve(axes, cameras, masks)
    b = gpu_carve(axes, cameras, masks)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    perm = [4, 0, 5, 2, 1, 3]
    c = gpu_carve(axes, [cameras[p] for p in perm], [masks[p] for p in perm])
    assert np.array_equal(a[0], c[0]) and a[1] == c[1]
    assert 0 < a[1] < a[0].size


# ---------------------------------------------------------------------------------------------- mesh and seeds
@pytest.fixture(scope="module")
def sphere_hull():
    from gaustudio_amd import carve
    cameras, masks = vm.ring_scene(6, 64, 48, distance=3.0, fov_deg=40.0, disc=0.5, elevation=0.6, seed=2)
    return carve(cameras, to_dev(masks), resolution=32, translate=np.array([0.05, -0.02, 0.03]), radius=0.9)


def test_extract_mesh_geometry(sphere_hull):
    t = _torch()
    hull = sphere_hull
    filled = hull.filled.cpu().numpy()
    assert hull.count > 100 and not (filled[0].any() or filled[-1].any() or filled[:, 0].any() or filled[:, -1].any()
                                     or filled[:, :, 0].any() or filled[:, :, -1].any())     # the hull does not touch the boundary
    v, f = hull.extract_mesh()
    assert v.dtype == t.float32 and f.dtype == t.int32 and v.is_cuda and f.is_cuda and v.shape[1] == 3 and f.shape[1] == 3
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert len(f) > 0 and f.min() >= 0 and f.max() < len(v) and len(np.unique(f)) == len(v)
    assert set(vm.edge_counts(f).tolist()) == {2}                       # closed: every edge is shared by exactly two faces
    assert vm.signed_volume(v + hull.translate, f) > 0                  # normals point away from the filled region
    # back to index units: every coordinate a multiple of 0.5 (binary volume, level 0.5), and x <-> j, y <-> i
    R = hull.resolution
    idx = (v.astype(np.float64) + hull.translate + hull.radius) / (2 * hull.radius) * (R - 1)
    assert np.abs(idx * 2 - np.round(idx * 2)).max() < 1e-3
    half = np.round(idx * 2).astype(int)
    assert ((half % 2).sum(axis=1) == 1).all()                          # a vertex sits on the midpoint of one grid edge
    lo, hi = half // 2, (half + 1) // 2
    a, b = filled[lo[:, 1], lo[:, 0], lo[:, 2]], filled[hi[:, 1], hi[:, 0], hi[:, 2]]
    assert (a != b).all()                                               # ... whose two ends differ
    # the signed volume is the volume of the marching cubes surface around `count` voxels
    cell = (2 * hull.radius / (R - 1)) ** 3
    assert 0.5 * hull.count * cell < vm.signed_volume(v + hull.translate, f) < 1.5 * hull.count * cell


def test_empty_hull_gives_empty_mesh_and_seeds(ring):
    from gaustudio_amd import carve
    cameras, masks = ring
    hull = carve(cameras, to_dev([np.zeros_like(m) for m in masks]), resolution=8, translate=np.zeros(3), radius=0.5)
    v, f = hull.extract_mesh()
    assert hull.count == 0 and tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)
    assert v.dtype == _torch().float32 and f.dtype == _torch().int32
    assert hull.seeds().num_points == 0


def test_seeds_roundtrip_and_render(sphere_hull, tmp_path):
    t = _torch()
    from gaustudio_amd import formats, scenes, visual_hull_init
    from gaustudio_diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    v, _ = sphere_hull.extract_mesh()
    cloud = sphere_hull.seeds(sh_degree=3)
    P = v.shape[0]
    assert cloud.num_points == P and t.equal(cloud.xyz, v)
    for name, shape, value in (("f_dc", (P, 1, 3), 0.0), ("f_rest", (P, 15, 3), 0.0), ("opacity", (P, 1), 0.1), ("scale", (P, 3), 0.01)):
        x = getattr(cloud, name)
        assert x.dtype == t.float32 and tuple(x.shape) == shape and (x == value).all() and x.is_cuda, name
    assert cloud.rot.dtype == t.float32 and t.equal(cloud.rot, t.tensor([1.0, 0, 0, 0], device="cuda").expand(P, 4))
    path = str(tmp_path / "seeds.ply")
    formats.export_gaussian_ply(path, cloud)
    back = formats.load_gaussian_ply(path, device="cuda")
    for name in ("xyz", "f_dc", "f_rest", "opacity", "scale", "rot"):
        assert t.equal(getattr(back, name).reshape(P, -1), getattr(cloud, name).reshape(P, -1)), name
    # one render of the seeds
    cam = scenes.look_at_camera(64, 64, (0.0, 0.0, -3.0), (0.0, 0.0, 0.0), fovx_deg=40.0)
    act = cloud.activated()
    rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, t.zeros(3), 1.0, cam.viewmatrix.cuda(),
                                       cam.projmatrix.cuda(), 3, cam.campos.cuda(), False, False)
    color, radii, depth, median, opac = GaussianRasterizer(rs)(
        means3D=act["means3D"], means2D=t.zeros_like(act["means3D"]), opacities=act["opacities"], shs=act["shs"],
        scales=act["scales"], rotations=act["rotations"])
    assert tuple(color.shape) == (3, 64, 64) and bool(t.isfinite(color).all()) and bool(t.isfinite(opac).all())
    assert float(opac.max()) > 0
    # the one-call form gives the same three results
    cameras, masks = vm.ring_scene(6, 64, 48, distance=3.0, fov_deg=40.0, disc=0.5, elevation=0.6, seed=2)
    hull2, (v2, f2), cloud2 = visual_hull_init(cameras, to_dev(masks), resolution=32, translate=sphere_hull.translate, radius=0.9)
    assert t.equal(hull2.filled, sphere_hull.filled) and t.equal(v2, v) and t.equal(cloud2.xyz, v)
