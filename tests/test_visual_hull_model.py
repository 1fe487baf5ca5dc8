"""CPU (-m "not gpu"): the float32 model of the visual hull kernels (tests/visual_hull_model.py) against
tests/golden/py_visual_hull.npz (what the reference's own Camera.insideView / getNerfppNorm / create_from_attribute produced,
tests/golden/make_visual_hull_fixture.py), hand-computed boundary cases, the packed mask layout, the seeds and every argument
error of gaustudio_amd.visual_hull.  The GPU tests (tests/test_gpu_visual_hull.py) compare the kernels with this model exactly."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import visual_hull_model as vm  # noqa: E402
from gaustudio_amd import formats, visual_hull as vh  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "py_visual_hull.npz")))


def fixture_scene(fx):
    W, H = (int(v) for v in fx["size"])
    cameras = [(M, W, H) for M in fx["matrices"]]
    masks = [m if h else None for m, h in zip(fx["masks"], fx["has_mask"])]
    return (fx["axis_x"], fx["axis_y"], fx["axis_z"]), cameras, masks


def records(fx):
    W, H = (int(v) for v in fx["size"])
    return [formats.CameraRecord(id=n, image_name=str(n), image_width=W, image_height=H, R=R, T=T, FoVx=float(f[0]), FoVy=float(f[1]))
            for n, (R, T, f) in enumerate(zip(fx["cam_R"], fx["cam_T"], fx["cam_fov"]))]


# ---------------------------------------------------------------------------------------------- model against the reference
def test_camera_normalization_equals_getNerfppNorm(fx):
    got = vh.camera_normalization(records(fx))
    # exact to float64 round-off: the function performs the reference's operations with the reference's dtypes
    for k, ref in (("translate", fx["translate"]), ("radius", fx["radius_norm"]), ("min_radius", fx["min_radius"])):
        assert np.asarray(got[k]).dtype == np.float64 or isinstance(got[k], float)
        np.testing.assert_allclose(np.asarray(got[k], dtype=np.float64), np.asarray(ref, dtype=np.float64), rtol=1e-15, atol=0)
    assert float(fx["radius"]) == got["min_radius"] * float(fx["radius_scale"])


def test_axis_tables_are_bit_equal(fx):
    axes = vh.grid_axes(int(fx["resolution"]), float(fx["radius"]), fx["translate"])
    for got, name in zip(axes, ("axis_x", "axis_y", "axis_z")):
        assert got.dtype == F and np.array_equal(got, fx[name]), name
    # through the public defaults too: CameraRecords -> camera_normalization -> min_radius * radius_scale
    norm = vh.camera_normalization(records(fx))
    axes = vh.grid_axes(int(fx["resolution"]), norm["min_radius"] * 1.2, norm["translate"])
    assert all(np.array_equal(a, fx[n]) for a, n in zip(axes, ("axis_x", "axis_y", "axis_z")))


def test_camera_records_give_the_reference_matrices(fx):
    for rec, M in zip(records(fx), fx["matrices"]):
        assert np.array_equal(rec.cam.projmatrix.numpy(), M)
    triples = vh._camera_triples(records(fx))
    assert all(np.array_equal(t[0], M) and t[1:] == (48, 36) for t, M in zip(triples, fx["matrices"]))


def test_model_against_the_reference_with_attribution(fx):
    """Every (voxel, camera) decision on which the float32 model and the reference (whose clip coordinates come from
    torch.matmul, another summation order) disagree must be attributed by the float64 replay to a decision boundary closer
    than 1e-4, and there may be at most 0.1 % of the grid of them.  Observed with the committed fixture: 0 disagreements
    (fixture `meta`); the attribution machinery is kept, and exercised by test_attribution_sees_a_boundary."""
    axes, cameras, masks = fixture_scene(fx)
    filled, count, carved_by, keep = vm.carve(axes, cameras, masks, per_camera=True)
    keep64, margin = vm.replay64(axes, cameras, masks)
    bad, ndiff = vm.unattributed(keep, fx["inside"], margin, 1e-4)
    print(f"model vs reference: {ndiff} differing decisions, {len(bad)} unattributed; fixture meta: {fx['meta']}")
    assert ndiff <= 1e-3 * filled.size
    assert len(bad) == 0
    # `filled` itself: a differing voxel must have a differing decision at a camera that decides it
    diff = np.flatnonzero(filled.ravel() != fx["filled"])
    assert len(diff) <= 1e-3 * filled.size
    for v in diff:
        cams = np.flatnonzero(keep[:, v] != fx["inside"][:, v])
        assert len(cams) and (margin[cams, v] < 1e-4).all()
    assert np.array_equal(fx["inside"].all(axis=0), fx["filled"])
    assert count == int(filled.sum()) and 0 < int(fx["filled"].sum()) < filled.size
    # carved_by is the first camera of the list that does not keep the voxel
    first = np.where(keep.all(axis=0), -1, np.argmin(keep, axis=0))
    assert np.array_equal(carved_by.ravel(), first)
    # float64 and float32 decisions agree wherever the replay sees no boundary nearby
    assert np.array_equal(keep64[margin >= 1e-4], keep[margin >= 1e-4])


def test_attribution_sees_a_boundary():
    """A point a hair inside ndc.x = 1 and one a hair across a mask edge have small margins; a point in the middle of a
    uniform mask region does not."""
    I = np.eye(4, dtype=F)
    mask = np.zeros((4, 8), dtype=np.uint8)
    mask[:, 4:] = 1                                                     # the edge between pixels 3 and 4: ndc.x = 0
    axes = (np.array([1 - 1e-6, 1e-6, 0.5], dtype=F), np.array([0.1], dtype=F), np.array([1.0], dtype=F))
    keep, margin = vm.replay64(axes, [(I, 8, 4)], [mask])
    assert keep.tolist() == [[True, True, True]]
    assert margin[0, 0] < 1e-5 and margin[0, 1] < 1e-5 and margin[0, 2] > 0.2
    other = keep.copy()
    other[0, 2] = False
    bad, ndiff = vm.unattributed(keep, other, margin)
    assert ndiff == 1 and bad.tolist() == [[0, 2]]
    other = keep.copy()
    other[0, 0] = False
    assert len(vm.unattributed(keep, other, margin)[0]) == 0


# ---------------------------------------------------------------------------------------------- hand-computed cases
def identity_case():
    """Identity full_proj_transform: clip = (x, y, z, 1), ndc = the point.  Axis tables -1, 0, 1; mask 4 x 3 (W x H)."""
    t = np.array([-1.0, 0.0, 1.0], dtype=F)
    return (t, t, t), (np.eye(4, dtype=F), 4, 3)


def test_identity_boundaries_by_hand():
    axes, cam = identity_case()
    # x = -1 -> pixel 0; x = 0 -> (0 + 1) * 0.5 * 4 = 2; x = 1 -> pixel 4, clamped to 3.  y = -1 -> 0; y = 0 -> 1.5 -> 1; y = 1 -> 3 -> 2
    col, row = [0, 2, 3], [0, 1, 2]
    rng = np.random.default_rng(3)
    for trial in range(4):
        mask = rng.integers(0, 2, (3, 4)).astype(np.uint8)
        filled, count, carved_by = vm.carve(axes, [cam], [mask])
        assert not filled[:, :, 0].any() and not filled[:, :, 1].any()           # z = -1 and z = 0 are not in front
        for i in range(3):
            for j in range(3):
                assert filled[i, j, 2] == bool(mask[row[i], col[j]]), (trial, i, j)
        assert count == int(filled.sum()) and np.array_equal(carved_by == -1, filled)
    only_last_column = np.zeros((3, 4), dtype=np.uint8)
    only_last_column[:, 3] = 1
    filled = vm.carve(axes, [cam], [only_last_column])[0]
    assert filled[:, 2, 2].all() and not filled[:, :2, 2].any()                    # ndc.x = 1 lands on pixel W, read as W - 1
    only_first = np.zeros((3, 4), dtype=np.uint8)
    only_first[0, 0] = 1
    filled = vm.carve(axes, [cam], [only_first])[0]
    assert filled[0, 0, 2] and filled.sum() == 1                                   # ndc = (-1, -1) lands on pixel (0, 0)
    assert vm.carve(axes, [cam], [None])[0][:, :, 2].all()                         # no mask: the whole view is kept


def test_negative_w_by_hand():
    """w = -1: ndc = -point, in_front still tests clip.z.  The point (1, -1, 1) reads pixel ndc (-1, 1) -> (0, H - 1)."""
    axes, (_, W, H) = identity_case()
    M = np.diag([1, 1, 1, -1]).astype(F)
    mask = np.zeros((3, 4), dtype=np.uint8)
    mask[2, 0] = 1
    filled = vm.carve(axes, [(M, W, H)], [mask])[0]
    assert filled[0, 2, 2] and filled.sum() == 1                                   # (i, j, k) = (y = -1, x = 1, z = 1)
    # w = 0: ndc is inf or nan, never inside
    M0 = np.diag([1, 1, 1, 0]).astype(F)
    assert not vm.carve(axes, [(M0, W, H)], [None])[0].any()


def test_outside_one_view_is_carved():
    axes, cam = identity_case()
    wide = (np.array([-2.0, 0.0, 2.0], dtype=F), axes[1], axes[2])
    filled, _, carved_by = vm.carve(wide, [cam, cam], [None, None])
    assert not filled[:, 0, :].any() and not filled[:, 2, :].any() and filled[:, 1, 2].all()
    assert (carved_by[:, 0, :] == 0).all()                                          # the FIRST camera of the list


# ---------------------------------------------------------------------------------------------- bit packing
def test_pack_bits_37x29_row_tail():
    rng = np.random.default_rng(5)
    mask = (rng.random((29, 37)) < 0.5).astype(np.uint8)                            # W = 37: stride 2, a row tail of 5 bits
    words, stride = vm.pack_bits(mask)
    assert stride == 2 and words.dtype == np.uint32 and words.shape == (58,)
    for y in range(29):
        for x in range(37):
            assert (int(words[y * 2 + (x >> 5)]) >> (x & 31)) & 1 == mask[y, x]
        assert int(words[y * 2 + 1]) >> 5 == 0                                     # the padding bits are zero
    assert np.array_equal(vm.unpack_bits(words, stride, 37, 29), mask.astype(bool))
    f = mask.astype(F) * F(-0.25)
    f[0, 0] = np.nan                                                                # .bool(): nonzero, NaN included, -0.0 not
    f[0, 1] = -0.0
    w2, _ = vm.pack_bits(f)
    want = mask.astype(bool)
    want[0, 0], want[0, 1] = True, False
    assert np.array_equal(vm.unpack_bits(w2, 2, 37, 29), want)
    assert np.array_equal(vm.pack_bits(mask.astype(bool))[0], words)


# ---------------------------------------------------------------------------------------------- seeds
def test_seeds_equal_create_from_attribute(fx):
    xyz = torch.from_numpy(fx["seed_xyz"])
    hull = vh.VisualHull(torch.zeros((2, 2, 2), dtype=torch.bool), None, np.zeros(3), 1.0, 0)
    cloud = hull.seeds(sh_degree=3, vertices=xyz)
    for k in ("xyz", "f_dc", "f_rest", "opacity", "scale", "rot"):
        got, ref = getattr(cloud, k), fx["seed_" + k]
        assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape, k
        assert np.array_equal(got.numpy(), ref), k
    assert (cloud.opacity == 0.1).all() and (cloud.scale == 0.01).all()             # raw values: no logit, no log
    assert cloud.max_sh_degree == 3 and hull.seeds(sh_degree=1, vertices=xyz).f_rest.shape == (5, 3, 3)
    with pytest.raises(ValueError, match="sh_degree"):
        hull.seeds(sh_degree=4, vertices=xyz)


# ---------------------------------------------------------------------------------------------- argument errors
def test_argument_errors(fx):
    """All raised before anything touches the GPU (this test runs without one)."""
    _, cameras, _ = fixture_scene(fx)
    cpu_masks = [torch.from_numpy(m) for m in fx["masks"]]
    kw = dict(translate=np.zeros(3), radius=1.0)
    with pytest.raises(ValueError, match="resolution must be at least 2"):
        vh.carve(cameras, cpu_masks, resolution=1, **kw)
    with pytest.raises(TypeError, match="resolution must be an int"):
        vh.carve(cameras, cpu_masks, resolution=12.5, **kw)
    with pytest.raises(ValueError, match="2\\^31"):
        vh.carve(cameras, cpu_masks, resolution=1300, **kw)
    with pytest.raises(ValueError, match="camera list is empty"):
        vh.carve([], [], **kw)
    with pytest.raises(ValueError, match="ROCm devices only"):
        vh.carve(cameras, cpu_masks, **kw)
    with pytest.raises(ValueError, match=r"mask 2 must have shape \[36, 48\]"):
        vh.carve(cameras, cpu_masks[:2] + [torch.zeros(48, 36)] + cpu_masks[3:], **kw)
    with pytest.raises(ValueError, match="7 cameras but 6 masks"):
        vh.carve(cameras, cpu_masks[:6], **kw)
    with pytest.raises(TypeError, match="mask 0 must be a torch tensor"):
        vh.carve(cameras, [fx["masks"][0]] + cpu_masks[1:], **kw)
    with pytest.raises(TypeError, match="uint8, bool or float32"):
        vh.carve(cameras, [cpu_masks[0].double()] + cpu_masks[1:], **kw)
    with pytest.raises(TypeError, match="camera 0"):
        vh.carve([object()] + cameras[1:], cpu_masks, **kw)
    with pytest.raises(ValueError, match=r"shape \[4, 4\]"):
        vh.carve([(np.eye(3), 48, 36)] + cameras[1:], cpu_masks, **kw)
    with pytest.raises(ValueError, match="image size"):
        vh.carve([(np.eye(4), 0, 36)] + cameras[1:], cpu_masks, **kw)
    with pytest.raises(ValueError, match="translate and radius must be given"):
        vh.carve(cameras, [None] * 7)
    with pytest.raises(ValueError, match="radius must be positive"):
        vh.carve(cameras, [None] * 7, translate=np.zeros(3), radius=0.0)
    with pytest.raises(ValueError, match="three finite numbers"):
        vh.carve(cameras, [None] * 7, translate=np.zeros(2), radius=1.0)
    with pytest.raises(ValueError, match="at least one camera"):
        vh.camera_normalization([])
    with pytest.raises(TypeError, match="CameraRecord"):
        vh.camera_normalization(cameras)
    with pytest.raises(ValueError, match="ROCm devices only"):
        vh.carve_axes(cameras, cpu_masks, (np.zeros(3, F),) * 3)
    with pytest.raises(ValueError, match="non-empty vector"):
        vh.carve_axes(cameras, [None] * 7, (np.zeros((2, 2), F),) * 3)
    hull = vh.VisualHull(torch.zeros((2, 2, 2), dtype=torch.bool), None, np.zeros(3), 1.0, 0)
    with pytest.raises(ValueError, match="threshold"):
        hull.extract_mesh(threshold=1.0)


def test_library_exports_the_hull_entry_points():
    from gaustudio_amd import _C
    import gaustudio_amd
    L = _C.lib()
    assert hasattr(L, "gsr_hull_pack_masks") and hasattr(L, "gsr_hull_carve")
    import ctypes
    assert ctypes.sizeof(vh._HullCamera) == 96
    assert gaustudio_amd.carve is vh.carve and gaustudio_amd.VisualHull is vh.VisualHull
