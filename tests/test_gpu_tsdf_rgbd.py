"""GPU tests of gaustudio_amd.tsdf_rgbd.ColorTSDFVolume (csrc/gsr_tsdf_rgbd.hip) against the float32 model
tests/tsdf_rgbd_model.py.  Every comparison with the model is exact (np.array_equal): block set, weights, tsdf, colours,
vertices, faces and vertex colours -- the library is built without contraction and with correctly rounded divide / sqrt,
and the model performs the kernels' operations in their order."""
import collections
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import tsdf_rgbd_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
CENTRE = np.array([-1.3, -0.7, -2.1])            # the scene lives in negative world coordinates (floor division of blocks)
RADIUS = 0.5


def _torch():
    import torch
    return torch


def look_at(eye, target, roll=0.0):
    """World-to-camera 4x4 (OpenCV axes: x right, y down, z forward), rolled about the optical axis."""
    eye, target = np.asarray(eye, float), np.asarray(target, float)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    right = np.cross(fwd, up); right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    c, s = np.cos(roll), np.sin(roll)
    right, down = c * right + s * down, -s * right + c * down
    E = np.eye(4)
    E[:3, :3] = np.stack([right, down, fwd])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def sphere_frame(H, W, K, E, centre=CENTRE, radius=RADIUS, two_tone=False):
    """Depth (z along the optical axis, 0 where the ray misses) and uint8 colour of a sphere; the ray of pixel (u, v) is
    ((u - cx) / fx, (v - cy) / fy, 1)."""
    fx, fy, cx, cy = K
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, float)], axis=-1)
    c = E[:3, :3] @ centre + E[:3, 3]
    a, b, cc = (d * d).sum(-1), d @ c, c @ c - radius * radius
    disc = b * b - a * cc
    t = np.where(disc > 0, (b - np.sqrt(np.maximum(disc, 0))) / a, 0.0)
    t = np.where(t > 0, t, 0.0)
    pw = (t[..., None] * d - E[:3, 3]) @ E[:3, :3]                      # world position of the hit
    n = (pw - centre) / radius
    if two_tone:
        col = np.where(n[..., :1] < 0, np.array([255, 0, 0]), np.array([0, 0, 255]))
    else:
        col = np.clip(127.5 + 127.5 * n, 0, 255)
    return t.astype(F), col.astype(np.uint8)


def gpu_volume(vl, tr, capacity=1 << 12, stride=4):
    from gaustudio_amd import ColorTSDFVolume
    return ColorTSDFVolume(vl, tr, depth_sampling_stride=stride, capacity_blocks=capacity)


def gpu_integrate(vol, depth, color, K, E, depth_trunc=5.0):
    t = _torch()
    vol.integrate(t.from_numpy(np.ascontiguousarray(depth)).cuda(), t.from_numpy(np.ascontiguousarray(color)).cuda(), K, E, depth_trunc)


def assert_same_state(vol, model):
    """Block set, voxel coordinates, tsdf, weight and colour of the device volume equal the model's, bit for bit."""
    _, bcoords = vol.occupied_blocks()
    assert {tuple(b) for b in bcoords.cpu().numpy().tolist()} == set(model.blocks)
    got = [x.cpu().numpy() for x in vol.export_voxels()]
    want = model.export_voxels()
    for name, g, w in zip(("coords", "tsdf", "weight", "color"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), f"{name} differs from the model"
    return want


def assert_same_mesh(vol, model, min_weight=0.0, allow_empty=False):
    v, f, c = [x.cpu().numpy() for x in vol.extract_triangle_mesh_device(min_weight)]
    mv, mf, mc = model.extract_triangle_mesh(min_weight)
    assert len(mf) > 0 or allow_empty
    assert v.dtype == F and c.dtype == F and f.dtype == np.int32
    assert np.array_equal(f, mf) and np.array_equal(v, mv) and np.array_equal(c, mc)
    return v, f, c


def directed_edges(tris):
    E = collections.Counter()
    for a, b, c in tris.tolist():
        for x, y in ((a, b), (b, c), (c, a)):
            E[(x, y)] += 1
    return E


# ---------------------------------------------------------------- 1. single frame, awkward sizes
@pytest.mark.parametrize("H,W", [(37, 53), (1, 300), (200, 7), (120, 160)])
def test_single_frame_matches_the_model_exactly(H, W):
    f = 0.9 * max(H, W)
    K = (f, 1.1 * f, W / 2 - 0.7, H / 2 + 0.4)                        # off-centre principal point
    E = look_at(CENTRE + np.array([1.1, -1.4, 0.8]), CENTRE, roll=0.3)
    depth, color = sphere_frame(H, W, K, E)
    assert (depth > 0).any() and (depth == 0).any()
    model = M.ModelVolume(0.04, 0.12)
    model.integrate(depth, color, K, E)
    vol = gpu_volume(0.04, 0.12)
    gpu_integrate(vol, depth, color, K, E)
    coords, _, w, _ = assert_same_state(vol, model)
    assert len(w) > 0 and coords.max() < 0                            # negative voxel coordinates throughout
    assert_same_mesh(vol, model, allow_empty=H == 1)                  # one pixel row observes a sheet thinner than a cube


# ---------------------------------------------------------------- 2. touch box
@pytest.mark.parametrize("tr,want", [(0.2, {(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (0, 1)}),
                                     (0.8, {(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (0, 1, 2)})])
def test_touch_box_of_one_pixel(tr, want):
    d = np.zeros((9, 9), F)
    d[4, 4] = 0.8                                                     # the point (0, 0, 0.8): a corner of eight 0.8-m blocks
    col = np.full((9, 9, 3), 77, np.uint8)
    K = (10.0, 10.0, 4.0, 4.0)
    model = M.ModelVolume(0.1, tr)
    assert model.integrate(d, col, K, np.eye(4)) == want and len(want) in (8, 27)
    vol = gpu_volume(0.1, tr)
    gpu_integrate(vol, d, col, K, np.eye(4))
    assert_same_state(vol, model)
    assert vol.last_touched == len(want)


# ---------------------------------------------------------------- 3. edge rules
def test_voxels_behind_the_camera_and_zero_depth_pixels():
    # a wall 0.15 in front of the camera with sdf_trunc 0.2: the opened blocks reach behind the camera
    H, W, K = 24, 32, (30.0, 30.0, 15.5, 11.5)
    d = np.full((H, W), 0.15, F)
    d[::3, ::5] = 0.0                                                 # holes: no observation, the neighbours are untouched by them
    d[8:12, 8:20] = 0.0                                               # a hole that swallows stride-grid pixels as well
    col = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    E = look_at([-0.5, -0.6, -0.7], [-0.5, -0.6, 0.3])
    model = M.ModelVolume(0.05, 0.2)
    model.integrate(d, col, K, E)
    local = np.arange(512)
    l3 = np.stack([local & 7, (local >> 3) & 7, local >> 6], axis=1)
    behind = 0
    for b, (_, w, _) in model.blocks.items():
        ctr = ((np.asarray(b) * 8 + l3) + 0.5) * 0.05
        m = (ctr @ E[2, :3] + E[2, 3]) < -1e-3
        behind += m.sum()
        assert not w[m].any()
    assert behind > 0
    vol = gpu_volume(0.05, 0.2)
    gpu_integrate(vol, d, col, K, E)
    assert_same_state(vol, model)


def _uf(K, vl, i, E=np.eye(4)):
    """The model's u_f of voxel (i, 0, k=19) for an identity pose, operation by operation."""
    X, Z = (F(i) + F(0.5)) * F(vl), (F(19) + F(0.5)) * F(vl)
    return ((X * F(K[0])) / Z + F(K[2])) + F(0.5)


@pytest.mark.parametrize("edge", ["lower", "upper"])
def test_projection_margins_keep_and_skip(edge):
    # chosen from the model: among the floats around cx = margin - 0.5 - x fx / z, the one that puts u_f of voxel (i, 0, 19)
    # at the smallest value >= the margin ("ge") and the one that puts it at the largest value below it ("lt")
    H, W, vl, tr = 16, 40, 0.05, 0.1
    i = -3 if edge == "lower" else 3
    target = F(0.0001) if edge == "lower" else F(W) - F(0.0001)
    base = (((F(i) + F(0.5)) * F(vl)) * F(20.0)) / ((F(19) + F(0.5)) * F(vl))
    cx = F(float(target) - 0.5 - float(base))
    cands = [cx]
    for _ in range(32):
        cands = [np.nextafter(cands[0], F(-np.inf))] + cands + [np.nextafter(cands[-1], F(np.inf))]
    ufs = np.array([_uf((20.0, 20.0, c, 8.25), vl, i) for c in cands], F)
    assert (ufs >= target).any() and (ufs < target).any()
    ge = np.where(ufs >= target, ufs, F(np.inf)).argmin()
    lt = np.where(ufs < target, ufs, F(-np.inf)).argmax()
    assert abs(float(ufs[ge]) - float(ufs[lt])) < 1e-5                # the two sit right beside the margin
    found = {"ge": cands[ge], "lt": cands[lt]}
    d = np.full((H, W), 1.0, F)
    col = np.full((H, W, 3), 200, np.uint8)
    for which, c in found.items():
        K = (20.0, 20.0, float(c), 8.25)
        model = M.ModelVolume(vl, tr)
        model.integrate(d, col, K, np.eye(4))
        # lower margin: kept iff 0.0001 <= u_f; upper margin: kept iff u_f < W - 0.0001
        kept = (which == "ge") == (edge == "lower")
        assert model.voxel(i, 0, 19)[1] == (1.0 if kept else 0.0)
        assert (i >> 3, 0, 2) in model.blocks
        vol = gpu_volume(vl, tr)
        gpu_integrate(vol, d, col, K, np.eye(4))
        assert_same_state(vol, model)


def test_sdf_exactly_at_minus_trunc_is_skipped():
    # powers of two: every value below is exact.  The camera sits on the axis through the voxel centres (1/32, 1/32, .),
    # pixel (8, 8) is the principal point (multiplier 1); d = 1.03125: voxel k = 18 (z_c = 1.15625) has sdf = -0.125 exactly
    vl, tr = 0.0625, 0.125
    K = (16.0, 16.0, 8.0, 8.0)
    E = np.eye(4)
    E[:3, 3] = [-0.03125, -0.03125, 0.0]
    d = np.full((17, 17), 1.03125, F)
    col = np.full((17, 17, 3), 9, np.uint8)
    model = M.ModelVolume(vl, tr)
    model.integrate(d, col, K, E)
    assert model.voxel(0, 0, 17)[1] == 1.0 and model.voxel(0, 0, 17)[0] == F(-0.5)
    assert model.voxel(0, 0, 18)[1] == 0.0 and (0, 0, 2) in model.blocks
    vol = gpu_volume(vl, tr)
    gpu_integrate(vol, d, col, K, E)
    assert_same_state(vol, model)


# ---------------------------------------------------------------- 4 / 6 / 7. views of a sphere at 96 x 72
VL6, TR6 = 0.05, 0.15
K6 = (110.0, 110.0, 47.3, 36.6)


def _frames(directions):
    out = []
    for n, axis in enumerate(directions):
        E = look_at(CENTRE + 2.0 * np.asarray(axis, float) / np.linalg.norm(axis), CENTRE, roll=0.2 * n)
        out.append(sphere_frame(72, 96, K6, E) + (E,))
    return out


def _six_frames():
    return _frames(np.concatenate([np.eye(3), -np.eye(3)]))


def _model_run(frames):
    model = M.ModelVolume(VL6, TR6)
    states = []
    for d, c, E in frames:
        model.integrate(d, c, K6, E)
        states.append((set(model.blocks), model.export_voxels()))
    return frames, states, model, model.extract_triangle_mesh()


@pytest.fixture(scope="module")
def six_views():
    """Six views along the axes: the frames, the model's state after every frame and its mesh; computed once, never modified."""
    return _model_run(_six_frames())


@pytest.fixture(scope="module")
def full_views():
    """Full coverage: eight views from the corners of a cube (every surface point is seen within 36 degrees of frontal;
    the six axis views leave grazing patches whose cubes lack an observed corner, and the mesh open there)."""
    return _model_run(_frames([(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]))


@pytest.fixture(scope="module")
def full_volume(full_views):
    vol = gpu_volume(VL6, TR6)
    for d, c, E in full_views[0]:
        gpu_integrate(vol, d, c, K6, E)
    return vol


def test_multi_frame_state_matches_after_every_frame(six_views):
    t = _torch()
    frames, states, model, _ = six_views
    a, b = gpu_volume(VL6, TR6), gpu_volume(VL6, TR6)
    for (d, c, E), (blocks, want) in zip(frames, states):
        gpu_integrate(a, d, c, K6, E)
        _, bc = a.occupied_blocks()
        assert {tuple(x) for x in bc.cpu().numpy().tolist()} == blocks
        for g, w in zip(a.export_voxels(), want):
            assert np.array_equal(g.cpu().numpy(), w)
    assert want[2].max() >= 3                                          # voxels seen by several views: real running averages
    for d, c, E in frames:
        gpu_integrate(b, d, c, K6, E)
    assert t.equal(a.keys, b.keys) and t.equal(a.voxels, b.voxels) and t.equal(a.stamp, b.stamp)
    for x, y in zip(a.extract_triangle_mesh_device(), b.extract_triangle_mesh_device()):
        assert t.equal(x, y)


def test_a_frame_over_existing_blocks_updates_them():
    d, c, E = _six_frames()[0]
    model = M.ModelVolume(VL6, TR6)
    vol = gpu_volume(VL6, TR6)
    for _ in range(2):                                                 # the second pass allocates nothing new
        model.integrate(d, c, K6, E)
        gpu_integrate(vol, d, c, K6, E)
        n_blocks = vol.occupied_blocks()[0].shape[0]
        assert vol.last_touched == n_blocks == len(model.blocks)
    _, _, w, _ = assert_same_state(vol, model)
    assert set(w.tolist()) == {2.0}


def test_sphere_mesh_is_closed_and_matches_the_model(full_views, full_volume):
    _, _, model, (mv, mf, mc) = full_views
    v, f, c = [x.cpu().numpy() for x in full_volume.extract_triangle_mesh_device()]
    assert np.array_equal(f, mf) and np.array_equal(v, mv) and np.array_equal(c, mc)
    E = directed_edges(f)
    assert all(n == 1 and E.get((b, a), 0) == 1 for (a, b), n in E.items())    # closed, consistently oriented
    assert len(v) - len(E) // 2 + len(f) == 2
    r = np.linalg.norm(v - CENTRE, axis=1)
    assert abs(r.mean() - RADIUS) < 0.02 and r.min() > RADIUS - 0.06 and r.max() < RADIUS + 0.06
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert ((n * (v[f].mean(1) - CENTRE)).sum(1) > 0).all()                   # outward
    assert c.min() >= 0 and c.max() <= 1
    # the numpy front end: float64 vertices and colours like TSDFVolume.extract_triangle_mesh
    nv, nf, nc = full_volume.extract_triangle_mesh()
    assert nv.dtype == np.float64 and nc.dtype == np.float64 and np.array_equal(nv, v.astype(np.float64)) and np.array_equal(nf, f)


def test_min_weight_cleaning_and_normals(full_views, full_volume):
    t = _torch()
    from gaustudio_amd.mesh_clean import remove_small_components
    from gaustudio_amd.mesh_raster import MeshRasterizer
    _, _, model, _ = full_views
    assert_same_mesh(full_volume, model, min_weight=2.0)                # fewer cubes qualify; still the model's mesh
    v, f, c = full_volume.extract_triangle_mesh_device(min_weight=2.0)
    v2, f2, c2, n2 = full_volume.extract_triangle_mesh_device(min_weight=2.0, clean_ratio=0.5, with_normals=True)
    wv, wf, _, vidx, _ = remove_small_components(v, f, 0.5, return_index=True)
    assert t.equal(v2, wv) and t.equal(f2, wf) and t.equal(c2, c[vidx.long()])
    assert t.equal(n2, MeshRasterizer(v2, f2).vertex_normals())
    v3, f3, c3, n3 = full_volume.extract_triangle_mesh_device(with_normals=True)
    assert t.equal(n3, MeshRasterizer(v3, f3).vertex_normals())
    nn = n3.cpu().numpy()
    out = (v3.cpu().numpy() - CENTRE) / np.linalg.norm(v3.cpu().numpy() - CENTRE, axis=1, keepdims=True)
    assert ((nn * out).sum(1) > 0).all()                               # outward, like the faces


def test_coloured_mesh_renders_and_round_trips_through_ply(full_views, full_volume, tmp_path):
    from gaustudio_amd import formats
    from gaustudio_amd.mesh_raster import MeshRasterizer
    frames = full_views[0]
    v, f, c, n = full_volume.extract_triangle_mesh_device(with_normals=True)
    mr = MeshRasterizer(v, f)                                           # straight from the device tensors
    Kmat = np.array([[K6[0], 0, K6[2]], [0, K6[1], K6[3]], [0, 0, 1]])
    d0, c0, E0 = frames[0]
    frags = mr.rasterize(Kmat, E0, 72, 96)
    img = mr.interpolate(frags, c).cpu().numpy()
    hit = frags.pix_to_face.cpu().numpy() >= 0
    both = hit & (d0 > 0)
    assert both.sum() > 0.9 * (d0 > 0).sum()
    # the fused colours are the input's up to the blur of 0.05-m voxels on a 0.5-m sphere whose colour spans 0..255 across
    # its diameter (unrelated colours would differ by ~85 on average)
    assert np.abs(img[both] * 255 - c0[both]).mean() < 40
    p = tmp_path / "fused_mesh.ply"
    formats.write_ply_mesh(p, v, f, vertex_colors=c, vertex_normals=n)
    v2, f2, attrs = formats.read_ply_mesh(p, return_attributes=True)
    assert np.array_equal(v2, v.cpu().numpy()) and np.array_equal(f2, f.cpu().numpy())
    want = (np.clip(c.cpu().numpy().astype(np.float64), 0, 1) * 255 + 0.5).astype(np.uint8)
    assert np.array_equal(attrs["colors"], want) and np.array_equal(attrs["normals"], n.cpu().numpy())


# ---------------------------------------------------------------- 5. colour
def test_two_tone_wall_colours():
    t = _torch()
    H, W, K, vl, tr = 48, 64, (40.0, 40.0, 31.5, 23.5), 0.05, 0.1
    d = np.full((H, W), 1.0, F)
    col = np.zeros((H, W, 3), np.uint8)
    col[:, :32, 0] = 255                                               # left half pure red, right half pure blue
    col[:, 32:, 2] = 255
    E = look_at([-3.0, -2.0, -4.0], [-3.0, -2.0, -3.0])
    model = M.ModelVolume(vl, tr)
    model.integrate(d, col, K, E)
    vol = gpu_volume(vl, tr)
    gpu_integrate(vol, d, col, K, E)
    coords, _, _, vcol = assert_same_state(vol, model)
    v, f, c = assert_same_mesh(vol, model)
    # uint8 input and the equivalent float input (HWC and CHW) give identical volumes
    for as_float in (col.astype(F) / F(255), np.transpose(col.astype(F) / F(255), (2, 0, 1))):
        other = gpu_volume(vl, tr)
        gpu_integrate(other, d, as_float, K, E)
        assert t.equal(other.keys, vol.keys) and t.equal(other.voxels, vol.voxels)
    # every vertex lies on the edge between two voxels: its colour is between theirs, and exactly red where both are red
    lut = {tuple(k): q for k, q in zip(coords.tolist(), vcol)}
    g = v.astype(np.float64) / vl - 0.5
    axis = np.abs(g - np.round(g)).argmax(1)
    reds = 0
    for p, a, cv in zip(g, axis, c):
        i0 = np.round(p).astype(int)
        i0[a] = int(np.floor(p[a]))
        i1 = i0.copy()
        i1[a] += 1
        q0, q1 = lut[tuple(i0)] / F(255), lut[tuple(i1)] / F(255)
        assert np.all(cv >= np.minimum(q0, q1)) and np.all(cv <= np.maximum(q0, q1))
        if np.array_equal(q0, [1, 0, 0]) and np.array_equal(q1, [1, 0, 0]):
            assert np.array_equal(cv, [1, 0, 0])
            reds += 1
    assert reds > 50 and len(np.unique(c, axis=0)) >= 2


# ---------------------------------------------------------------- 8. failure paths
def test_overflow_and_bad_arguments_raise():
    t = _torch()
    d, c, E = _six_frames()[0]
    vol = gpu_volume(VL6, TR6, capacity=16)                            # the frame opens far more than 16 blocks
    gpu_integrate(vol, d, c, K6, E)
    for read in (vol.occupied_blocks, vol.export_voxels, vol.extract_triangle_mesh_device, vol.extract_triangle_mesh):
        with pytest.raises(RuntimeError, match="overflowed"):
            read()
    vol = gpu_volume(VL6, TR6)
    dd, cc = t.from_numpy(d), t.from_numpy(c)
    with pytest.raises(RuntimeError, match="ROCm device"):
        vol.integrate(dd, cc.cuda(), K6, E)
    with pytest.raises(RuntimeError, match="ROCm device"):
        vol.integrate(dd.cuda(), cc, K6, E)
    with pytest.raises(ValueError, match="shape"):
        vol.integrate(dd.cuda(), cc[:, :-1].contiguous().cuda(), K6, E)
    with pytest.raises(ValueError, match="shape"):
        vol.integrate(dd.cuda()[None, None], cc.cuda(), K6, E)
    singular = E.copy()
    singular[2, :3] = singular[1, :3]
    with pytest.raises(ValueError, match="singular"):
        vol.integrate(dd.cuda(), cc.cuda(), K6, singular)
    with pytest.raises(ValueError, match="intrinsic"):
        vol.integrate(dd.cuda(), cc.cuda(), (0.0, 1.0, 2.0, 3.0), E)
    assert vol.frames == 0 and vol.occupied_blocks()[0].shape[0] == 0  # nothing was integrated by the refused calls
    v, f, col = vol.extract_triangle_mesh_device()
    assert v.shape == (0, 3) and f.shape == (0, 3) and col.shape == (0, 3)


def test_fuse_rgbd_skips_frames_without_depth_or_pose(full_views, full_volume):
    t = _torch()
    from gaustudio_amd import fuse_rgbd
    frames = full_views[0]
    seq = [(d, c, K6, E) for d, c, E in frames]
    seq.insert(2, (None, frames[0][1], K6, frames[0][2]))              # no depth
    seq.insert(4, (frames[0][0], frames[0][1], K6, None))              # no pose
    v, f, c, n = fuse_rgbd(seq, voxel_size=VL6, sdf_trunc=TR6, capacity_blocks=1 << 12)
    wv, wf, wc, wn = full_volume.extract_triangle_mesh_device(with_normals=True)
    assert t.equal(v, wv) and t.equal(f, wf) and t.equal(c, wc) and t.equal(n, wn)
