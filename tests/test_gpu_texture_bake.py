"""GPU tests of gaustudio_amd.texture_bake (csrc/gsr_mesh_bake.hip bake_select / bake_sample) against the float32 model
tests/texture_bake_model.py.  Every comparison with the model is exact (np.array_equal, NaN positions included): cos, the
colours and baked_by -- the library is built without contraction, with correctly rounded divides and square roots, and the
model performs the kernels' operations in their order.  The model is given the visibility the device rasterizer found
(bit-equal to tests/mesh_raster_model.py by tests/test_gpu_mesh_raster.py; one test here checks that again)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mesh_raster_model as rm  # noqa: E402
import texture_bake_model as tm  # noqa: E402
from gaustudio_amd import texture_bake as tb  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
RED, GREEN = F32([1, 0, 0]), F32([0, 1, 0])


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def oriented(verts, faces, E=np.eye(4), towards=True):
    """The faces rewound so that every normal points at the camera (cos < 0), or away from it."""
    faces = np.array(faces, dtype=np.int32).reshape(-1, 3)
    cos, _ = tm.select(verts, faces, np.ones(len(faces), bool), E)
    swap = (cos > 0) == towards
    faces[swap] = faces[swap][:, [0, 2, 1]]
    return faces


def run(verts, faces, views, sampling="reference", strict=True):
    """Bakes on the device and in the model, compares everything, returns (colors, baked_by, [cos], [visible], [stats])."""
    verts, faces = np.asarray(verts, dtype=F32), np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    baker = tb.TextureBaker(dev(verts), dev(faces), sampling)
    colors = np.zeros((len(verts), 3), dtype=F32)
    baked_by = np.full(len(verts), -1, dtype=np.int32)
    coss, visibles, stats = [], [], []
    for seq, (image, K, E) in enumerate(views):
        H, W = image.shape[:2]
        vis = baker.raster.visible_faces(baker.raster.rasterize(K, E, H, W)).cpu().numpy()
        st = baker.add_view(dev(image), K, E, strict=strict)
        cos, sel, m = tm.add_view(colors, baked_by, seq, verts, faces, vis, image, K, E, sampling)
        got_cos = baker.last_cos.cpu().numpy()
        assert got_cos.dtype == F32 and np.array_equal(got_cos, cos, equal_nan=True), f"view {seq}: cos differs"
        assert (st.visible_faces, st.selected_faces, st.baked_vertices) == (int(vis.sum()), int(sel.sum()), int(m.sum())), f"view {seq}"
        if vis.any():
            mean = np.where(vis, cos, 0).astype(np.float64).sum() / vis.sum()
            assert np.isnan(mean) if np.isnan(st.mean_cos) else abs(st.mean_cos - mean) <= 1e-5
        else:
            assert np.isnan(st.mean_cos)
        coss.append(cos), visibles.append(vis), stats.append(st)
    got_c, got_b = baker.vertex_colors.cpu().numpy(), baker.baked_by.cpu().numpy()
    assert got_c.dtype == F32 and got_b.dtype == np.int32
    assert np.array_equal(got_b, baked_by), "baked_by differs from the model"
    assert np.array_equal(got_c, colors, equal_nan=True), "colours differ from the model"
    return got_c, got_b, coss, visibles, stats


def ring_views(n, W, H, fx, image_of, radius=3.0, cx=None, cy=None):
    views = []
    for a in range(n):
        t = 2 * np.pi * a / n + 0.3
        E = rm.look_at((radius * np.cos(t), 0.4 * (-1) ** a, radius * np.sin(t)), (0, 0, 0))
        views.append((image_of(a), tm.intrinsics(fx, fx, W / 2 if cx is None else cx, H / 2 if cy is None else cy), E))
    return views


# ------------------------------------------------------------------------------------------------ small scenes
@pytest.mark.parametrize("sampling", ["reference", "exact"])
def test_one_triangle_under_a_gradient(sampling):
    W, H = 8, 6
    verts = F32([[-0.5, -0.4, 2], [0.6, -0.3, 2], [0.1, 0.5, 2]])
    faces = oriented(verts, [[0, 1, 2]])
    image = tm.gradient_image(H, W, 0.1, 0.1, 0.03)
    colors, baked_by, coss, _, _ = run(verts, faces, [(image, tm.intrinsics(6.0, 6.0, 4.0, 3.0), np.eye(4))], sampling)
    assert (baked_by == 0).all() and coss[0][0] == -1 and (colors > 0).all()
    assert len({tuple(c) for c in colors}) == 3


def test_facing_threshold():
    """Two faces on the shared edge (0, -+0.3, 3): one tilted to cos ~ -0.2, the other to ~ -0.02, past the -0.05 limit."""
    W, H = 64, 48
    tilt = lambda c, side: (side * 2 * c, 0.0, 3 + 2 * np.sqrt(1 - c * c))
    verts = F32([[0, -0.3, 3], [0, 0.3, 3], tilt(0.2, -1), tilt(0.02, 1)])
    faces = oriented(verts, [[0, 1, 2], [0, 1, 3]])
    image = tm.gradient_image(H, W, 0.2, 0.01, 0.004)
    colors, baked_by, coss, vis, st = run(verts, faces, [(image, tm.intrinsics(200.0, 200.0, 32.0, 24.0), np.eye(4))])
    cos = coss[0]
    assert vis[0].all() and abs(cos[0] + 0.2) < 0.01 and abs(cos[1] + 0.02) < 0.005
    assert (np.abs(cos - tm.COS_LIMIT) > 1e-4).all()
    assert st[0].visible_faces == 2 and st[0].selected_faces == 1
    assert list(baked_by) == [0, 0, 0, -1] and not colors[3].any() and (colors[:3] > 0).all()


def test_occlusion_is_per_face():
    """A rear face that is partly visible colours all its vertices, the hidden one included; a fully hidden face none."""
    W, H = 48, 36
    verts = F32([[-0.5, -0.5, 2], [0.5, -0.5, 2], [0.5, 0.5, 2], [-0.5, 0.5, 2],          # the occluder
                 [0, 0, 4], [3, 0, 4], [0, 2, 4],                                          # rear, vertex 4 behind the occluder
                 [-0.3, -0.6, 4], [0.3, -0.6, 4], [0, -0.2, 4]])                           # rear, wholly behind it
    faces = oriented(verts, [[0, 1, 2], [0, 2, 3], [4, 5, 6], [7, 8, 9]])
    image = tm.gradient_image(H, W, 0.1, 0.01, 0.01)
    colors, baked_by, _, vis, _ = run(verts, faces, [(image, tm.intrinsics(20.0, 20.0, 24.0, 18.0), np.eye(4))])
    assert list(vis[0]) == [True, True, True, False]
    assert (baked_by[:7] == 0).all() and (baked_by[7:] == -1).all() and not colors[7:].any()


@pytest.mark.parametrize("sampling", ["reference", "exact"])
def test_validity_is_inclusive(sampling):
    """z = 1, fx = 8, cx = 8 in a 16 x 12 image: the reference's x = 16 - u.  Vertex 0 has x = 0 (g = -1), vertex 1 x = 15 = W - 1
    (g = +1), vertex 2 x = 16: outside for the reference although its pixel u = 0 is on the image's edge."""
    W, H = 16, 12
    verts = F32([[1, 0, 1], [-0.875, 0.25, 1], [-1, -0.5, 1], [0, 0.5, 1]])
    faces = oriented(verts, [[0, 1, 3], [1, 2, 3], [0, 2, 1]])
    image = tm.random_image(H, W, seed=4)
    colors, baked_by, _, vis, _ = run(verts, faces, [(image, tm.intrinsics(8.0, 8.0, 8.0, 6.0), np.eye(4))], sampling)
    x, _, u, _ = tm.screen_points(verts, tm.intrinsics(8.0, 8.0, 8.0, 6.0), np.eye(4))
    assert list(x[:3]) == [0, 15, 16] and list(u[:3]) == [16, 1, 0] and vis[0].all()
    assert list(baked_by) == ([0, 0, -1, 0] if sampling == "reference" else [0, 0, 0, 0])


def test_view_order():
    """Constant red and green views: the later view wins where both see a vertex, and swapping the order swaps the result."""
    W, H = 48, 36
    v, f = rm.icosphere(1)
    red, green = np.zeros((H, W, 3), F32) + RED, np.zeros((H, W, 3), F32) + GREEN
    K = tm.intrinsics(40.0, 40.0, W / 2, H / 2)
    Ea, Eb = rm.look_at((3, 0.2, 0.5), (0, 0, 0)), rm.look_at((0.5, 0.2, 3), (0, 0, 0))
    c1, b1, _, _, _ = run(v, f, [(red, K, Ea), (green, K, Eb)])
    c2, b2, _, _, _ = run(v, f, [(green, K, Eb), (red, K, Ea)])
    both = (b1 == 1) & (b2 == 1)                  # baked by the second view either way: seen by both
    only_a, only_b = (b1 == 0), (b2 == 0)         # never overwritten by the other view
    assert both.sum() > 3 and only_a.sum() > 3 and only_b.sum() > 3 and (b1 == -1).sum() > 3
    assert np.array_equal(b1 == -1, b2 == -1)
    # the four bilinear weights sum to 1 only up to rounding (and to less where a tap falls off the image): the other channels are 0
    is_red = lambda c: (c[:, 0] > 0.2).all() and not c[:, 1:].any()
    is_green = lambda c: (c[:, 1] > 0.2).all() and not c[:, [0, 2]].any()
    assert is_green(c1[both]) and is_red(c2[both])
    assert is_red(c1[only_a]) and is_red(c2[only_a]) and (b2[only_a] == 1).all()
    assert is_green(c1[only_b]) and is_green(c2[only_b]) and (b1[only_b] == 1).all()


@pytest.mark.parametrize("W,H", [(7, 5), (50, 33)])
@pytest.mark.parametrize("sampling", ["reference", "exact"])
def test_ragged_sizes_off_centre(W, H, sampling):
    v, f = rm.icosphere(1)
    image_of = lambda a: tm.random_image(H, W, seed=10 * W + a)
    views = ring_views(3, W, H, 0.8 * W, image_of, cx=W / 2 + 0.7, cy=H / 2 - 1.2)
    _, baked_by, _, _, stats = run(v, f, views, sampling)
    assert (baked_by >= 0).sum() > 10 and all(s.selected_faces > 0 for s in stats)


def test_vertex_behind_the_camera():
    """A face that crosses the camera plane: its front part is visible, and its vertex at z_c = -1 is looked up all the same
    (x = (fx (-x_c)) / z_c + cx is finite there): the reference does not reject it."""
    W, H = 32, 24
    verts = F32([[-0.5, -0.2, 2], [0.5, -0.2, 2], [0.1, 0.05, -1]])
    faces = oriented(verts, [[0, 1, 2]])
    K = tm.intrinsics(20.0, 20.0, 16.0, 12.0)
    image = tm.random_image(H, W, seed=8)
    for sampling in tb.SAMPLING:
        colors, baked_by, coss, vis, _ = run(verts, faces, [(image, K, np.eye(4))], sampling)
        assert vis[0][0] and coss[0][0] < -0.05
        assert list(baked_by) == [0, 0, 0] and colors[2].any()


def test_degenerate_and_nan_faces():
    W, H = 32, 24
    verts = F32([[-0.5, -0.4, 2], [0.6, -0.3, 2], [0.1, 0.5, 2], [0.3, 0.3, 1.5], [np.nan, 0, 2], [0.2, 0.2, 1.5], [0.2, 0.2, 1.5]])
    faces = np.concatenate([oriented(verts[:3], [[0, 1, 2]]), [[0, 1, 4], [3, 5, 6], [0, 0, 1]]]).astype(np.int32)
    K = tm.intrinsics(20.0, 20.0, 16.0, 12.0)
    image = tm.random_image(H, W, seed=9)
    colors, baked_by, coss, vis, _ = run(verts, faces, [(image, K, np.eye(4))])
    assert list(vis[0]) == [True, False, False, False] and list(baked_by) == [0, 0, 0, -1, -1, -1, -1]
    # the filter on its own, every face declared visible: NaN for the degenerate faces and the NaN vertex, nothing stamped for them
    baker = tb.TextureBaker(dev(verts), dev(faces))
    cos = baker.select(dev(np.ones(4, dtype=bool)), np.eye(4), 0).cpu().numpy()
    want, sel = tm.select(verts, faces, np.ones(4, bool), np.eye(4))
    assert np.array_equal(cos, want, equal_nan=True) and list(np.isnan(cos)) == [False, True, True, True] and list(sel) == [True, False, False, False]
    assert list(baker._stamp.cpu().numpy()) == [0, 0, 0, -1, -1, -1, -1]


def test_orientation_check():
    W, H = 48, 36
    v, f = rm.icosphere(1)
    inside_out = np.ascontiguousarray(f[:, [0, 2, 1]])
    view = (tm.random_image(H, W, seed=2), tm.intrinsics(40.0, 40.0, 24.0, 18.0), rm.look_at((3, 0.2, 0.5), (0, 0, 0)))
    baker = tb.TextureBaker(dev(v), dev(inside_out))
    with pytest.raises(ValueError, match="view direction"):
        baker.add_view(dev(view[0]), view[1], view[2])
    assert (baker.baked_by.cpu().numpy() == -1).all() and not baker.vertex_colors.cpu().numpy().any()
    st = baker.add_view(dev(view[0]), view[1], view[2], strict=False)
    assert st.visible_faces > 10 and st.selected_faces == 0 and st.baked_vertices == 0 and st.mean_cos > 0.3
    assert (baker.baked_by.cpu().numpy() == -1).all() and not baker.vertex_colors.cpu().numpy().any()
    run(v, inside_out, [view], strict=False)


# ------------------------------------------------------------------------------------------------ past one block
@pytest.mark.parametrize("sampling", ["reference", "exact"])
def test_icosphere_four_views(sampling):
    """320 faces and 162 vertices: the last block of either kernel is partly filled.  The visibility is checked against the
    rasterizer's model as well; two runs are bit-identical."""
    W, H = 48, 36
    v, f = rm.icosphere(2)
    assert f.shape[0] == 320 and v.shape[0] == 162
    views = ring_views(4, W, H, 40.0, lambda a: tm.random_image(H, W, seed=20 + a))
    colors, baked_by, _, vis, _ = run(v, f, views, sampling)
    for (image, K, E), got in zip(views, vis):
        assert np.array_equal(got, tm.visible_faces(v, f, K, E, H, W))
    assert sorted(np.unique(baked_by)) == [0, 1, 2, 3] or sorted(np.unique(baked_by)) == [-1, 0, 1, 2, 3]
    import torch
    c2, b2, stats = tb.bake_vertex_colors(dev(v), dev(f), [(dev(i), K, E) for i, K, E in views], sampling=sampling)
    assert torch.equal(c2.cpu(), torch.from_numpy(colors)) and torch.equal(b2.cpu(), torch.from_numpy(baked_by)) and len(stats) == 4


def test_strip_257_faces():
    W, H = 320, 24                           # wide enough for every face of the strip to own a pixel
    x = np.linspace(-1.2, 1.2, 259)          # a zig-zag strip across the image: V = 259, F = 257
    verts = np.stack([x, np.where(np.arange(259) % 2 == 0, -0.5, 0.5) + 0.1 * np.sin(7 * x), 2 + 0.3 * np.cos(5 * x)], axis=1).astype(F32)
    faces = oriented(verts, np.stack([np.arange(257), np.arange(257) + 1, np.arange(257) + 2], axis=1))
    assert faces.shape[0] == 257 and verts.shape[0] == 259
    image = tm.random_image(H, W, seed=31)
    colors, baked_by, _, vis, st = run(verts, faces, [(image, tm.intrinsics(240.0, 30.0, 160.0, 12.0), np.eye(4))])
    assert vis[0].sum() > 200 and baked_by[-1] == 0 and baked_by[256] == 0 and (baked_by == 0).sum() > 200


# ------------------------------------------------------------------------------------------------ nothing to do
def test_empty_mesh_and_blind_view():
    import torch
    W, H = 16, 12
    image, K = tm.random_image(H, W, seed=1), tm.intrinsics(10.0, 10.0, 8.0, 6.0)
    colors, baked_by, stats = tb.bake_vertex_colors(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"),
                                                    [(dev(image), K, np.eye(4))])
    assert colors.shape == (0, 3) and baked_by.shape == (0,) and stats[0].visible_faces == 0 and np.isnan(stats[0].mean_cos)
    v, f = rm.icosphere(0)
    away = rm.look_at((3, 0, 0), (6, 0, 0))                       # the mesh is behind the camera
    colors, baked_by, _, vis, st = run(v, f, [(image, K, away), (image, K, rm.look_at((3, 0, 0), (0, 0, 0)))])
    assert not vis[0].any() and st[0].baked_vertices == 0 and np.isnan(st[0].mean_cos)
    assert st[1].baked_vertices > 0 and set(np.unique(baked_by)) == {-1, 1}


def test_uint8_image():
    W, H = 16, 12
    v, f = rm.icosphere(0)
    K, E = tm.intrinsics(10.0, 10.0, 8.0, 6.0), rm.look_at((3, 0, 0), (0, 0, 0))
    img8 = (tm.random_image(H, W, seed=5) * 255).astype(np.uint8)
    c8, b8, _ = tb.bake_vertex_colors(dev(v), dev(f), [(dev(img8), K, E)])
    cf, bf, _ = tb.bake_vertex_colors(dev(v), dev(f), [(dev(img8).float() / 255.0, K, E)])
    assert np.array_equal(c8.cpu().numpy(), cf.cpu().numpy()) and np.array_equal(b8.cpu().numpy(), bf.cpu().numpy()) and (b8 == 0).any()
