"""CPU tests of the vertex-colour bake's float32 model (tests/texture_bake_model.py) and of the Python
boundary of gaustudio_amd.texture_bake / mesh_init: the sampler against torch's grid_sample called with the script's own
arguments, the camera mapping against a float64 restatement of the script's PyTorch3D camera, the affine identities that pin
both sampling modes (the reference's one-pixel quirk included)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mesh_raster_model as rm  # noqa: E402
import texture_bake_model as tm  # noqa: E402
from gaustudio_amd import mesh_init, texture_bake  # noqa: E402

F32 = np.float32
SIZES = [(7, 5), (16, 16), (50, 33), (2, 3)]          # W x H


def tol(W, H):
    """Coordinates of magnitude W carry a few ulp of error and colour slopes are <= 1 per pixel."""
    return 8 * max(W, H) * 2.0 ** -24


def grid_sample_lookup(image, x, y):
    """What the script's lookup amounts to for screen positions (x, y), written out independently: the normalised coordinates
    g = 2 p / (size - 1) - 1 and the mask `both inside [-1, 1]` in numpy float32, then torch's grid_sample with the script's
    arguments -- the image flipped in both axes, bilinear, reflection padding, align_corners=False -- on an [1, N, 1, 2] grid.
    Returns (colours of the accepted points [Na,3] clamped to [0, 1], accepted [N])."""
    H, W = image.shape[:2]
    with np.errstate(invalid="ignore"):
        g = np.stack([F32(2) * (x.astype(F32) / F32(W - 1)) - F32(1), F32(2) * (y.astype(F32) / F32(H - 1)) - F32(1)], axis=1)
        accepted = np.all(np.abs(g) <= 1, axis=1)                   # NaN compares false
    grid = torch.from_numpy(g[accepted]).reshape(1, -1, 1, 2)
    flipped = torch.from_numpy(image[::-1, ::-1].copy()).permute(2, 0, 1).unsqueeze(0)         # [1,3,H,W]
    out = torch.nn.functional.grid_sample(flipped, grid, mode="bilinear", padding_mode="reflection", align_corners=False)
    return out[0, :, :, 0].t().clamp(0, 1).numpy(), accepted


@pytest.mark.parametrize("W,H", SIZES)
def test_sampler_equals_grid_sample(W, H):
    rng = np.random.default_rng(100 + W)
    image = tm.random_image(H, W, seed=W * 100 + H)
    x = np.concatenate([rng.uniform(-1, W, 400), [0, W - 1, 0, W - 1], rng.uniform(0, W - 1, 4), [0, W - 1, np.nan]]).astype(F32)
    y = np.concatenate([rng.uniform(-1, H, 400), [0, 0, H - 1, H - 1], [0, H - 1, 0, H - 1], rng.uniform(0, H - 1, 2), [1]]).astype(F32)
    want, want_valid = grid_sample_lookup(image, x, y)
    got, valid = tm.sample_points(image, x, y, None, None, "reference")
    assert np.array_equal(valid, want_valid)
    assert 20 <= valid.sum() <= valid.size - 20      # both outcomes are exercised
    err = np.abs(got[valid].astype(np.float64) - want).max()
    print(f"{W}x{H}: max |model - grid_sample| = {err:.3g} (bound {tol(W, H):.3g}), {int(valid.sum())} valid of {valid.size}")
    assert err <= tol(W, H)


def test_sampler_corners_read_the_flipped_image():
    """g = (-1, -1) is the top-left corner of the FLIPPED image, i.e. the last texel of the image; a tap at column W is skipped,
    so the corner keeps a quarter of the texel's value (bilinear with align_corners=False)."""
    W, H = 7, 5
    image = tm.random_image(H, W, seed=1)
    got, valid = tm.sample_points(image, F32([0, W - 1]), F32([0, H - 1]), None, None, "reference")
    assert valid.all()
    assert np.array_equal(got[0], image[H - 1, W - 1]) and np.array_equal(got[1], image[0, 0])
    # the clip to [0, W - 1] comes before the taps: ix = -0.5 -> 0, all the weight on one texel


def script_screen_points(verts, K, E):
    """float64 restatement of texture_mesh.py:77-91, 129 with plain 4x4 matrices: PyTorch3D's row-vector convention
    X_view = X_world R + T, screen x = fx X / Z + px."""
    E = np.asarray(E, dtype=np.float64)
    c2w = np.linalg.inv(E)
    R, T = c2w[:3, :3], c2w[:3, 3:]
    R = np.stack([-R[:, 0], -R[:, 1], R[:, 2]], 1)
    w2c = np.linalg.inv(np.concatenate([np.concatenate([R, T], 1), [[0, 0, 0, 1]]], 0))
    R, T = w2c[:3, :3].T, w2c[:3, 3]
    view = np.asarray(verts, dtype=np.float64) @ R + T
    return K[0, 0] * view[:, 0] / view[:, 2] + K[0, 2], K[1, 1] * view[:, 1] / view[:, 2] + K[1, 2]


def test_camera_mapping_is_the_flipped_screen_camera():
    rng = np.random.default_rng(3)
    W, H = 50, 33
    K = tm.intrinsics(41.0, 39.0, 21.3, 18.9)           # principal point off centre
    E = rm.look_at((0.4, -0.3, -3.0), (0.1, 0.05, 0.0))
    verts = rng.uniform(-1, 1, (200, 3)).astype(F32)
    sx, sy = script_screen_points(verts, K, E)
    x, y, u, w = tm.screen_points(verts, K, E)
    err = max(np.abs(x - sx).max(), np.abs(y - sy).max())
    flip = max(np.abs((2 * K[0, 2] - u.astype(np.float64)) - sx).max(), np.abs((2 * K[1, 2] - w.astype(np.float64)) - sy).max())
    print(f"max |model - script| = {err:.3g} px, |(2c - u) - script| = {flip:.3g} px")
    assert err <= 1e-4 and flip <= 1e-4
    assert -W < sx.min() and sx.max() < 2 * W


def quad_scene():
    """A fronto-parallel 4 x 3 grid of quads at z = 2 seen by the identity camera, fx = fy = 20, centred principal point:
    vertex (ix, iy) sits at pixel (4 + 4 ix, 3 + 4 iy) of a 24 x 18 image."""
    W, H = 24, 18
    verts, faces = rm.grid_mesh(4, 3, -0.8, -0.6, 0.4, 2.0)            # wound to face the camera
    K, E = tm.intrinsics(20.0, 20.0, W / 2, H / 2), np.eye(4)
    return verts, faces, K, E, W, H


@pytest.mark.parametrize("sampling", ["exact", "reference"])
def test_affine_identity(sampling):
    verts, faces, K, E, W, H = quad_scene()
    a, b, c = 0.1, 0.02, 0.01
    image = tm.gradient_image(H, W, a, b, c)
    colors, baked_by, coss = tm.bake(verts, faces, [(image, K, E)], sampling)
    assert (coss[0] < -0.99).all() and (baked_by == 0).all()
    u, v = 12 + 20 * verts[:, 0].astype(np.float64) / 2, 9 + 20 * verts[:, 1].astype(np.float64) / 2
    if sampling == "exact":
        col, row = u - 0.5, v - 0.5
    else:               # the documented quirk: about one pixel off u - 0.5
        col, row = (u - 1) * W / (W - 1) - 0.5, (v - 1) * H / (H - 1) - 0.5
        assert np.abs((col - (u - 0.5))).max() > 0.3
    assert col.min() > 1 and col.max() < W - 2 and row.min() > 1 and row.max() < H - 2      # away from the clamped border
    want = (a + b * col + c * row)[:, None] * np.array([1.0, 0.5, 0.25])
    err = np.abs(colors - want).max()
    print(f"{sampling}: max error {err:.3g} (bound {tol(W, H):.3g})")
    assert err <= tol(W, H)


def test_later_views_overwrite_and_unseen_vertices_stay_zero():
    verts, faces, K, E, W, H = quad_scene()
    red = np.zeros((H, W, 3), F32) + F32([1, 0, 0])
    green = np.zeros((H, W, 3), F32) + F32([0, 1, 0])
    K_left = tm.intrinsics(20.0, 20.0, W / 2 + 6, H / 2)      # u = 10 .. 26: the first column maps to x = 2 cx - u = 26 > W - 1
    colors, baked_by, _ = tm.bake(verts, faces, [(red, K, E), (green, K_left, E)])
    assert set(np.unique(baked_by)) == {0, 1}
    assert np.array_equal(colors[baked_by == 0], np.tile(F32([1, 0, 0]), ((baked_by == 0).sum(), 1)))
    assert np.array_equal(colors[baked_by == 1], np.tile(F32([0, 1, 0]), ((baked_by == 1).sum(), 1)))
    inside_out = faces[:, [0, 2, 1]]
    colors, baked_by, coss = tm.bake(verts, inside_out, [(red, K, E)])
    assert (coss[0] > 0.99).all() and (baked_by == -1).all() and not colors.any()


def test_degenerate_face_is_not_selected():
    verts = F32([[0, 0, 2], [1, 0, 2], [2, 0, 2], [0, 1, 2]])
    faces = np.array([[0, 1, 2], [0, 3, 1]], dtype=np.int32)
    cos, sel = tm.select(verts, faces, [True, True], np.eye(4))
    assert np.isnan(cos[0]) and not sel[0] and cos[1] == -1 and sel[1]
    cos, sel = tm.select(verts, faces, [False, False], np.eye(4))
    assert np.isnan(cos).all() and not sel.any()


# ------------------------------------------------------------------------------------------------ the Python boundary
def cpu_mesh():
    v, f = rm.icosphere(0)
    return torch.from_numpy(v), torch.from_numpy(f)


def test_boundary_shapes_and_dtypes_come_before_devices():
    v, f = cpu_mesh()
    with pytest.raises(TypeError):
        texture_bake.TextureBaker(v.numpy(), f)
    with pytest.raises(TypeError):
        texture_bake.TextureBaker(v.double(), f)
    with pytest.raises(TypeError):
        texture_bake.TextureBaker(v, f.float())
    with pytest.raises(ValueError, match="shape"):
        texture_bake.TextureBaker(v[:, :2], f)
    with pytest.raises(ValueError, match="shape"):
        texture_bake.TextureBaker(v, f[:, :2])
    with pytest.raises(ValueError, match="sampling"):
        texture_bake.TextureBaker(v, f, sampling="nearest")
    with pytest.raises(ValueError, match="ROCm"):
        texture_bake.TextureBaker(v, f)
    with pytest.raises(ValueError, match="ROCm"):
        texture_bake.bake_vertex_colors(v, f, [])


def test_boundary_image_checks():
    dev = torch.device("cpu")
    with pytest.raises(TypeError):
        texture_bake._image(np.zeros((4, 4, 3), F32), dev)
    with pytest.raises(TypeError):
        texture_bake._image(torch.zeros((4, 4, 3), dtype=torch.float64), dev)
    with pytest.raises(ValueError, match="shape"):
        texture_bake._image(torch.zeros((3, 4, 4)), dev)
    with pytest.raises(ValueError, match="ROCm"):
        texture_bake._image(torch.zeros((4, 4, 3)), dev)


def test_boundary_mesh_seeds():
    v, f = cpu_mesh()
    for n in (0, 2, 5, 7, True, 1.5, "1"):
        with pytest.raises(ValueError, match="n_per_triangle"):
            mesh_init.mesh_seeds(v, f, n_per_triangle=n)
    with pytest.raises(TypeError):
        mesh_init.mesh_seeds(v.numpy(), f)
    with pytest.raises(TypeError):
        mesh_init.mesh_seeds(v, f, vertex_colors=v.double())
    with pytest.raises(TypeError):
        mesh_init.mesh_seeds(v, f, vertex_normals=v.numpy())
    with pytest.raises(ValueError, match="shape"):
        mesh_init.mesh_seeds(v, f, vertex_colors=v[:5])
    with pytest.raises(ValueError, match="shape"):
        mesh_init.mesh_seeds(v, f, vertex_normals=v[:5])
    with pytest.raises(ValueError, match="sh_degree"):
        mesh_init.mesh_seeds(v, f, sh_degree=4)
    for n in mesh_init.N_PER_TRIANGLE:
        with pytest.raises(ValueError, match="ROCm"):
            mesh_init.mesh_seeds(v, f, v, v, n_per_triangle=n)
