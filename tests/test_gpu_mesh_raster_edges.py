"""The HIP mesh rasterizer (csrc/gsr_mesh.hip) at the edges of its contract, bit for bit against the float32 replay of
tests/mesh_raster_model.py: slivers whose hits the pixel rectangle clips, independence of the tile grid, tile lists of
several LDS batches, one-pixel-wide images, mirrored and far off-axis cameras, a 60 k-face mesh at 640 x 480, and the
helpers' corner cases."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_raster_model as mm  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
RADIX_TILE = 256 * 16          # csrc/gsr_sort.h: 256 lanes x RADIX_ITEMS keys per workgroup of the radix sort


def mr():
    from gaustudio_amd import mesh_raster
    return mesh_raster


def gpu(v, f, k, E, H, W, cull=False, z_near=0.0):
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    r = mr().MeshRasterizer(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    fr = r.rasterize(k, E, H, W, cull_backfaces=cull, z_near=z_near)
    return r, fr, tuple(t.cpu().numpy() for t in fr)


def render(v, f, k, E, H, W):
    return gpu(v, f, k, E, H, W)[2]


def assert_bit_equal(got, want, what=""):
    for n, a, b in zip(("pix_to_face", "zbuf", "bary"), got, want):
        assert a.shape == b.shape, f"{what} {n} shape"
        same = a.view(np.int32) == b.view(np.int32)
        assert same.all(), f"{what} {n}: {np.count_nonzero(~same)} values differ from the float32 replay"


# ------------------------------------------------------------------------------------------------ slivers
NEEDLE_SETS = [("well-1080p-corner", 1002, mm.NEEDLES_WELL[2]), ("well-4k-corner", 1004, mm.NEEDLES_WELL[4]),
               ("pathological-0", 2000, mm.NEEDLES_PATHOLOGICAL[0]), ("pathological-1", 2001, mm.NEEDLES_PATHOLOGICAL[1])]


@pytest.mark.parametrize("name,seed,row", [pytest.param(*s, id=s[0]) for s in NEEDLE_SETS])
def test_needles(name, seed, row):
    # the sets (and seeds) of tests/test_mesh_raster_model.py: on the pathological ones the rectangle clips hits, on the
    # well-conditioned ones float32 cross products would put hits outside it (and outside the face's tiles)
    H, W = 64, 80
    v, f, k = mm.needles(np.random.default_rng(seed), 3000, H, W, *row)
    for cull in (False, True):
        _, _, got = gpu(v, f, k, np.eye(4), H, W, cull)
        assert_bit_equal(got, mm.rasterize(v, f, k, np.eye(4), H, W, cull_backfaces=cull), f"{name} cull={cull}")
        assert (got[0] >= 0).sum() > 5


def tile_grid_scenes():
    rng = np.random.default_rng(11)
    k = mm.intrinsics(45, 20.5, 17.0, fy=50)
    yield "random", mm.random_scene(rng, 300) + (k, mm.look_at([0.1, -0.1, 0], [0, 0, 3]), 37, 53)
    yield "crossing", mm.random_scene(rng, 300, crossing=True) + (k, np.eye(4), 37, 53)
    yield "needles", mm.needles(rng, 1000, 37, 53, *mm.NEEDLES_PATHOLOGICAL[0]) + (np.eye(4), 37, 53)


@pytest.mark.parametrize("name,scene", [pytest.param(*s, id=s[0]) for s in tile_grid_scenes()])
def test_tile_grid_independence(name, scene):
    # (cx, cy), W x H against (cx + 5, cy + 3), (W + 5) x (H + 3): the same rays ((j + 0.5) - cx is exact) on another place
    # of the 16 x 16 grid give the same bits
    v, f, k, E, H, W = scene
    k2 = k.copy()
    k2[0, 2] += 5
    k2[1, 2] += 3
    a = render(v, f, k, E, H, W)
    b = tuple(x[3:, 5:] for x in render(v, f, k2, E, H + 3, W + 5))
    assert (a[0] >= 0).sum() > 15
    for n, x, y in zip(("pix_to_face", "zbuf", "bary"), a, b):
        same = x.view(np.int32) == y.view(np.int32)
        assert same.all(), f"{n}: {np.count_nonzero(~same)} values depend on where the tile grid falls"
    assert_bit_equal(a, mm.rasterize(v, f, k, E, H, W), name)


# ------------------------------------------------------------------------------------------------ long tile lists
def wall(depths):
    """One triangle per entry of depths [n,3] over the directions (-9, -9), (9, -9), (0, 9): each covers a 32 x 32 image of
    f = 20, c = 16 (|d| < 0.8) with room to spare."""
    d = np.array([[-9.0, -9.0, 1.0], [9.0, -9.0, 1.0], [0.0, 9.0, 1.0]])
    v = (d[None] * np.asarray(depths, np.float64)[:, :, None]).reshape(-1, 3)
    return v.astype(np.float32), np.arange(3 * len(depths), dtype=np.int32).reshape(-1, 3)


def test_long_tile_lists():
    H = W = 32
    k = mm.intrinsics(20, 16, 16)
    rng = np.random.default_rng(21)
    # 700 parallel walls at distinct depths, ids in random depth order: three LDS batches per tile, and the walk may stop
    # after the nearest
    z = rng.permutation(np.linspace(2, 10, 700))
    v, f = wall(np.repeat(z[:, None], 3, 1))
    _, _, got = gpu(v, f, k, np.eye(4), H, W)
    assert_bit_equal(got, mm.rasterize(v, f, k, np.eye(4), H, W), "700 walls")
    assert np.all(got[0] == np.argmin(z))
    # 700 tilted walls that share (up to the order) their nearest vertex depth: every key lies below every hit z, so no
    # pixel can stop early and all three batches are walked
    za = 1 + 1e-4 * rng.permutation(700)
    zb = rng.permutation(np.linspace(2, 10, 700))
    v, f = wall(np.stack([za, zb, zb], 1))
    _, _, got = gpu(v, f, k, np.eye(4), H, W)
    want = mm.rasterize(v, f, k, np.eye(4), H, W)
    assert_bit_equal(got, want, "700 tilted walls")
    key = mm.face_key(mm.camera_space(v, np.eye(4), np.float32), f, 0.0)
    assert key.max() < got[1].min(), "the tilted walls' keys must not allow an early stop"
    assert np.all(got[0] >= 0)
    # 1000 walls behind a nearest wall whose id is last, and in front of it a pair of coincident faces over a part of the
    # image: the lower id of the pair wins there
    z = rng.permutation(np.linspace(2, 10, 1000))
    v, f = wall(np.repeat(z[:, None], 3, 1))
    small = np.array([[-0.5, -0.5, 1.5], [0.4, -0.3, 1.5], [-0.2, 0.6, 1.5]], dtype=np.float32)
    vl, _ = wall([[1.8, 1.8, 1.8]])
    v = np.concatenate([v, small, vl])
    f = np.concatenate([f, [[3000, 3001, 3002], [3000, 3001, 3002], [3003, 3004, 3005]]]).astype(np.int32)
    _, _, got = gpu(v, f, k, np.eye(4), H, W)
    assert_bit_equal(got, mm.rasterize(v, f, k, np.eye(4), H, W), "1000 walls, duplicates, nearest last")
    assert set(np.unique(got[0])) == {1000, 1002} and (got[0] == 1000).sum() > 50


# ------------------------------------------------------------------------------------------------ image shapes, cameras
@pytest.mark.parametrize("H,W", [(1, 1), (1, 40), (40, 1), (16, 17), (17, 16)])
def test_image_shapes(H, W):
    rng = np.random.default_rng(31)
    v, f = mm.random_scene(rng, 300)
    k = mm.intrinsics(30, W / 2, H / 2, fy=28)
    for cull in (False, True):
        _, _, got = gpu(v, f, k, np.eye(4), H, W, cull)
        assert got[0].shape == (H, W) and got[2].shape == (H, W, 3)
        assert_bit_equal(got, mm.rasterize(v, f, k, np.eye(4), H, W, cull_backfaces=cull), f"{H}x{W} cull={cull}")
        assert (got[0] >= 0).any()


CAMERAS = {
    "negative fx": (mm.intrinsics(-42, 30.2, 24.9, fy=47), np.eye(4)),
    "negative fy": (mm.intrinsics(42, 30.2, 24.9, fy=-47), np.eye(4)),
    "negative fx and fy": (mm.intrinsics(-42, 30.2, 24.9, fy=-47), np.eye(4)),
    # the principal point 2000 px left of and 1500 px above the image; the scene is moved along the ray of the window's centre
    "principal point far outside": (mm.intrinsics(1000, -2000.25, -1500.5), None),
}


@pytest.mark.parametrize("name", list(CAMERAS))
def test_cameras(name):
    H, W = 48, 64
    rng = np.random.default_rng(41)
    v, f = mm.random_scene(rng, 300)
    k, E = CAMERAS[name]
    if E is None:      # the scene's centre (0, 0, 3) goes to 40 d, d the ray of the window's centre: about 2.7 and 2 off the axis
        d = np.array([(W / 2 - k[0, 2]) / k[0, 0], (H / 2 - k[1, 2]) / k[1, 1], 1.0])
        E = np.eye(4)
        E[:3, 3] = 40 * d - [0, 0, 3]
    for cull in (False, True):
        _, _, got = gpu(v, f, k, E, H, W, cull)
        assert_bit_equal(got, mm.rasterize(v, f, k, E, H, W, cull_backfaces=cull), f"{name} cull={cull}")
        assert (got[0] >= 0).mean() > 0.1, "the mesh must be visible"


def test_mesh_wholly_off_screen():
    rng = np.random.default_rng(43)
    v, f = mm.random_scene(rng, 300)
    k = mm.intrinsics(40, 30, 25)
    for shift in ([50, 0, 0], [-50, 0, 0], [0, 50, 0], [0, -50, 0], [0, 0, -10]):       # right, left, below, above, behind
        r, _, (p2f, zb, bary) = gpu(v + np.float32(shift), f, k, np.eye(4), 50, 60)
        assert r.last_binned == 0, f"shift {shift}: {r.last_binned} entries binned for a mesh outside the image"
        assert np.all(p2f == -1) and np.all(zb == -1) and np.all(bary == -1)


# ------------------------------------------------------------------------------------------------ scale, exactly
def test_60k_faces_exactly():
    v, f = mm.sphere_grid(200, 150)
    assert len(f) == 60000
    H, W = 480, 640
    k, E = mm.intrinsics(500, 320.3, 240.2), mm.look_at([0.3, 0.4, -2.6], [0, 0, 0])
    r, _, got = gpu(v, f, k, E, H, W)
    assert r.last_binned > RADIX_TILE, "the sort must span more than one radix tile"
    assert (got[0] >= 0).mean() > 0.3
    rng = np.random.default_rng(5)
    i, j = np.mgrid[0:16, 0:16]
    tiles = [((ty * 16 + i) * W + tx * 16 + j).ravel() for ty, tx in ((15, 20), (4, 13))]     # the centre; on the silhouette
    pix = np.concatenate([rng.choice(H * W, 4096, replace=False)] + tiles)
    assert 0 < (got[0].ravel()[tiles[1]] >= 0).sum() < 256, "the second tile must straddle the silhouette"
    want = mm.rasterize(v, f, k, E, H, W, pixels=pix)
    sub = (got[0].ravel()[pix], got[1].ravel()[pix], got[2].reshape(-1, 3)[pix])
    assert_bit_equal(sub, want, "60 k faces")


# ------------------------------------------------------------------------------------------------ helpers
def test_helper_corner_cases():
    rng = np.random.default_rng(51)
    # a fan of 5000 faces on vertex 0, plus vertex V - 1 that no face uses
    n = 5000
    ang = np.sort(rng.uniform(0, 2 * np.pi, n + 1))
    rim = np.stack([np.cos(ang), np.sin(ang), 0.3 * rng.random(n + 1)], 1) * (1 + rng.random((n + 1, 1)))
    v = np.concatenate([[[0, 0, 1.0]], rim, [[7, 7, 7]]]).astype(np.float32)
    f = np.stack([np.zeros(n, int), 1 + np.arange(n), 2 + np.arange(n)], 1).astype(np.int32)
    f = f[rng.permutation(n)]
    r = mr().MeshRasterizer(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    got = r.vertex_normals().cpu().numpy()
    want = mm.vertex_normals(v, f)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "the fan's normal is not the fixed-order float32 sum"
    assert np.all(got[-1] == 0), "a vertex used by no face has the zero normal"
    assert abs(np.linalg.norm(got[0]) - 1) < 1e-6
    # interpolate with two channels
    k, E = mm.intrinsics(60, 24, 24), mm.look_at([0, 0, 4], [0, 0, 0])
    fr = r.rasterize(k, E, 48, 48)
    p2f, bary = fr.pix_to_face.cpu().numpy(), fr.bary_coords.cpu().numpy()
    assert (p2f >= 0).mean() > 0.2
    attr = rng.normal(size=(len(v), 2)).astype(np.float32)
    out = r.interpolate(fr, torch.from_numpy(attr).to(DEV)).cpu().numpy()
    assert out.shape == (48, 48, 2)
    assert np.array_equal(out.view(np.int32), mm.interpolate(f, p2f, bary, attr).view(np.int32))
    # a pix_to_face at or beyond F is refused by both helpers that read it
    for bad_id in (n, n + 7, 2 ** 31 - 1):
        bad = fr.pix_to_face.clone()
        bad[5, 6] = bad_id
        frb = mr().Fragments(bad, fr.zbuf, fr.bary_coords)
        with pytest.raises(ValueError):
            r.visible_faces(frb)
        with pytest.raises(ValueError):
            r.interpolate(frb, torch.from_numpy(attr).to(DEV))
    vis = r.visible_faces(fr).cpu().numpy()
    assert np.array_equal(vis, mm.visible_faces(p2f, n))


@pytest.mark.parametrize("V", [256, 257])
def test_vertex_normals_just_past_one_radix_tile(V):
    """4098 corners (one radix tile and two keys, no multiple of 256) sorted by a vertex id of 8 bits (one pass) and of
    9 bits (two passes)."""
    F = 1366
    assert 3 * F == RADIX_TILE + 2 and (3 * F) % 256 != 0
    rng = np.random.default_rng(60 + V)
    v = rng.normal(size=(V, 3)).astype(np.float32)
    f = rng.integers(0, V, size=(F, 3)).astype(np.int32)
    f[F // 2, 1], f[-1, 2] = V - 1, V - 1                    # the highest key, in the first tile and as the last corner
    r = mr().MeshRasterizer(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    got = r.vertex_normals().cpu().numpy()
    want = mm.vertex_normals(v, f)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "normals are not the fixed-order float32 sums"
