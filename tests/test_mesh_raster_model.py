"""The mesh rasterizer's numpy model (tests/mesh_raster_model.py) on closed-form cases, and its float32 replay against
the float64 model.  CPU only: these pin the contract the GPU tests hold the kernel to."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_raster_model as mm  # noqa: E402

I4 = np.eye(4)


def K(f, cx, cy, fy=None):
    return np.array([[f, 0, cx], [0, f if fy is None else fy, cy], [0, 0, 1]], dtype=np.float64)


def both(*args, **kw):
    return mm.rasterize(*args, dtype=np.float32, **kw), mm.rasterize(*args, dtype=np.float64, **kw)


def test_axis_aligned_triangle():
    # at z = 2 with f = 4, c = 4: u = 2 x + 4, so the triangle is (2,2), (6,2), (2,6) in pixels: centres with
    # j, i >= 2 and i + j <= 7 (an edge through centres is inclusive)
    v = np.array([[-1, -1, 2], [1, -1, 2], [-1, 1, 2]], dtype=np.float32)
    f = np.array([[0, 1, 2]], dtype=np.int32)
    for p2f, zb, bary in both(v, f, K(4, 4, 4), I4, 8, 8):
        i, j = np.mgrid[0:8, 0:8]
        want = (i >= 2) & (j >= 2) & (i + j <= 7)
        assert np.array_equal(p2f >= 0, want)
        assert np.allclose(zb[want], 2, rtol=1e-6) and np.all(zb[~want] == -1)
        assert np.allclose(bary[want].sum(-1), 1, atol=1e-6) and np.all(bary[~want] == -1)
        # barycentrics: pixel (2, 2) has its centre at (2.5, 2.5) -> x = y = -0.75
        assert np.allclose(bary[2, 2], [0.75, 0.125, 0.125], atol=1e-6)


def test_quad_diagonal_through_centres():
    # a quad covering the whole 6x6 image at z = 1, split along the diagonal j = i, which passes through pixel centres:
    # no hole, and the diagonal pixels go to face 0 (the lower id wins the exact z tie)
    v = np.array([[-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    for p2f, zb, _ in both(v, f, K(3, 3, 3), I4, 6, 6):
        i, j = np.mgrid[0:6, 0:6]
        assert np.all(p2f >= 0) and np.allclose(zb, 1, rtol=1e-6)
        assert np.all(p2f[j > i] == 0) and np.all(p2f[j < i] == 1) and np.all(p2f[j == i] == 0)


def cube(c=(0.0, 0.0, 5.0), h=1.0):
    v = np.array([[x, y, z] for z in (-h, h) for y in (-h, h) for x in (-h, h)], dtype=np.float64) + np.array(c)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]   # outward
    f = [(a, b, c_) for a, b, c_, d in quads] + [(a, c_, d) for a, b, c_, d in quads]
    return v.astype(np.float32), np.array(f, dtype=np.int32)


def test_cube_from_outside():
    v, f = cube()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    assert np.all(np.einsum("ij,ij->i", np.cross(b - a, c - a), a - v.mean(0)) > 0), "cube winding is outward"
    H = W = 40
    for p2f, zb, _ in both(v, f, K(40, 20, 20), I4, H, W):
        i, j = np.mgrid[0:H, 0:W]
        dx, dy = (j + 0.5 - 20) / 40, (i + 0.5 - 20) / 40
        m = np.maximum(abs(dx), abs(dy))
        inside, outside = m < 0.25 - 1e-3, m > 0.25 + 1e-3
        assert np.allclose(zb[inside], 4, rtol=1e-6) and np.all(p2f[outside] == -1)
        front = {0, 6}                                   # the z = 4 quad
        assert set(np.unique(p2f[inside])) <= front


def test_floor_crossing_camera_plane():
    # the plane y = 1 (below the camera in OpenCV axes), x in [-5, 5], z in [-5, 10]: rows with dy > 0 see it at z = 1 / dy
    # as long as z <= 10; the part behind the camera is never hit
    v = np.array([[-5, 1, -5], [5, 1, -5], [5, 1, 10], [-5, 1, 10]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    H, W = 30, 20
    p2f, zb, _ = mm.rasterize(v, f, K(10, 10, 15), I4, H, W, dtype=np.float64)
    i, j = np.mgrid[0:H, 0:W]
    dx, dy = (j + 0.5 - 10) / 10, (i + 0.5 - 15) / 10
    with np.errstate(divide="ignore"):
        z = 1 / dy
    want = (dy > 0) & (z <= 10) & (np.abs(dx * z) <= 5)
    assert np.array_equal(p2f >= 0, want)
    assert np.allclose(zb[want], z[want], rtol=1e-6)   # float32 output
    assert np.all(zb[want] > 0)
    # z_near cuts the near part off
    p2f2, zb2, _ = mm.rasterize(v, f, K(10, 10, 15), I4, H, W, z_near=2.0, dtype=np.float64)
    assert np.array_equal(p2f2 >= 0, want & (z > 2))
    p32, z32, _ = mm.rasterize(v, f, K(10, 10, 15), I4, H, W)
    assert np.array_equal(p32, p2f) and np.allclose(z32[want], z[want], rtol=1e-5)


def test_backface_culling():
    v = np.array([[-1, -1, 2], [1, -1, 2], [-1, 1, 2]], dtype=np.float32)
    front = np.array([[0, 2, 1]], dtype=np.int32)     # (b - a) x (c - a) = -z: towards the camera
    back = np.array([[0, 1, 2]], dtype=np.int32)
    k = K(4, 4, 4)
    assert (mm.rasterize(v, front, k, I4, 8, 8, cull_backfaces=True)[0] >= 0).sum() == 10
    assert (mm.rasterize(v, back, k, I4, 8, 8, cull_backfaces=True)[0] >= 0).sum() == 0
    assert (mm.rasterize(v, back, k, I4, 8, 8, cull_backfaces=False)[0] >= 0).sum() == 10
    # a closed outward mesh looks the same with and without culling from outside
    vc, fc = cube()
    a = mm.rasterize(vc, fc, K(40, 20, 20), I4, 40, 40, cull_backfaces=True)
    b = mm.rasterize(vc, fc, K(40, 20, 20), I4, 40, 40)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def random_mesh(rng, F, V=None):
    V = V or 3 * F
    v = rng.uniform(-1, 1, size=(V, 3)) * [1.0, 1.0, 0.6] + [0, 0, 3]
    return v.astype(np.float32), rng.integers(0, V, size=(F, 3)).astype(np.int32)


def test_float32_replay_against_float64():
    rng = np.random.default_rng(1)
    for trial in range(4):
        v, f = random_mesh(rng, 60)
        k = K(30, 17.3, 11.6, fy=33)
        E = mm.look_at(rng.normal(size=3) * 0.3, [0, 0, 3])
        (p32, z32, b32), (p64, z64, b64) = both(v, f, k, E, 24, 36, cull_backfaces=bool(trial % 2))
        # pixels away from near-ties agree exactly on the face; z and barycentrics to float32 precision
        e, z, okf = mm.face_setup(v, f, E, bool(trial % 2), np.float64)
        dx, dy = mm.pixel_rays(k, 24, 36, np.float64)
        with np.errstate(all="ignore"):
            Ek, ok, lam, zz = mm.hits(e[None], z[None], dx[:, None], dy[:, None], 0.0, np.float64)
            scale = np.abs(e).sum(-1)[None] * (np.abs(dx)[:, None, None] + np.abs(dy)[:, None, None] + 1)
            near_edge = ((np.abs(Ek) / scale) < 1e-5).any(-1).any(-1).reshape(24, 36)
            zs = np.sort(np.where(ok & okf[None], zz, np.inf), axis=1)
            near_z = (np.abs(zs[:, 1] - zs[:, 0]) < 1e-5 * np.abs(zs[:, 0])).reshape(24, 36)
        clean = ~near_edge & ~near_z
        assert clean.mean() > 0.8
        assert np.array_equal(p32[clean], p64[clean])
        h = clean & (p64 >= 0)
        assert np.allclose(z32[h], z64[h], rtol=1e-5)
        assert np.allclose(b32[h], b64[h], atol=1e-4)


def test_helpers_model():
    v, f = mm.icosphere(1)
    n = mm.vertex_normals(v, f)
    assert np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-6)
    assert np.all(np.einsum("ij,ij->i", n, v) > 0.95)          # outward, close to the radial direction
    E = mm.look_at([0, 0, -4], [0, 0, 0])
    p2f, zb, bary = mm.rasterize(v, f, K(50, 32, 32), E, 64, 64)
    pos = mm.interpolate(f, p2f, bary, v)
    assert np.all(pos[p2f < 0] == 0)
    assert np.allclose(np.linalg.norm(pos[p2f >= 0], axis=-1), 1, atol=0.1)
    nm = mm.normal_map(f, p2f, n, E)
    # seen from outside, the normals face the camera: camera-space z < 0, so the negated z of render_mesh.py is > 0
    assert np.all(nm[p2f >= 0][:, 2] > 0)
    # one flat normal per face (render_mesh.py interpolates with barycentrics of ones), not a smooth interpolation
    for face in np.unique(p2f[p2f >= 0]):
        px = nm[p2f == face]
        assert np.all(px == px[0])
    smooth = mm.interpolate(f, p2f, bary, n)[p2f >= 0]
    smooth = smooth / np.linalg.norm(smooth, axis=-1, keepdims=True)
    c2w_R = np.linalg.inv(E)[:3, :3]
    assert np.abs(smooth @ c2w_R * [1, -1, -1] - nm[p2f >= 0]).max() > 1e-2
    vis = mm.visible_faces(p2f, len(f))
    assert 0 < vis.sum() < len(f)


# ------------------------------------------------------------------------------------------------ culls on hard shapes
def cull_report(v, f, k, E, H, W, z_near, chunk=256):
    """Brute force over every (pixel, face) pair with the rectangle ignored, against face_setup's culls: the number of
    float32 hits, of hits outside their face's padded pixel rectangle (with the farthest, in pixels), of hits on a face
    that is not binned at all (culled, or its rectangle misses the image) and of hits whose z lies below the face's key."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        vc = mm.camera_space(v, E, f32)
        e, z, okf = mm.face_setup(v, f, E, False, f32)
        rect, okr = mm.pixel_rect(vc, f, k, H, W, z_near)
        key = mm.face_key(vc, f, z_near)
        dx, dy = mm.pixel_rays(k, H, W, f32)
        i, j = np.divmod(np.arange(H * W), W)
        rep = dict(hits=0, outside=0, worst=0, culled=0, below_key=0)
        for f0 in range(0, len(f), chunk):
            s = slice(f0, f0 + chunk)
            _, ok, _, zz = mm.hits(e[None, s], z[None, s], dx[:, None], dy[:, None], z_near, f32)
            ok &= okf[None, s]
            r = rect[s]
            out = ok & okr[None, s] & ~mm.in_rect(r, i, j)
            rep["hits"] += int(ok.sum())
            rep["outside"] += int(out.sum())
            rep["culled"] += int((ok & ~okr[None, s]).sum())
            rep["below_key"] += int((ok & (zz < key[None, s])).sum())
            if out.any():
                d = np.maximum(np.maximum(r[None, :, 0] - j[:, None], j[:, None] - r[None, :, 2]),
                               np.maximum(r[None, :, 1] - i[:, None], i[:, None] - r[None, :, 3]))
                rep["worst"] = max(rep["worst"], int(d[out].max()))
    return rep


NEEDLE_H, NEEDLE_W, NEEDLE_F = 64, 80, 3000


@pytest.mark.parametrize("row", range(len(mm.NEEDLES_WELL)))
def test_needles_stay_inside_their_rectangle(row):
    # the float32 cross products of the first version put up to 3340 of these hits as far as 70 px outside the rectangle
    # (2350 outside the tile rectangle: lost by the kernel); formed in float64 and rounded once, none leaves it
    v, f, k = mm.needles(np.random.default_rng(1000 + row), NEEDLE_F, NEEDLE_H, NEEDLE_W, *mm.NEEDLES_WELL[row])
    rep = cull_report(v, f, k, I4, NEEDLE_H, NEEDLE_W, 0.0)
    print(mm.NEEDLES_WELL[row], rep)
    assert rep["hits"] > 100
    assert rep["outside"] == 0 and rep["culled"] == 0, rep
    assert rep["below_key"] == 0, rep


@pytest.mark.parametrize("row", range(len(mm.NEEDLES_PATHOLOGICAL)))
def test_pathological_needles_are_clipped_by_the_rectangle(row):
    # no fixed pad covers needles a few thousandths of a pixel wide 8000 px off-axis: here the rectangle is what defines
    # the image, and the GPU test on the same sets exercises the clip only because these counts are not zero
    v, f, k = mm.needles(np.random.default_rng(2000 + row), NEEDLE_F, NEEDLE_H, NEEDLE_W, *mm.NEEDLES_PATHOLOGICAL[row])
    rep = cull_report(v, f, k, I4, NEEDLE_H, NEEDLE_W, 0.0)
    print(mm.NEEDLES_PATHOLOGICAL[row], rep)
    assert rep["outside"] + rep["culled"] >= 1, rep
    assert rep["below_key"] == 0, rep
    # and rasterize applies it: no pixel shows a face outside the face's rectangle
    p2f = mm.rasterize(v, f, k, I4, NEEDLE_H, NEEDLE_W)[0]
    rect, okr = mm.pixel_rect(mm.camera_space(v, I4, np.float32), f, k, NEEDLE_H, NEEDLE_W, 0.0)
    i, j = np.nonzero(p2f >= 0)
    r = rect[p2f[i, j]]
    assert okr[p2f[i, j]].all()
    assert np.all((j >= r[:, 0]) & (j <= r[:, 2]) & (i >= r[:, 1]) & (i <= r[:, 3]))


HARD_K = mm.intrinsics(70.3, 39.7, 31.2, fy=66.1)


def hard_shapes():
    rng = np.random.default_rng(0)
    F = 1500
    v, f = mm.radial_edge_faces(rng, F)
    yield "radial edges", v, f, 0.0
    yield "radial edges x 1000", (v * 1000).astype(np.float32), f, 0.0
    v, f = mm.camera_plane_faces(rng, F)
    for zn in (0.0, 0.05, 0.5):
        yield f"camera plane z_near={zn}", v, f, zn
    v, f = mm.edge_on_faces(rng, F)
    yield "edge-on", v, f, 0.0
    yield "edge-on z_near=0.5", v, f, 0.5


@pytest.mark.parametrize("name,v,f,z_near", [pytest.param(*s, id=s[0]) for s in hard_shapes()])
def test_culls_hold_on_hard_shapes(name, v, f, z_near):
    rep = cull_report(v, f, HARD_K, I4, 64, 80, z_near)
    print(name, rep)
    assert rep["hits"] > 0     # (a face through the camera centre covers every ray at z near 0: few are left at z_near = 0.5)
    assert rep["outside"] == 0, rep
    assert rep["culled"] == 0, rep
    assert rep["below_key"] == 0, rep


def test_camera_plane_set_has_the_vertices_it_claims():
    v, f = mm.camera_plane_faces(np.random.default_rng(0), 1500)
    z = v[f][:, :, 2]
    assert (z == 0).any(1).sum() > 100 and (z == np.float32(1e-30)).any(1).sum() > 100 and (z == np.float32(-1e-30)).any(1).sum() > 100
    assert ((z.min(1) < 0) & (z.max(1) > 0)).sum() > 300


def test_watertight_sliver_sphere_off_axis():
    # a closed mesh of slivers (2048 longitudes x 8 latitudes, pole fans) in the corner of a wide render: every pixel
    # strictly inside the float64 silhouette is covered, the rectangle applied
    from scipy.spatial import ConvexHull
    v, f = mm.sliver_sphere(2048, 8)
    assert len(f) == 2 * 2048 * 8
    a, b, c = (v[f[:, n]].astype(np.float64) for n in range(3))
    assert np.all(np.einsum("ij,ij->i", np.cross(b - a, c - a), a + b + c) > 0), "outward winding"
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    assert np.all(np.unique(edges, axis=0, return_counts=True)[1] == 2), "closed: every edge is shared by two faces"
    H, W = 64, 80
    k = mm.intrinsics(1500, -1000, -800)
    # the window looks at the region of the north pole (its fan of 2048 needles, the silhouette and background): the
    # sphere spans about 200 px, its centre lies on the ray of the window's centre moved 0.8 radii along the sphere's axis
    d = np.array([(W / 2 + 1000) / 1500, (H / 2 + 800) / 1500, 1.0])
    E = np.eye(4)
    E[:3, 3] = d * 15.0 - [0, 0.8, 0]
    vc = mm.camera_space(v, E, np.float64)
    uv = np.stack([k[0, 0] * vc[:, 0] / vc[:, 2] + k[0, 2], k[1, 1] * vc[:, 1] / vc[:, 2] + k[1, 2]], axis=1)
    assert np.all((uv[-2] > [4, 4]) & (uv[-2] < [W - 4, H - 4])), "the north pole is in the window"
    hull = ConvexHull(uv)
    i, j = np.mgrid[0:H, 0:W]
    ctr = np.stack([j.ravel() + 0.5, i.ravel() + 0.5], axis=1)
    inside = (ctr @ hull.equations[:, :2].T + hull.equations[:, 2] < -1e-3).all(1).reshape(H, W)
    assert 1000 < inside.sum() < H * W - 200, "the window holds silhouette and background"
    p2f, zb, _ = mm.rasterize(v, f, k, E, H, W)
    holes = inside & (p2f < 0)
    assert not holes.any(), f"{holes.sum()} background pixels inside the silhouette"
    assert np.all(p2f[~inside & (p2f >= 0)] >= 0) and len(np.unique(p2f[inside])) > 500     # slivers: many faces show


def shifted_pair(v, f, k, E, H, W, render):
    """render(...) with (cx, cy), W x H and with (cx + 5, cy + 3), (W + 5) x (H + 3): the same rays fall on another place of
    the 16 x 16 tile grid.  Returns the outputs at corresponding pixels."""
    k2 = k.copy()
    k2[0, 2] += 5
    k2[1, 2] += 3
    a = render(v, f, k, E, H, W)
    b = render(v, f, k2, E, H + 3, W + 5)
    return a, tuple(x[3:, 5:] for x in b)


def tile_grid_scenes():
    rng = np.random.default_rng(11)
    yield "random", mm.random_scene(rng, 300) + (mm.intrinsics(45, 20.5, 17.0, fy=50), mm.look_at([0.1, -0.1, 0], [0, 0, 3]), 37, 53)
    yield "crossing", mm.random_scene(rng, 300, crossing=True) + (mm.intrinsics(45, 20.5, 17.0, fy=50), np.eye(4), 37, 53)
    yield "needles", mm.needles(rng, 1000, 37, 53, *mm.NEEDLES_PATHOLOGICAL[0]) + (np.eye(4), 37, 53)


@pytest.mark.parametrize("name,scene", [pytest.param(*s, id=s[0]) for s in tile_grid_scenes()])
def test_tile_grid_independence(name, scene):
    v, f, k, E, H, W = scene
    assert np.all(k[:2, 2] * 2 == np.round(k[:2, 2] * 2)), "(j + 0.5) - cx must be exact"
    a, b = shifted_pair(v, f, k, E, H, W, mm.rasterize)
    assert (a[0] >= 0).sum() > 15          # (needles cover little)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
