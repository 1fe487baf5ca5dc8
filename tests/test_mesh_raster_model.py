"""The mesh rasterizer's numpy model (tests/mesh_raster_model.py) on closed-form cases, and its float32 replay against
the float64 model.  CPU only: these pin the contract the GPU tests hold the kernel to."""
import os
import sys

import numpy as np

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
