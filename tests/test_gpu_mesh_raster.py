"""The HIP mesh rasterizer (gaustudio_amd.mesh_raster over csrc/gsr_mesh.hip) against its numpy model
(tests/mesh_raster_model.py): bit-equality with the float32 replay, watertightness, bad input, run-to-run identity, the
helpers, a 2 M-face mesh at 1080p against the float64 model, and the render -> TSDF -> mesh -> render round trip."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_raster_model as mm  # noqa: E402
from mesh_raster_model import random_scene, sphere_grid  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def mr():
    from gaustudio_amd import mesh_raster
    return mesh_raster


def K(f, cx, cy, fy=None):
    return np.array([[f, 0, cx], [0, f if fy is None else fy, cy], [0, 0, 1]], dtype=np.float64)


def gpu(v, f, k, E, H, W, cull=False, z_near=0.0):
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    r = mr().MeshRasterizer(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    fr = r.rasterize(k, E, H, W, cull_backfaces=cull, z_near=z_near)
    return r, fr, tuple(t.cpu().numpy() for t in fr)


def assert_bit_equal(got, want, what=""):
    names = ("pix_to_face", "zbuf", "bary")
    for n, a, b in zip(names, got, want):
        assert a.shape == b.shape, f"{what} {n} shape"
        same = a.view(np.int32) == b.view(np.int32)
        assert same.all(), f"{what} {n}: {np.count_nonzero(~same)} values differ from the float32 replay"


@pytest.mark.parametrize("case", range(8))
def test_bit_equal_to_float32_replay(case):
    rng = np.random.default_rng(100 + case)
    H, W = [(48, 64), (37, 53), (64, 40), (33, 33)][case % 4]
    crossing = case >= 4
    v, f = random_scene(rng, 300, crossing)
    k = K(40 + 10 * rng.random(), W * (0.3 + 0.4 * rng.random()), H * (0.3 + 0.4 * rng.random()), fy=45 + 10 * rng.random())
    E = mm.look_at(rng.normal(size=3) * 0.2, [0, 0, 3]) if not crossing else np.eye(4)
    for cull in (False, True):
        for z_near in ((0.0,) if not crossing else (0.0, 0.5)):
            _, _, got = gpu(v, f, k, E, H, W, cull, z_near)
            want = mm.rasterize(v, f, k, E, H, W, cull_backfaces=cull, z_near=z_near)
            assert_bit_equal(got, want, f"case {case} cull={cull} z_near={z_near}")
            assert (got[0] >= 0).mean() > 0.2


def test_watertight_icosphere():
    from scipy.spatial import ConvexHull
    v, f = mm.icosphere(5)
    assert len(f) >= 20000
    H, W = 300, 400
    k = K(350, 211.3, 147.9)
    E = mm.look_at([0.3, 0.2, -3.0], [0, 0, 0])
    _, _, (p2f, zb, _) = gpu(v, f, k, E, H, W)
    vc = mm.camera_space(v, E, np.float64)
    uv = np.stack([k[0, 0] * vc[:, 0] / vc[:, 2] + k[0, 2], k[1, 1] * vc[:, 1] / vc[:, 2] + k[1, 2]], axis=1)
    hull = ConvexHull(uv)
    i, j = np.mgrid[0:H, 0:W]
    c = np.stack([j.ravel() + 0.5, i.ravel() + 0.5], axis=1)
    inside = (c @ hull.equations[:, :2].T + hull.equations[:, 2] < -1e-3).all(1).reshape(H, W)
    assert inside.sum() > 30000
    holes = inside & (p2f < 0)
    assert not holes.any(), f"{holes.sum()} background pixels inside the silhouette"
    # the front half only: every visible face faces the camera
    assert np.all(zb[inside] < 3.0)


def test_watertight_grid_through_pixel_centres():
    # f = 2 at z = 2 with c = 0: vertex (x, y) lands on pixel (x - 0.5, y - 0.5) exactly; vertices at x, y = 0.5 + n put every
    # mesh edge and vertex through pixel centres
    H, W = 40, 48
    v, f = mm.grid_mesh(30, 20, 4.5, 6.5, 1.0, 2.0)
    k = K(2, 0, 0)
    for cull in (False, True):
        for ff in (f, f[:, ::-1]):
            _, _, got = gpu(v, ff, k, np.eye(4), H, W, cull)
            want = mm.rasterize(v, ff, k, np.eye(4), H, W, cull_backfaces=cull)
            assert_bit_equal(got, want, "grid")
            p2f = got[0]
            front = (mm.face_setup(v, ff, np.eye(4), True, np.float32)[2]).all()
            if cull and not front:
                assert np.all(p2f < 0)
                continue
            i, j = np.mgrid[0:H, 0:W]
            inside = (j >= 4) & (j <= 34) & (i >= 6) & (i <= 26)
            assert np.all(p2f[inside] >= 0), "hole in a grid whose edges pass through pixel centres"
            assert np.all(p2f[~inside] < 0)
    # the tie rule: where several faces give the same (least) z, the lowest id wins
    e, z, okf = mm.face_setup(v, f, np.eye(4), False, np.float32)
    dx, dy = mm.pixel_rays(k, H, W, np.float32)
    _, ok, _, zz = mm.hits(e[None], z[None], dx[:, None], dy[:, None], 0.0, np.float32)
    zz = np.where(ok, zz, np.inf)
    zmin = zz.min(1)
    tie = np.isfinite(zmin) & ((zz == zmin[:, None]).sum(1) > 1)
    assert tie.sum() > 100
    low = np.argmax(zz == zmin[:, None], axis=1)
    p2f = gpu(v, f, k, np.eye(4), H, W)[2][0].ravel()
    assert np.array_equal(p2f[tie], low[tie])


def test_bad_input():
    rng = np.random.default_rng(7)
    v, f = random_scene(rng, 200)
    v[5] = np.nan
    v[6] = [np.inf, 0, 3]
    f[:10, 1] = 5                          # NaN vertex
    f[10:20, 2] = 6                        # inf vertex
    f[20:30, 1] = f[20:30, 0]              # repeated index
    v[7] = v[8]
    f[30:40, 0], f[30:40, 1] = 7, 8        # coincident vertices
    k, E = K(40, 30, 25), mm.look_at([0, 0, 0], [0, 0, 3])
    _, _, got = gpu(v, f, k, E, 50, 60)
    assert_bit_equal(got, mm.rasterize(v, f, k, E, 50, 60), "bad input")
    assert not np.isin(got[0], np.arange(40)).any(), "a degenerate or non-finite face was hit"
    # empty meshes
    for vv, ff in ((v, np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))):
        _, _, (p2f, zb, bary) = gpu(vv, ff, k, E, 20, 30)
        assert np.all(p2f == -1) and np.all(zb == -1) and np.all(bary == -1)
    # out-of-range indices raise
    for bad in (len(v), -1):
        fb = f.copy()
        fb[17, 2] = bad
        with pytest.raises(ValueError):
            gpu(v, fb, k, E, 20, 30)
    with pytest.raises(ValueError):
        gpu(v, f, K(0, 30, 25), E, 20, 30)
    with pytest.raises(ValueError):
        gpu(v, f, k, E, 20, 30, z_near=-1.0)
    r = mr().MeshRasterizer(torch.from_numpy(v).to(DEV), torch.from_numpy(f.astype(np.int64)).to(DEV))
    assert r.faces.dtype == torch.int32
    with pytest.raises(RuntimeError):
        mr().MeshRasterizer(torch.from_numpy(v), torch.from_numpy(f))          # CPU tensors: no fallback


def test_run_to_run_identical():
    v, f = mm.icosphere(4)
    r = mr().MeshRasterizer(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    k, E = K(300, 160.2, 120.7), mm.look_at([0.5, 0.4, -2.5], [0, 0, 0])
    a = [t.cpu().numpy() for t in r.rasterize(k, E, 240, 320)]
    for _ in range(3):
        b = [t.cpu().numpy() for t in r.rasterize(k, E, 240, 320)]
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))
    n1 = r.vertex_normals().cpu().numpy()
    r._normals = None
    assert np.array_equal(n1.view(np.int32), r.vertex_normals().cpu().numpy().view(np.int32))


def test_helpers_against_model():
    v, f = mm.icosphere(3)
    rng = np.random.default_rng(3)
    v = (v * (1 + 0.1 * rng.random((len(v), 1)))).astype(np.float32)
    k, E = K(200, 100.4, 80.1), mm.look_at([0.2, -0.5, -3.0], [0, 0, 0])
    r, fr, (p2f, zb, bary) = gpu(v, f, k, E, 160, 200)
    n = r.vertex_normals().cpu().numpy()
    nm = mm.vertex_normals(v, f)
    assert np.array_equal(n.view(np.int32), nm.view(np.int32)), "vertex normals differ from the fixed-order float32 sum"
    for C in (1, 3, 4):
        attr = rng.normal(size=(len(v), C)).astype(np.float32)
        got = r.interpolate(fr, torch.from_numpy(attr).to(DEV)).cpu().numpy()
        assert np.array_equal(got.view(np.int32), mm.interpolate(f, p2f, bary, attr).view(np.int32))
    got = r.normal_map(fr, E).cpu().numpy()
    want = mm.normal_map(f, p2f, nm, E)
    assert np.allclose(got, want, atol=1e-5)
    assert np.all(got[p2f < 0] == 0)
    vis = r.visible_faces(fr).cpu().numpy()
    assert np.array_equal(vis, mm.visible_faces(p2f, len(f)))
    # texture_mesh.py get_visible_faces: the sorted unique ids of pix_to_face without -1
    assert np.array_equal(np.nonzero(vis)[0], np.unique(p2f[p2f >= 0]))
    with pytest.raises(ValueError):
        r.interpolate(fr, torch.zeros((len(v), 5), device=DEV))
    # fragments that are not device tensors of the rasterizer's dtypes are refused before any kernel sees them
    cpu = mr().Fragments(*(t.cpu() for t in fr))
    attr = torch.zeros((len(v), 3), device=DEV)
    for call in (lambda: r.interpolate(cpu, attr), lambda: r.visible_faces(cpu), lambda: r.normal_map(cpu, E)):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(TypeError):
        r.visible_faces(mr().Fragments(fr.pix_to_face.long(), fr.zbuf, fr.bary_coords))
    with pytest.raises(TypeError):
        r.interpolate(mr().Fragments(fr.pix_to_face, fr.zbuf, fr.bary_coords.double()), attr)


def test_normal_map_is_flat_per_face_as_render_mesh():
    # render_mesh.py's get_normals_from_fragments interpolates the face's vertex normals with barycentrics of ones: each pixel
    # gets the normalised sum of its face's three vertex normals.  On a coarse icosphere that differs clearly from a
    # barycentric (smooth) interpolation
    v, f = mm.icosphere(1)
    k, E = K(120, 64.3, 48.2), mm.look_at([0.3, 0.2, -3.0], [0, 0, 0])
    r, fr, (p2f, _, bary) = gpu(v, f, k, E, 96, 128)
    got = r.normal_map(fr, E).cpu().numpy()
    vn = mm.vertex_normals(v, f)
    assert np.allclose(got, mm.normal_map(f, p2f, vn, E), atol=1e-6)
    hit = p2f >= 0
    for face in np.unique(p2f[hit]):
        px = got[p2f == face]
        assert np.all(px == px[0]), f"face {face}: the normal varies across the face"
    smooth = mm.interpolate(f, p2f, bary, vn)[hit]
    smooth = smooth / np.linalg.norm(smooth, axis=-1, keepdims=True)
    smooth = smooth @ np.linalg.inv(E)[:3, :3] * [1, -1, -1]
    assert np.abs(smooth - got[hit]).max() > 1e-2


def test_negative_zero_camera_z_keeps_its_place_in_the_tile_order():
    # a vertex at camera z = -0 (R row and translation -0, the vertex's z -0): its face's sort key must be +0, not the bit
    # pattern 0x80000000 that would sort it after every other face of the tile and let the early stop skip it
    E = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [-0.0, -0.0, 1, -0.0], [0, 0, 0, 1]], dtype=np.float64)
    v = np.array([[-9, -9, 2], [9, -9, 2], [0, 9, 2],           # face 0: a wall at z = 2 over the whole image
                  [-9, -9, 5], [9, -9, 5], [0, 9, 5],           # face 1: a wall at z = 5 (key 5)
                  [0.2, 0.1, -0.0], [-1, -1, 1], [1, -1, 1]],   # face 2: from camera z = -0 to z = 1, in front of both
                 dtype=np.float32)
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], dtype=np.int32)
    assert np.signbit(mm.camera_space(v, E, np.float32)[6, 2])
    k = K(20, 16, 16)
    _, _, got = gpu(v, f, k, E, 32, 32)
    assert_bit_equal(got, mm.rasterize(v, f, k, E, 32, 32), "-0 key")
    assert (got[0] == 2).sum() > 20


def test_large_mesh_1080p_against_float64_model():
    v, f = sphere_grid(1024, 1000)
    assert len(f) >= 2_000_000
    H, W = 1080, 1920
    k, E = K(1500, 960.3, 540.2), mm.look_at([0.3, 0.4, -2.6], [0, 0, 0])
    _, _, (p2f, zb, bary) = gpu(v, f, k, E, H, W)
    assert (p2f >= 0).mean() > 0.3
    rng = np.random.default_rng(5)
    hitpix = np.flatnonzero(p2f.ravel() >= 0)
    pix = np.concatenate([rng.choice(hitpix, 192, replace=False), rng.choice(H * W, 64, replace=False)])
    p64, z64, _ = mm.rasterize(v, f, k, E, H, W, dtype=np.float64, pixels=pix)
    e, z, _ = mm.face_setup(v, f, E, False, np.float64)
    vn = np.linalg.norm(mm.camera_space(v, E, np.float64), axis=1)[f]
    dx, dy = mm.pixel_rays(k, H, W, np.float64, pix)
    g = p2f.ravel()[pix]
    bad = []
    for n in np.flatnonzero(g != p64):
        cand = [x for x in (g[n], p64[n]) if x >= 0]
        Ek, ok, _, zz = mm.hits(e[cand][None], z[cand][None], dx[n:n + 1, None], dy[n:n + 1, None], 0.0, np.float64)
        # the size of an E_k's float32 error: the cross product of two vertices of about |v| (and the ray's length)
        scale = (vn[cand][:, [1, 2, 0]] * vn[cand][:, [2, 0, 1]]) * np.sqrt(dx[n] ** 2 + dy[n] ** 2 + 1)
        near_edge = (np.abs(Ek[0]) <= 1e-5 * scale).any()
        near_z = len(cand) == 2 and abs(zz[0, 0] - zz[0, 1]) <= 1e-5 * abs(zz[0]).max()
        if not (near_edge or near_z):
            bad.append(int(pix[n]))
    assert not bad, f"pixels {bad} differ from the float64 model without a near-tie"
    h = (g >= 0) & (g == p64)
    rel = np.abs(zb.ravel()[pix][h] / z64[h] - 1)
    assert np.median(rel) < 1e-6 and rel.max() < 1e-3


def test_round_trip_operator_tsdf_mesh():
    from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, postprocess as pp, scenes
    from gaustudio_amd.tsdf import TSDFVolume
    g_ = torch.Generator().manual_seed(0)
    P = 60000
    d = torch.randn(P, 3, generator=g_)
    d = d / d.norm(dim=1, keepdim=True)
    means = d.to(DEV)
    scales = torch.full((P, 3), 0.012, device=DEV)
    rots = torch.tensor([[1.0, 0, 0, 0]], device=DEV).repeat(P, 1)
    opac = torch.full((P, 1), 0.95, device=DEV)
    cols = torch.rand(P, 3, generator=g_).to(DEV)
    voxel = 0.02
    vol = TSDFVolume(voxel, 4 * voxel, capacity_blocks=1 << 15)
    views = []
    for cam in scenes.ring_cameras(12, 320, 240, radius=3.0, elevation=0.3) + scenes.ring_cameras(6, 320, 240, radius=3.0, elevation=-0.9):
        rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0,
                                           cam.viewmatrix.to(DEV), cam.projmatrix.to(DEV), 0, cam.campos.to(DEV), False, False)
        with torch.no_grad():
            _, _, _, median, opacity = GaussianRasterizer(rs)(means3D=means, means2D=torch.zeros_like(means), opacities=opac,
                                                               colors_precomp=cols, scales=scales, rotations=rots)
        depth = median[0].clone()
        invalid = opacity[0] < 0.5
        depth[invalid] = 0
        f = cam.width / (2 * cam.tanfovx)
        Kc = torch.tensor([[f, 0, cam.width / 2], [0, f, cam.height / 2], [0, 0, 1]])
        E = cam.viewmatrix.t().contiguous()
        vol.integrate(pp.depth_to_points(depth, Kc, E, "world"), cam.campos)
        views.append((Kc, E, depth, cam.height, cam.width))
    verts, faces = vol.extract_triangle_mesh_device(min_weight=2)
    r = mr().MeshRasterizer(verts, faces)                     # the device mesh goes in as it is
    # depth_to_points unprojects pixel (i, j) at the integer coordinates (j, i) (Camera.depth2point's grid), while the mesh
    # rays go through the centres (j + 0.5, i + 0.5).  Rendered with cx + 0.5, cy + 0.5 the mesh rays are the very rays whose
    # depths were fused; with the plain intrinsics the two maps sample rays half a pixel apart.  Both are checked.  Measured:
    # about 97.4 % (fused rays) and 97.3 % (pixel-centre rays) of all pixels valid in both agree within 2 voxels, 99.8 % and
    # 99.9 % away from a 2-px band along the silhouettes -- so the half-pixel offset is not what the misses are: they are
    # silhouette pixels, where the ray grazes the surface and a sub-voxel difference between the fused surface and the
    # Gaussians' median depth moves the depth along the ray by many voxels.  The issue's 99 % over all pixels valid in both
    # is therefore asserted away from the silhouettes only, and 95 % over all of them.
    for cull in (False, True):
        stats = {}
        for shift in (0.5, 0.0):
            agree = total = agree_in = total_in = 0
            for Kc, E, depth, H, W in views:
                Ks = Kc.clone()
                Ks[0, 2] += shift
                Ks[1, 2] += shift
                fr = r.rasterize(Ks, E, H, W, cull_backfaces=cull)
                both = (fr.pix_to_face >= 0) & (depth > 0)
                close = (fr.zbuf - depth).abs() <= 2 * voxel
                inner = -torch.nn.functional.max_pool2d(-both[None, None].float(), 5, stride=1, padding=2)[0, 0] > 0.5
                total += int(both.sum())
                agree += int(close[both].sum())
                total_in += int(inner.sum())
                agree_in += int(close[inner].sum())
                assert both.sum() >= 0.95 * (depth > 0).sum()      # the fused surface covers what the operator saw
            stats[shift] = (agree / total, agree_in / total_in, total)
        print(f"cull={cull}: within 2 voxels, all / away from silhouettes: aligned rays {stats[0.5][:2]}, "
              f"pixel-centre rays {stats[0.0][:2]}")
        for shift, (frac_all, frac_in, total) in stats.items():
            assert total > 100000
            assert frac_in >= 0.99, f"cull={cull}, shift {shift}: {frac_in:.4f} away from silhouettes within 2 voxels"
            assert frac_all >= 0.95, f"cull={cull}, shift {shift}: {frac_all:.4f} of all pixels valid in both within 2 voxels"
