"""GPU tests of gaustudio_amd.mesh_init (csrc/gsr_mesh_bake.hip gsr_mesh_seeds) against the float32 model
tests/mesh_init_model.py: every field of the seeds is compared exactly (np.array_equal, NaN positions included).  The last
test composes the bake, the mesh renderer and the seeds."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mesh_init_model as mi  # noqa: E402
import mesh_raster_model as rm  # noqa: E402
import texture_bake_model as tm  # noqa: E402
from gaustudio_amd import formats, mesh_init, texture_bake  # noqa: E402
from gaustudio_amd.mesh_raster import MeshRasterizer  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
FIELDS = ("xyz", "f_dc", "f_rest", "opacity", "scale", "rot")


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(v, f, normals, colors, n, sh_degree=3):
    cloud = mesh_init.mesh_seeds(dev(v), dev(f), dev(colors), dev(normals), n_per_triangle=n, sh_degree=sh_degree)
    want = mi.seeds(v, f, normals, colors, n, sh_degree)
    for k in FIELDS:
        got = getattr(cloud, k).cpu().numpy()
        assert got.dtype == F32 and got.shape == want[k].shape, k
        assert np.array_equal(got, want[k], equal_nan=True), f"n = {n}: {k} differs from the model"
    assert np.isposinf(cloud.opacity.cpu().numpy()).all()
    return cloud, want


@pytest.mark.parametrize("n", [1, 3, 4, 6])
@pytest.mark.parametrize("with_colors", [True, False])
def test_equals_model(n, with_colors):
    v, f, nr, col = mi.random_mesh()
    cloud, want = check(v, f, nr, col if with_colors else None, n)
    assert cloud.num_points == 40 * n
    if not with_colors:
        assert (cloud.f_dc.cpu().numpy() == F32(0.5) / F32(mi.C0)).all()


@pytest.mark.parametrize("n", [1, 6])
def test_257_faces(n):
    """Just past one block of (face, k) items for n = 1; 1542 items for n = 6."""
    v, f, nr, col = mi.random_mesh(num_faces=257, num_verts=140, seed=12)
    check(v, f, nr, col, n, sh_degree=1)


@pytest.mark.parametrize("n", [1, 3, 4, 6])
def test_sign_cases(n):
    """One triangle per normal (1,0,0), (-1,0,0), (0,0,1), (0,1,0), (0,0,-1) and a generic one: R0 = 0, sign(n_z) = 0 ..."""
    normals = F32([[1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 1, 0], [0, 0, -1], [0.3, -0.5, 0.8]])
    rng = np.random.default_rng(2)
    v = rng.uniform(-1, 1, (18, 3)).astype(F32)
    f = np.arange(18, dtype=np.int32).reshape(6, 3)
    cloud, want = check(v, f, np.repeat(normals, 3, axis=0), None, n)
    rot = cloud.rot.cpu().numpy().reshape(6, n, 4)
    r = F32(np.sqrt(F32(1) + F32(1e-6)) / F32(2))
    assert (rot[0] == F32([r, 0, F32(1) / (F32(4) * r), 0])).all() and (rot[1] == F32([r, 0, F32(-1) / (F32(4) * r), 0])).all()
    assert (rot[2, :, 1:] == 0).all() and np.allclose(rot[2, :, 0], 1, atol=1e-6)
    assert (rot[3, :, 2:] == 0).all() and (rot[4, :, 1:] == 0).all() and np.isfinite(rot).all()


def test_zero_area_and_nan():
    v = F32([[0.5, 0.5, 0.5]] * 3 + [[0, 0, 0], [1, 0, 0], [np.nan, 1, 0]] + [[0, 0, 0], [2, 0, 0], [1, 0, 0]])
    f = np.arange(9, dtype=np.int32).reshape(3, 3)
    nr = F32([[0, 0, 1]] * 6 + [[0, 0, 0]] * 3)              # the last triangle: a zero normal stays zero through both normalisations
    cloud, want = check(v, f, nr, None, 3)
    scale = cloud.scale.cpu().numpy().reshape(3, 3, 3)
    assert (scale[0] == mi.log32(F32(1e-7))).all() and abs(float(scale[0, 0, 0]) - np.log(1e-7)) < 1e-5
    assert np.isnan(scale[1, :, :2]).all() and (scale[1, :, 2] == mi.log32(F32(1e-7))).all()
    assert np.isfinite(cloud.rot.cpu().numpy()[6:]).all()


def test_default_normals_and_errors():
    import torch
    v, f = rm.icosphere(1)
    cloud = mesh_init.mesh_seeds(dev(v), dev(f.astype(np.int64)))
    want = mi.seeds(v, f, rm.vertex_normals(v, f), None, 1)
    for k in FIELDS:
        assert np.array_equal(getattr(cloud, k).cpu().numpy(), want[k]), k
    bad = f.copy()
    bad[7, 1] = v.shape[0]
    with pytest.raises(ValueError):
        mesh_init.mesh_seeds(dev(v), dev(bad), vertex_normals=dev(v))
    with pytest.raises(ValueError):
        mesh_init.mesh_seeds(dev(v), dev(bad))
    empty = mesh_init.mesh_seeds(dev(v), torch.zeros((0, 3), dtype=torch.int32, device="cuda"), n_per_triangle=4)
    assert empty.num_points == 0 and empty.rot.shape == (0, 4) and empty.f_rest.shape == (0, 15, 3)


def test_formats_round_trip(tmp_path):
    v, f, nr, col = mi.random_mesh()
    cloud, want = check(v, f, nr, col, 3)
    path = str(tmp_path / "seeds.ply")
    formats.export_gaussian_ply(path, cloud)
    back = formats.load_gaussian_ply(path)
    for k in ("xyz", "opacity", "scale", "rot"):
        assert np.array_equal(getattr(back, k).numpy(), want[k]), k
    assert np.array_equal(back.f_dc.numpy().reshape(-1, 1, 3), want["f_dc"]) and np.isposinf(back.opacity.numpy()).all()
    assert back.max_sh_degree == 3 and not back.f_rest.numpy().any()


def test_bake_render_seed_composition():
    """The bake writes vertex colours; mesh_raster.interpolate re-renders them; mesh_seeds takes the same colours: the seeds'
    colours are the model's barycentric sums of the baked colours, the re-rendered image is the model's interpolation."""
    W, H = 48, 36
    v, f = rm.icosphere(2)
    views = []
    for a in range(4):
        t = 2 * np.pi * a / 4 + 0.3
        views.append((tm.random_image(H, W, seed=40 + a), tm.intrinsics(40.0, 40.0, W / 2, H / 2),
                      rm.look_at((3 * np.cos(t), 0.4, 3 * np.sin(t)), (0, 0, 0))))
    colors, baked_by, _ = texture_bake.bake_vertex_colors(dev(v), dev(f), [(dev(i), K, E) for i, K, E in views])
    baked = colors.cpu().numpy()
    assert (baked_by.cpu().numpy() >= 0).sum() > 100
    mesh = MeshRasterizer(dev(v), dev(f))
    _, K, E = views[0]
    frags = mesh.rasterize(K, E, H, W)
    image = mesh.interpolate(frags, colors).cpu().numpy()
    p2f, bary = frags.pix_to_face.cpu().numpy(), frags.bary_coords.cpu().numpy()
    assert np.array_equal(image, rm.interpolate(f, p2f, bary, baked)) and image[p2f >= 0].any()
    cloud = mesh_init.mesh_seeds(dev(v), dev(f), vertex_colors=colors, n_per_triangle=3)
    want = mi.rgb2sh(mi.bary_sum(baked, f, 3)).reshape(-1, 1, 3)
    assert np.array_equal(cloud.f_dc.cpu().numpy(), want)
    path_colors = texture_bake.bake_vertex_colors(dev(v), dev(f), [(dev(i), K, E) for i, K, E in views])[0]
    assert np.array_equal(path_colors.cpu().numpy(), baked)
