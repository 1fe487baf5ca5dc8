"""GPU tests of gaustudio_amd.voxelize (csrc/gsr_voxel.hip) against the float64 model tests/mesh_voxel_model.py.  Every
comparison with the model is exact (np.array_equal): voxel_index, pair_start, pair_tri, closest_tri, closest_uvw (float64
bits) and color -- the library is built without contraction, float64 divides are correctly rounded, and the model performs the
kernels' operations in their order."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mesh_voxel_model as mm  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MB, XB = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)


def _torch():
    import torch
    return torch


def dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_run(vn, faces, vs, min_bound=MB, max_bound=XB, colors=None, closest=True):
    """The voxelization and the closest triangles of the device as numpy arrays."""
    from gaustudio_amd import voxelize as vx
    grid = vx.voxelize_mesh(dev(vn), dev(faces), vs, min_bound, max_bound, return_occupancy=True)
    t = _torch()
    assert all(a.dtype == t.int32 for a in (grid.grid_index, grid.voxel_index, grid.pair_start, grid.pair_tri, grid.occupancy))
    out = {k: getattr(grid, k).cpu().numpy() for k in ("grid_index", "voxel_index", "pair_start", "pair_tri", "occupancy")}
    out["shape"], out["grid"], out["centers"] = grid.shape, grid, grid.centers().cpu().numpy()
    if closest:
        near = vx.closest_on_mesh(grid, dev(vn), dev(faces), None if colors is None else dev(colors))
        assert near["closest_tri"].dtype == t.int32 and near["closest_uvw"].dtype == t.float64
        out.update({k: v.cpu().numpy() for k, v in near.items()})
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(got, want_vox, want_near=None, what=""):
    assert got["shape"] == tuple(want_vox["shape"])
    for k in ("voxel_index", "pair_start", "pair_tri", "grid_index"):
        assert np.array_equal(got[k], want_vox[k]), f"{what}{k} differs"
    nn = int(np.prod(got["shape"]))
    bits = np.zeros(((nn + 31) // 32) * 32, dtype=bool)
    bits[want_vox["voxel_index"]] = True
    assert np.array_equal(np.unpackbits(got["occupancy"].view(np.uint8), bitorder="little").astype(bool), bits), f"{what}occupancy"
    if want_near is not None:
        assert np.array_equal(got["closest_tri"], want_near["closest_tri"]), f"{what}closest_tri differs"
        assert got["closest_uvw"].dtype == np.float64 and same_bits(got["closest_uvw"], want_near["closest_uvw"]), f"{what}closest_uvw"
        if "color" in want_near:
            assert got["color"].dtype == F and same_bits(got["color"], want_near["color"]), f"{what}color differs"


def model_run(vn, faces, vs, min_bound=MB, max_bound=XB, colors=None, closest=True, slab=8):
    shape = mm.grid_shape(vs, min_bound, max_bound)
    vox = mm.voxelize_boxed(vn, faces, vs, min_bound, shape, slab=slab)
    return vox, (mm.closest(vox, vn, faces, vs, min_bound, colors) if closest else None)


def check(vn, faces, vs, min_bound=MB, max_bound=XB, colors=None, closest=True):
    got = gpu_run(vn, faces, vs, min_bound, max_bound, colors, closest)
    vox, near = model_run(vn, faces, vs, min_bound, max_bound, colors, closest)
    assert_same(got, vox, near)
    return got, vox, near


# ---------------------------------------------------------------------------------------------- 1. the three model cases
@pytest.mark.parametrize("name", ["icosphere16", "ellipsoid24", "soup16"])
def test_equals_model(name):
    make, n = {"icosphere16": (lambda: mm.icosphere(1), 16), "ellipsoid24": (mm.ellipsoid, 24), "soup16": (mm.soup, 16)}[name]
    v, f = make()
    from gaustudio_amd import voxelize as vx
    vn_dev, scale, center = vx.normalize_mesh(dev(v))
    vn, mscale, mcenter = mm.normalize_mesh(v)
    assert same_bits(vn_dev.cpu().numpy(), vn) and scale == mscale and same_bits(center, mcenter)
    got, vox, near = check(vn, f, 1.0 / n, colors=mm.vertex_colors(v))
    assert vox["voxel_index"].shape[0] > 300 and (near["closest_tri"] >= 0).all()
    assert same_bits(got["centers"], mm.centres(vox["grid_index"], 1.0 / n, MB))


# ---------------------------------------------------------------------------------------------- 2. the default voxel size
def test_cube_at_default_voxel_size():
    """390 152 voxels by the closed form n^3 - (n-2)^3 at n = 256; no CPU model at this size."""
    from gaustudio_amd import voxelize as vx
    v, f = mm.cube()
    col = mm.vertex_colors(v)
    grid, cloud = vx.voxel_init(dev(v), dev(f), dev(col))           # voxel_size = 1 / 256
    assert grid.shape == (256, 256, 256) and grid.num_voxels == 256 ** 3 - 254 ** 3 == 390152
    gi = grid.grid_index.cpu().numpy()
    assert np.array_equal(gi, mm.cube_shell(256))
    assert np.array_equal(grid.voxel_index.cpu().numpy(), (gi[:, 0].astype(np.int64) * 256 + gi[:, 1]) * 256 + gi[:, 2])
    ps = grid.pair_start.cpu().numpy()
    assert ps[0] == 0 and ps[-1] == grid.pair_tri.shape[0] and (np.diff(ps) >= 1).all() and (np.diff(ps) <= 12).all()
    assert cloud.num_points == 390152
    xyz = cloud.xyz.cpu().numpy()
    assert xyz.dtype == F and np.array_equal(xyz, (mm.centres(gi, 1 / 256, MB) * 2.0 + np.zeros(3)).astype(F))
    rgb = cloud.f_dc.cpu().numpy().reshape(-1, 3) * F(mm.C0) + F(0.5)
    assert np.isfinite(rgb).all() and rgb.min() > col.min() - 1e-5 and rgb.max() < col.max() + 1e-5      # convex combinations


# ---------------------------------------------------------------------------------------------- 3. load balance
@pytest.mark.parametrize("n", [64, 128])
def test_one_triangle_across_the_grid(n):
    """A triangle whose box is the whole grid (one lane per column, a few voxels each by the plane range), and one in a plane
    that contains the column direction (every column walks its whole range)."""
    vn = np.array([(-0.49, -0.47, -0.48), (0.49, 0.2, 0.47), (0.1, 0.49, 0.3),
                   (-0.45, -0.4, -0.49), (0.4, 0.45, -0.49), (-0.1, -0.05, 0.49)], dtype=np.float64)
    vn[5, :2] = vn[3, :2] + 0.375 * (vn[4, :2] - vn[3, :2])         # the second triangle's normal has no component along i2
    f = np.array([(0, 1, 2), (3, 4, 5)], dtype=np.int32)
    got, vox, _ = check(vn, f, 1.0 / n, colors=mm.vertex_colors(vn))
    assert vox["voxel_index"].shape[0] > n * n // 4


# ---------------------------------------------------------------------------------------------- 4. long candidate lists
def test_fan_of_2000_triangles_in_one_voxel():
    k = 2000
    a = np.linspace(0, 2 * np.pi, k, endpoint=False)
    centre = np.array([0.03, 0.035, 0.04])
    rim = centre + 0.02 * np.stack([np.cos(a), np.sin(a), 0.3 * np.sin(3 * a)], axis=1)
    sv, sf = mm.soup(seed=11, n=6)
    vn = np.concatenate([centre[None], rim, sv.astype(np.float64) * 0.45])
    fan = np.stack([np.zeros(k, dtype=np.int64), 1 + np.arange(k), 1 + (np.arange(k) + 1) % k], axis=1)
    f = np.concatenate([fan, sf + k + 1]).astype(np.int32)
    got, vox, near = check(vn, f, 1 / 16, colors=mm.vertex_colors(vn))
    assert np.diff(vox["pair_start"]).max() == k                     # one voxel lists the whole fan


# ---------------------------------------------------------------------------------------------- 5. degenerate triangles
def test_degenerate_triangles():
    v, f = mm.icosphere(1)
    vn, _, _ = mm.normalize_mesh(v)
    p, d = np.array([0.05, -0.1, 0.02]), np.array([0.11, 0.07, -0.13])
    extra = np.array([p, p + d, p + 2.5 * d, (-0.2, 0.1, 0.1), (-0.05, 0.2, 0.15)])          # inside the sphere
    nv = vn.shape[0]
    vn = np.concatenate([vn, extra])
    deg = [(0, 0, 5), (3, 7, 3), (9, 9, 9), (nv, nv + 1, nv + 2), (nv + 2, nv, nv + 1), (nv + 3, nv + 3, nv + 4),
           (nv + 3, nv + 4, nv + 4), (nv + 4, nv + 4, nv + 4)]
    f = np.concatenate([f[:40], np.array(deg, dtype=np.int32), f[40:]]).astype(np.int32)
    got, vox, near = check(vn, f, 1 / 16, colors=mm.vertex_colors(vn))
    listed = np.unique(vox["pair_tri"])
    assert set(range(40, 48)) <= set(listed.tolist())                # each voxelizes as the segment or point it is
    assert np.isfinite(got["closest_uvw"]).all() and np.isfinite(got["color"]).all()
    tri = got["closest_tri"]
    assert np.isfinite(near["d2"][tri >= 0]).all() and (near["d2"][tri < 0] == np.inf).all()
    assert (got["closest_uvw"][tri < 0] == 0).all() and (got["color"][tri < 0] == 0.5).all()


# ---------------------------------------------------------------------------------------------- 6. triangles on voxel faces
def test_quad_on_a_voxel_face_occupies_both_sides():
    v, f = mm.cube(interior_quad=True)
    vn, _, _ = mm.normalize_mesh(v)
    n = 16
    got, vox, _ = check(vn, f, 1 / n, colors=mm.vertex_colors(v))
    g = got["grid_index"]
    inner = g[((g > 0) & (g < n - 1)).all(axis=1)]
    assert g.shape[0] == 1352 + 2 * (n - 2) ** 2 and set(inner[:, 0].tolist()) == {n // 2 - 1, n // 2}


# ---------------------------------------------------------------------------------------------- 7. determinism
def test_two_runs_and_a_face_permutation():
    v, f = mm.soup(seed=21, n=60)          # triangles that share no vertex or edge: no two at exactly the same distance
    vn, _, _ = mm.normalize_mesh(v)
    col = mm.vertex_colors(v)
    a, b = gpu_run(vn, f, 1 / 24, colors=col), gpu_run(vn, f, 1 / 24, colors=col)
    for k in ("voxel_index", "pair_start", "pair_tri", "grid_index", "occupancy", "closest_tri", "closest_uvw", "color"):
        assert same_bits(a[k], b[k]), k
    perm = np.random.default_rng(5).permutation(f.shape[0])          # new face j is old face perm[j]
    fp = f[perm]
    # the model says this mesh has no voxel whose winner depends on the tie rule; then the device must agree too
    vox, near = model_run(vn, f, 1 / 24, colors=col)
    voxp, nearp = model_run(vn, fp, 1 / 24, colors=col)
    assert np.array_equal(perm[nearp["closest_tri"]], near["closest_tri"])
    c = gpu_run(vn, fp, 1 / 24, colors=col)
    assert_same(c, voxp, nearp)
    assert np.array_equal(c["voxel_index"], a["voxel_index"]) and np.array_equal(c["pair_start"], a["pair_start"])
    assert np.array_equal(perm[c["closest_tri"]], a["closest_tri"])
    assert same_bits(c["color"], a["color"]) and same_bits(c["closest_uvw"], a["closest_uvw"])


# ---------------------------------------------------------------------------------------------- 8. general bounds
def test_general_bounds_and_a_voxel_size_that_is_no_power_of_two():
    v, f = mm.ellipsoid()
    vn = v.astype(np.float64) * 0.45 + np.array([0.55, 1.0, -1.25])         # partly outside the bounds
    lo, hi, vs = (0.3, -0.2, 0.1), (1.3, 0.5, 1.3), 0.1
    assert mm.grid_shape(vs, lo, hi) == (10, 7, 12)
    got, vox, near = check(vn, f, vs, lo, hi, colors=mm.vertex_colors(v))
    assert 100 < vox["voxel_index"].shape[0] and got["grid_index"].max(axis=0).tolist() == [9, 6, 11]
    want = mm.centres(vox["grid_index"], vs, lo)
    assert same_bits(got["centers"], want)
    box = np.stack([mm.box_centre(vox["grid_index"][:, d], d, vs, lo) for d in range(3)], axis=1)
    assert not np.array_equal(box, want) and np.abs(box - want).max() < 1e-15          # the two centre formulas differ here
    # float32 vertices are used as float64
    got32 = gpu_run(vn.astype(F), f, vs, lo, hi, closest=False)
    vox32, _ = model_run(vn.astype(F).astype(np.float64), f, vs, lo, hi, closest=False)
    assert_same(got32, vox32)


# ---------------------------------------------------------------------------------------------- 8b. the pair sort's edges
@pytest.mark.parametrize("n2", [5, 7])
def test_pair_sort_past_one_radix_tile_on_one_and_two_digit_grids(n2):
    """More pairs than one 4096-key radix tile, no multiple of 256, on 7 x 7 x 5 = 245 cells (8 key bits: one pass) and
    7 x 7 x 7 = 343 cells (9 bits: two passes)."""
    v, f = mm.soup(seed=31, n=1100)
    vn = v.astype(np.float64) * 0.3 + np.array([0.44, 0.44, 0.4])
    vs, lo, hi = 0.125, (0.0, 0.0, 0.0), (0.875, 0.875, 0.125 * n2)
    assert mm.grid_shape(vs, lo, hi) == (7, 7, n2)
    got, vox, _ = check(vn, f, vs, lo, hi, closest=False)
    pairs = got["pair_tri"].shape[0]
    assert pairs > 4096 and pairs % 256 != 0
    assert vox["voxel_index"].max() == 7 * 7 * n2 - 1                  # the highest key is there


# ---------------------------------------------------------------------------------------------- 9. errors
def test_errors_leave_the_outputs_untouched():
    from gaustudio_amd import _C, voxelize as vx
    from gaustudio_amd._abi import Workspace
    t = _torch()
    v, f = mm.icosphere(1)
    vn, _, _ = mm.normalize_mesh(v)
    bad_f = f.copy()
    bad_f[17, 1] = vn.shape[0]
    neg_f = f.copy()
    neg_f[3, 0] = -1
    bad_v = vn.copy()
    bad_v[5, 2] = np.nan
    inf_v = vn.copy()
    inf_v[0, 0] = np.inf
    for vv, ff in ((vn, bad_f), (vn, neg_f), (bad_v, f), (inf_v, f)):
        with pytest.raises(ValueError, match="face index lies outside|not finite"):
            vx.voxelize_mesh(dev(vv), dev(ff), 1 / 16)
        # the C entry: GSR_ERR_ARG and nothing written
        vd, fd = dev(vv), dev(ff)
        nf = ff.shape[0]
        tri_box = t.full((nf * 6,), -77, dtype=t.int32, device="cuda")
        col_start = t.full((nf + 1,), -77, dtype=t.int32, device="cuda")
        items = ctypes.c_int(-77)
        ws = Workspace(vd.device)
        rc = _C.lib().gsr_voxel_plan(ws.fn, None, _C._ptr(vd), ctypes.c_int(vv.shape[0]), _C._ptr(fd), ctypes.c_int(nf),
                                     ctypes.c_double(1 / 16), (ctypes.c_double * 3)(*MB), ctypes.c_int(16), ctypes.c_int(16),
                                     ctypes.c_int(16), _C._ptr(tri_box), _C._ptr(col_start), ctypes.byref(items), _C._stream(vd.device))
        t.cuda.synchronize()
        assert rc == -2 and items.value == -77 and bool((tri_box == -77).all()) and bool((col_start == -77).all())
    with pytest.raises(ValueError, match="between 2 and 1024"):
        vx.voxelize_mesh(dev(vn), dev(f), 1 / 1025)
    with pytest.raises(ValueError, match="not finite"):
        vx.voxel_seeds(dev(bad_v.astype(F)), dev(f))
    with pytest.raises(ValueError, match="no extent"):
        vx.voxel_seeds(dev(np.ones((3, 3), dtype=F)), dev(f[:1] * 0))
    # an empty face list: an empty grid from the Open3D-equivalent call, the reference's error from the initializer
    empty = vx.voxelize_mesh(dev(vn), dev(f[:0]), 1 / 16, return_occupancy=True)
    assert empty.num_voxels == 0 and empty.pair_start.tolist() == [0] and empty.grid_index.shape == (0, 3) and not empty.occupancy.any()
    assert vx.closest_on_mesh(empty, dev(vn), dev(f[:0]))["closest_tri"].shape == (0,)
    with pytest.raises(ValueError, match="No voxels generated from mesh"):
        vx.voxel_seeds(dev(v), dev(f[:0]))
    # a mesh outside the bounds touches no voxel
    assert vx.voxelize_mesh(dev(vn + 5.0), dev(f), 1 / 16).num_voxels == 0
    # the largest grid is accepted
    g = vx.voxelize_mesh(dev(vn), dev(f[:2]), 1 / 1024)
    assert g.shape == (1024, 1024, 1024) and g.num_voxels > 1000


# ---------------------------------------------------------------------------------------------- 10. end to end
def test_seeds_export_and_render(tmp_path):
    from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, formats, scenes, voxelize as vx
    t = _torch()
    v, f, col = mm.colored_sphere(3)
    gen = t.Generator(device="cuda").manual_seed(3)
    grid, cloud = vx.voxel_init(dev(v), dev(f), dev(col), voxel_size=1 / 32, sh_degree=3, generator=gen)
    P = cloud.num_points
    assert P == grid.num_voxels > 2000
    # against the model's seeds
    vn, scale, center = mm.normalize_mesh(v)
    vox, near = model_run(vn, f, 1 / 32, colors=col)
    want = mm.seeds(mm.centres(vox["grid_index"], 1 / 32, MB), scale, center, 1 / 32, rgb=near["color"], sh_degree=3)
    for k in ("xyz", "scale", "opacity", "f_dc", "f_rest"):
        assert same_bits(getattr(cloud, k).cpu().numpy(), want[k]), k
    assert bool(t.isposinf(cloud.opacity).all())
    rot = cloud.rot.cpu().numpy()
    assert rot.shape == (P, 4) and np.abs(np.linalg.norm(rot, axis=1) - 1).max() < 1e-6
    gray = vx.voxel_seeds(dev(v), dev(f), dev(col), voxel_size=1 / 32, sh_degree=0, colors="gray", rotations="identity", opacity=0.5)
    assert not gray.f_dc.any() and not gray.opacity.any() and gray.f_rest.shape == (P, 0, 3)
    assert bool((gray.rot == t.tensor([1.0, 0, 0, 0], device="cuda")).all())
    ones = vx.voxel_seeds(dev(v), dev(f), voxel_size=1 / 32, sh_degree=1)
    assert same_bits(ones.f_dc.cpu().numpy(), np.broadcast_to(mm.rgb2sh(np.ones(3, dtype=F)), (P, 1, 3)))
    # PLY round trip
    path = str(tmp_path / "seeds.ply")
    formats.export_gaussian_ply(path, cloud)
    back = formats.load_gaussian_ply(path)
    for k in ("xyz", "f_dc", "f_rest", "opacity", "scale", "rot"):
        a, b = getattr(cloud, k).cpu(), getattr(back, k)
        assert a.numel() == b.numel() and same_bits(a.numpy().reshape(-1), b.numpy().reshape(-1)), k
    # one 64 x 64 forward
    cam = scenes.look_at_camera(64, 64, (0.0, 0.0, -3.0), (0.0, 0.0, 0.0))
    rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, t.zeros(3), 1.0, cam.viewmatrix.cuda(),
                                       cam.projmatrix.cuda(), 3, cam.campos.cuda(), False, False)
    act = cloud.activated()
    with t.no_grad():
        out = GaussianRasterizer(rs)(means3D=act["means3D"], means2D=t.zeros_like(act["means3D"]), opacities=act["opacities"],
                                     shs=act["shs"], scales=act["scales"], rotations=act["rotations"])
    color, opac = out[0], out[4]
    assert all(bool(t.isfinite(o.float()).all()) for o in out)
    assert float(opac[0, 32, 32]) > 0.5 and float(opac[0, 0, 0]) == 0.0 and float(color[:, 32, 32].max()) > 0.1
