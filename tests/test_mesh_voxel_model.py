"""CPU (-m "not gpu"): the float64 model of the mesh voxelizer (tests/mesh_voxel_model.py) against hand cases, against itself
in its two forms, against closed forms; the seeds against hand-computed values; the Python boundary of
gaustudio_amd.voxelize and the exported gsr_voxel_* symbols."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import mesh_voxel_model as mm  # noqa: E402
from gaustudio_amd import voxelize as vx  # noqa: E402

F = np.float32
MB = (-0.5, -0.5, -0.5)
CASES = {"icosphere16": (lambda: mm.icosphere(1), 16), "ellipsoid24": (mm.ellipsoid, 24), "soup16": (mm.soup, 16)}


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (make, n) in CASES.items():
        v, f = make()
        vn, scale, center = mm.normalize_mesh(v)
        vs = 1.0 / n
        shape = mm.grid_shape(vs)
        assert shape == (n, n, n)
        out[name] = dict(v=v, f=f, vn=vn, vs=vs, shape=shape, boxed=mm.voxelize_boxed(vn, f, vs, MB, shape))
    return out


# ---------------------------------------------------------------------------------------------- 1. tribox hand cases
def _tb(tri, c=(0.0, 0.0, 0.0), h=0.5):
    t = np.asarray(tri, dtype=np.float64)
    return bool(mm.tribox(np.asarray(c, dtype=np.float64), h, t[0], t[1], t[2]))


def test_tribox_hand_cases():
    assert _tb([(-0.2, -0.1, 0.0), (0.3, 0.0, 0.1), (0.0, 0.25, -0.2)])                       # inside the box
    assert not _tb([(2.0, 2.0, 2.0), (3.0, 2.0, 2.5), (2.0, 3.0, 2.0)])                      # outside
    assert _tb([(0.5, -0.2, -0.2), (0.5, 0.2, -0.2), (0.5, 0.0, 0.3)])                        # lies in the face x = h
    assert _tb([(0.5, 0.0, 0.0), (1.5, 0.3, 0.0), (1.5, -0.3, 0.2)])                          # touches the face from outside
    assert not _tb([(0.5000001, 0.0, 0.0), (1.5, 0.3, 0.0), (1.5, -0.3, 0.2)])
    # a large triangle in the plane x + y + z = s: cuts the corner (h, h, h) for s < 1.5, touches it at 1.5, misses above
    plane = lambda s: [(s, 0.0, 0.0), (0.0, s, 0.0), (0.0, 0.0, s)]
    assert _tb(plane(1.25)) and _tb(plane(1.5))
    assert not _tb(plane(1.75))                      # its AABB [0, 1.75]^3 overlaps the box, its plane does not
    assert _tb(plane(10.0), c=(3.0, 3.0, 4.0))       # far from every vertex and edge, inside the face
    assert not _tb(plane(10.0), c=(3.0, 3.0, 2.0))
    # zero-area triangles: a segment through the box, a segment past it, a point in it, a point outside (no NaN: plain tests)
    assert _tb([(-1.0, 0.1, 0.1), (1.0, 0.1, 0.1), (1.0, 0.1, 0.1)])
    assert _tb([(-1.0, 0.1, 0.1), (0.0, 0.1, 0.1), (1.0, 0.1, 0.1)])
    assert not _tb([(-1.0, 0.7, 0.1), (0.0, 0.7, 0.1), (1.0, 0.7, 0.1)])
    assert not _tb([(-0.3, 1.5, 0.0), (1.5, -0.3, 0.0), (1.5, -0.3, 0.0)])     # a diagonal segment (x + y = 1.2) past the corner
    assert _tb([(-0.5, 1.5, 0.0), (1.5, -0.5, 0.0), (1.5, -0.5, 0.0)])         # x + y = 1 touches the edge of the box
    assert _tb([(0.2, 0.2, 0.2)] * 3) and not _tb([(0.2, 0.6, 0.2)] * 3)
    assert _tb([(0.5, 0.5, 0.5)] * 3)                                         # a point on the corner touches


def test_grid_and_centres():
    assert mm.grid_shape(1 / 256) == (256, 256, 256)
    assert mm.grid_shape(0.1, (0, 0, 0), (1.0, 0.25, 0.64)) == (10, 3, 6)          # 2.5 rounds away from zero
    i = np.arange(256)
    assert np.array_equal(mm.box_centre(i, 0, 1 / 256, MB), mm.voxel_centre(i, 0, 1 / 256, MB))      # a power of two
    i = np.arange(10)
    a, b = mm.box_centre(i, 0, 0.1, (0.3, 0, 0)), mm.voxel_centre(i, 0, 0.1, (0.3, 0, 0))
    assert np.abs(a - b).max() < 1e-15 and not np.array_equal(a, b)               # otherwise they differ in the last bits
    with pytest.raises(ValueError):
        mm.normalize_mesh(np.ones((3, 3), dtype=F))
    vn, scale, center = mm.normalize_mesh(mm.cube()[0])
    assert scale == 2.0 and np.array_equal(center, np.zeros(3)) and vn.min() == -0.5 + 1e-6 and vn.max() == 0.5 - 1e-6


# ---------------------------------------------------------------------------------------------- 2. the two forms agree
@pytest.mark.parametrize("name", list(CASES))
def test_brute_equals_boxed(cases, name):
    c = cases[name]
    brute = mm.voxelize_brute(c["vn"], c["f"], c["vs"], MB, c["shape"])
    filtered = mm.voxelize_boxed(c["vn"], c["f"], c["vs"], MB, c["shape"], plane_filter=True)
    assert brute["voxel_index"].shape[0] > 300
    for k in ("voxel_index", "pair_start", "pair_tri", "grid_index"):
        assert np.array_equal(brute[k], c["boxed"][k]), k
        assert np.array_equal(brute[k], filtered[k]), f"{k}: the plane range dropped or added a voxel"
    vi, ps, pt = (brute[k] for k in ("voxel_index", "pair_start", "pair_tri"))
    assert (np.diff(vi) > 0).all() and ps[0] == 0 and ps[-1] == pt.shape[0] and (np.diff(ps) > 0).all()
    for q in range(vi.shape[0]):
        assert (np.diff(pt[ps[q]:ps[q + 1]]) > 0).all()


def test_icosphere_count():
    v, f = mm.icosphere(1)
    assert f.shape[0] == 80
    vn, _, _ = mm.normalize_mesh(v)
    assert mm.voxelize_boxed(vn, f, 1 / 16, MB, (16, 16, 16))["voxel_index"].shape[0] == 1088


# ---------------------------------------------------------------------------------------------- 3. 27 voxels suffice
@pytest.mark.parametrize("name", list(CASES))
def test_neighbourhood_equals_global(cases, name):
    c = cases[name]
    col = mm.vertex_colors(c["v"])
    near = mm.closest(c["boxed"], c["vn"], c["f"], c["vs"], MB, col)
    far = mm.closest(c["boxed"], c["vn"], c["f"], c["vs"], MB, col, neighbourhood=False)
    for k in ("closest_tri", "closest_uvw", "d2", "color"):
        assert np.array_equal(near[k], far[k]), k
    assert (near["closest_tri"] >= 0).all() and np.isfinite(near["closest_uvw"]).all()
    assert np.sqrt(near["d2"].max()) <= 0.8660254037844387 * c["vs"]             # half a voxel diagonal
    assert np.abs(near["closest_uvw"].sum(axis=1) - 1).max() < 1e-12 and near["closest_uvw"].min() > -1e-12


def test_closest_point_regions_and_ties():
    a, b, c = np.array([0.0, 0, 0]), np.array([1.0, 0, 0]), np.array([0.0, 1, 0])
    q = lambda p: tuple(float(x) for x in mm.closest_point(np.array(p, dtype=np.float64), a, b, c))
    assert q([-1, -1, 0]) == (0.0, 0.0, 2.0)                       # vertex A
    assert q([2, -0.5, 0]) == (1.0, 0.0, 1.25)                     # vertex B
    assert q([-0.5, 3, 0]) == (0.0, 1.0, 4.25)                     # vertex C
    assert q([0.25, -1, 0]) == (0.25, 0.0, 1.0)                    # edge AB
    assert q([-2, 0.5, 0]) == (0.0, 0.5, 4.0)                      # edge AC
    assert q([1, 1, 0]) == (0.5, 0.5, 0.5)                         # edge BC
    assert q([0.25, 0.25, 3]) == (0.25, 0.25, 9.0)                 # interior
    # a repeated vertex gives 0 / 0 in the edge region: NaN, which never wins
    assert math.isnan(float(mm.closest_point(np.array([0.2, 0.3, 0.1]), a, a, c)[2]))
    # an exact tie between two triangles sharing an edge goes to the lower index, whatever the order of the faces
    v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], dtype=np.float64) * 0.25 - 0.1
    for faces in ([(0, 1, 2), (0, 3, 1)], [(0, 3, 1), (0, 1, 2)]):
        vox = mm.voxelize_boxed(v, np.array(faces), 0.25, MB, (4, 4, 4))
        got = mm.closest(vox, v, np.array(faces), 0.25, MB)
        d_all = np.stack([mm.closest_point(mm.centres(vox["grid_index"], 0.25, MB), v[f[0]], v[f[1]], v[f[2]])[2] for f in faces])
        tie = d_all[0] == d_all[1]
        assert tie.any() and (got["closest_tri"][tie] == 0).all()


# ---------------------------------------------------------------------------------------------- 4. closed forms
def test_cube_closed_form():
    v, f = mm.cube()
    vn, _, _ = mm.normalize_mesh(v)
    assert np.abs(vn).min() == np.abs(vn).max() == 0.5 - 1e-6
    n = 16
    vox = mm.voxelize_boxed(vn, f, 1 / n, MB, (n, n, n))
    assert vox["voxel_index"].shape[0] == n ** 3 - (n - 2) ** 3 == 1352
    assert np.array_equal(vox["grid_index"], mm.cube_shell(n))
    v, f = mm.cube(interior_quad=True)
    vn, _, _ = mm.normalize_mesh(v)
    g = mm.voxelize_boxed(vn, f, 1 / n, MB, (n, n, n))["grid_index"]
    assert g.shape[0] == 1352 + 2 * (n - 2) ** 2
    inner = g[((g > 0) & (g < n - 1)).all(axis=1)]
    assert inner.shape[0] == 2 * (n - 2) ** 2 and set(inner[:, 0]) == {n // 2 - 1, n // 2}      # x = 0 lies on a voxel face


# ---------------------------------------------------------------------------------------------- 5. seeds
def test_seeds_hand_values():
    # the cube [-1, 1]^3: scale 2, center 0; voxel_size 1/4: voxel (0,0,0) has the centre -0.375 -> -0.75, (3,1,2) -> 0.75, -0.25, 0.25
    centres = mm.centres(np.array([(0, 0, 0), (3, 1, 2)]), 0.25, MB)
    assert np.array_equal(centres, [(-0.375, -0.375, -0.375), (0.375, -0.125, 0.125)])
    s = mm.seeds(centres, 2.0, np.zeros(3), 0.25, rgb=np.array([(0.25, 0.5, 1.0), (1.0, 0.0, 0.75)], dtype=F), sh_degree=2)
    assert all(a.dtype == F for a in s.values())
    assert np.array_equal(s["xyz"], np.array([(-0.75, -0.75, -0.75), (0.75, -0.25, 0.25)], dtype=F))
    want_scale = math.log(0.4 + 1e-7)                                   # log(0.25 * 2 * 0.8 + 1e-7) = -0.91629048...
    assert s["scale"].shape == (2, 3) and np.abs(s["scale"] - want_scale).max() < 2e-7 and abs(want_scale + 0.9162905) < 1e-7
    assert s["opacity"].shape == (2, 1) and np.isposinf(s["opacity"]).all()         # inverse_sigmoid(1.0); its sigmoid is 1
    assert float(torch.sigmoid(torch.from_numpy(s["opacity"])).min()) == 1.0
    want = np.array([(-0.25, 0.0, 0.5), (0.5, -0.5, 0.25)]) / mm.C0     # RGB2SH: -0.8862269, 0, 1.7724539; 1.7724539, ..., 0.8862269
    assert s["f_dc"].shape == (2, 1, 3) and np.abs(s["f_dc"][:, 0] - want).max() < 2e-7
    assert abs(float(s["f_dc"][0, 0, 2]) - 1.7724539) < 2e-7 and s["f_dc"][0, 0, 1] == 0
    assert s["f_rest"].shape == (2, 8, 3) and not s["f_rest"].any()
    ones = mm.seeds(centres, 2.0, np.zeros(3), 0.25)                   # rgb=None means ones
    assert np.abs(ones["f_dc"] - 0.5 / mm.C0).max() < 2e-7 and ones["f_rest"].shape == (2, 15, 3)
    half = mm.seeds(centres, 2.0, np.array([1.0, 2.0, 3.0]), 0.25, opacity=0.5)
    assert not half["opacity"].any() and np.array_equal(half["xyz"][0], np.array([0.25, 1.25, 2.25], dtype=F))


# ---------------------------------------------------------------------------------------------- 6. Python boundary, exports
def test_argument_checks_need_no_gpu():
    v, f = torch.zeros(4, 3), torch.zeros((2, 3), dtype=torch.int32)
    col = torch.zeros(4, 3)
    for call in (lambda: vx.voxel_seeds(v, f), lambda: vx.voxel_init(v, f, col), lambda: vx.voxelize_mesh(v, f, 0.1),
                 lambda: vx.normalize_mesh(v), lambda: vx.voxelize_mesh(v.double(), f.long(), 0.1)):
        with pytest.raises(ValueError, match="ROCm devices only"):
            call()
    grid = vx.VoxelGrid(f, f[:, 0], f[:, 0], f[:, 0], (4, 4, 4), 0.25, MB)
    with pytest.raises(ValueError, match="ROCm devices only"):
        vx.closest_on_mesh(grid, v, f, col)
    with pytest.raises(TypeError, match="VoxelGrid"):
        vx.closest_on_mesh(None, v, f)
    with pytest.raises(TypeError, match="torch tensors"):
        vx.voxel_seeds(np.zeros((4, 3), dtype=F), f)
    with pytest.raises(TypeError, match="vertices must be"):
        vx.voxel_seeds(v.double(), f)                               # the initializer takes float32 vertices
    with pytest.raises(TypeError, match="vertices must be"):
        vx.voxelize_mesh(v.half(), f, 0.1)
    with pytest.raises(TypeError, match="faces must be int32 or int64"):
        vx.voxel_seeds(v, f.float())
    with pytest.raises(TypeError, match="vertex_colors must be float32"):
        vx.voxel_seeds(v, f, col.double())
    with pytest.raises(ValueError, match=r"vertices must have shape \[V, 3\]"):
        vx.voxel_seeds(torch.zeros(4, 2), f)
    with pytest.raises(ValueError, match=r"faces must have shape \[F, 3\]"):
        vx.voxel_seeds(v, torch.zeros((2, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="vertex_colors must have shape"):
        vx.voxel_seeds(v, f, torch.zeros(3, 3))
    for bad in (4, -1, 1.5):
        with pytest.raises(ValueError, match="sh_degree must be 0..3"):
            vx.voxel_seeds(v, f, sh_degree=bad)
    with pytest.raises(ValueError, match="colors must be"):
        vx.voxel_seeds(v, f, colors="nearest")
    with pytest.raises(ValueError, match="rotations must be"):
        vx.voxel_seeds(v, f, rotations="normal")
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError, match="opacity must lie"):
            vx.voxel_seeds(v, f, opacity=bad)
    with pytest.raises(TypeError, match="generator"):
        vx.voxel_seeds(v, f, generator=3)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size must be positive"):
            vx.voxel_seeds(v, f, voxel_size=bad)
    with pytest.raises(ValueError, match="between 2 and 1024"):
        vx.voxel_seeds(v, f, voxel_size=1 / 2048)                  # n = 2048
    with pytest.raises(ValueError, match="between 2 and 1024"):
        vx.voxelize_mesh(v, f, 1.0, MB, (0.5, 0.5, 0.5))           # n = 1
    with pytest.raises(ValueError, match="three entries"):
        vx.voxelize_mesh(v, f, 0.1, (0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="finite"):
        vx.voxelize_mesh(v, f, 0.1, (0, 0, float("nan")), (1, 1, 1))
    assert vx._bounds(0.1, (0, 0, 0), (1.0, 0.25, 0.64))[3] == mm.grid_shape(0.1, (0, 0, 0), (1.0, 0.25, 0.64)) == (10, 3, 6)


def test_library_exports_and_rejects_bad_grids():
    import ctypes
    from gaustudio_amd import _C
    hdr = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    L = _C.lib()
    names = ("gsr_voxel_plan", "gsr_voxel_count", "gsr_voxel_emit", "gsr_voxel_sort", "gsr_voxel_closest")
    for n in names:
        assert re.search(r"\bint %s\(" % n, hdr) and hasattr(L, n), n
    assert L.gsr_abi_version() == 6
    # bad grids are refused before anything touches a device
    mb = (ctypes.c_double * 3)(-0.5, -0.5, -0.5)
    out = ctypes.c_int(-7)
    null = ctypes.c_void_p(0)
    for vs, n in ((1 / 16, (16, 16, 1)), (1 / 16, (16, 1025, 16)), (0.0, (16, 16, 16)), (-1.0, (16, 16, 16)),
                  (float("nan"), (16, 16, 16))):
        rc = L.gsr_voxel_plan(null, null, null, ctypes.c_int(0), null, ctypes.c_int(0), ctypes.c_double(vs), mb,
                              *(ctypes.c_int(k) for k in n), null, null, ctypes.byref(out), null)
        assert rc == -2 and out.value == -7
    assert L.gsr_voxel_closest(null, ctypes.c_int(0), null, ctypes.c_int(0), null, ctypes.c_double(1 / 16), mb, ctypes.c_int(16),
                               ctypes.c_int(16), ctypes.c_int(2000), null, null, null, ctypes.c_int(0), null, null, null, null) == -2
