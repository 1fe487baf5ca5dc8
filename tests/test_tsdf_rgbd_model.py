"""CPU checks of the float32 model of ColorTSDFVolume (tests/tsdf_rgbd_model.py) against hand-computed values, and of the
coloured PLY mesh container (gaustudio_amd/formats.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import tsdf_rgbd_model as M  # noqa: E402
from gaustudio_amd import formats  # noqa: E402

F = np.float32
W, H = 64, 48
K = (20.0, 20.0, 32.25, 24.25)           # a voxel column next to the optical axis projects into ONE pixel for both of its z
VL, TR = 0.05, 0.1


def _wall(color=(200, 100, 50), depth=1.0):
    return np.full((H, W), depth, F), np.broadcast_to(np.asarray(color, np.uint8), (H, W, 3)).copy()


@pytest.fixture(scope="module")
def wall_volume():
    vol = M.ModelVolume(VL, TR)
    d, c = _wall()
    vol.integrate(d, c, K, np.eye(4), depth_trunc=5.0)
    return vol


def _hand_tsdf(i, j, k):
    """min(1, (1 - z_c) * mult / trunc) of voxel (i, j, k) for the wall at depth 1 seen from the origin, in float64."""
    x, y, z = (i + 0.5) * VL, (j + 0.5) * VL, (k + 0.5) * VL
    u, v = int(x * K[0] / z + K[2] + 0.5), int(y * K[1] / z + K[3] + 0.5)
    mult = np.sqrt(((u - K[2]) / K[0]) ** 2 + ((v - K[3]) / K[1]) ** 2 + 1.0)
    return min(1.0, (1.0 - z) * mult / TR), mult


@pytest.mark.parametrize("ijk", [(0, 0, 19), (0, 0, 20), (-1, -1, 18), (0, 0, 17), (12, -9, 19), (-20, 7, 20)])
def test_wall_tsdf_of_named_voxels(wall_volume, ijk):
    # float32 against float64: the chain (d - z_c) * mult / trunc has ~6 roundings of 6e-8 relative on values <= 1.2,
    # amplified by 1 / trunc = 10: below 1e-5
    want, mult = _hand_tsdf(*ijk)
    tsdf, w, col = wall_volume.voxel(*ijk)
    assert w == 1.0
    assert abs(float(tsdf) - want) < 1e-5
    assert np.array_equal(col, np.asarray([200, 100, 50], F))
    if ijk == (12, -9, 19):
        assert mult > 1.1                 # the off-axis voxel: the depth-to-distance multiplier is not 1
    if ijk == (0, 0, 17):
        assert tsdf == 1.0                # truncated in front of the surface


def test_wall_voxels_behind_the_band_are_not_written(wall_volume):
    # z_c = 1.125: sdf = -0.125 * mult <= -trunc
    assert wall_volume.voxel(0, 0, 22)[1] == 0.0
    # z_c = 1.075: sdf = -0.075 * mult > -trunc on the axis
    assert wall_volume.voxel(0, 0, 21)[1] == 1.0


def test_wall_mesh_zero_crossing_lies_at_z_1(wall_volume):
    v, f, c = wall_volume.extract_triangle_mesh()
    assert len(v) and len(f)
    # every vertex lies between the two voxel layers around the wall
    assert np.all(np.abs(v[:, 2] - 1.0) <= VL / 2 + 1e-6)
    # next to the optical axis both voxels of a z edge see the same pixel, hence the same multiplier: the crossing of
    # (1 - 0.975) m and (1 - 1.025) m is z = 1 up to the roundings of 0.975 + 0.05 * a0 / (a0 + a1) (a few ulp of 1)
    near = (np.abs(v[:, 0]) < VL) & (np.abs(v[:, 1]) < VL)
    assert near.sum() == 4
    assert np.all(np.abs(v[near, 2] - 1.0) <= 4 * np.finfo(F).eps)
    assert np.array_equal(c, np.broadcast_to(np.asarray([200, 100, 50], F) / F(255), c.shape))
    # the surface faces the camera: normals towards positive tsdf, i.e. -z
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert np.all(n[:, 2] < 0)


def test_running_average_over_three_frames():
    vol = M.ModelVolume(VL, TR)
    colors = [(255, 0, 0), (0, 128, 7), (10, 20, 30)]
    depths = [1.0, 1.01, 0.98]
    for d, c in zip(depths, colors):
        vol.integrate(*_wall(c, d), K, np.eye(4), depth_trunc=5.0)
    tsdf, w, col = vol.voxel(0, 0, 19)
    assert w == 3.0
    # the hand-computed sequence of float32 updates; this voxel (centre 0.025, 0.025, 0.975) projects to
    # u_f = 0.025 * 20 / 0.975 + 32.25 + 0.5 = 33.26, v_f = 25.26: (u, v) = (33, 25)
    a = (F(33) - F(K[2])) / F(K[0])
    b = (F(25) - F(K[3])) / F(K[1])
    mult = np.sqrt((a * a + b * b) + F(1))
    zc = (F(19) + F(0.5)) * F(VL)
    t_run, c_run, w_run = F(0), np.zeros(3, F), F(0)
    for d, c in zip(depths, colors):
        t = min(F(1), ((F(d) - zc) * mult) / F(TR))
        t_run = (t_run * w_run + t) / (w_run + F(1))
        c_run = (c_run * w_run + np.asarray(c, F)) / (w_run + F(1))
        w_run = w_run + F(1)
    assert tsdf == t_run and tsdf.dtype == F
    assert np.array_equal(col, c_run)


def test_invalid_depth_contributes_nothing_and_float_colour_truncates():
    d, _ = _wall()
    bad = d.copy()
    bad[0:8, :] = np.nan
    bad[8:16, :] = np.inf
    bad[16:20, :] = -np.inf
    bad[20:24, :] = -1.0
    bad[24:28, :] = 5.5                       # > depth_trunc
    zeroed = d.copy()
    zeroed[0:28, :] = 0.0
    col = np.full((H, W, 3), 0.999, F)
    a, b = M.ModelVolume(VL, TR), M.ModelVolume(VL, TR)
    a.integrate(bad, col, K, np.eye(4), depth_trunc=5.0)
    b.integrate(zeroed, col, K, np.eye(4), depth_trunc=5.0)
    ea, eb = a.export_voxels(), b.export_voxels()
    assert len(ea[0]) > 0
    for x, y in zip(ea, eb):
        assert np.array_equal(x, y)
    assert np.all(ea[3] == 254.0)             # uint8(0.999 * 255 = 254.745) truncates
    only_bad = np.full((H, W), np.nan, F)
    assert M.ModelVolume(VL, TR).integrate(only_bad, col, K, np.eye(4)) == set()
    # the three colour layouts agree; out-of-range and NaN floats clip
    q = M.quantise_color(np.asarray([[[1.5, -0.2, np.nan]]], F))
    assert np.array_equal(q, np.asarray([[[255, 0, 0]]], F))
    chw = np.random.default_rng(0).random((3, 5, 7)).astype(F)
    assert np.array_equal(M.quantise_color(chw), M.quantise_color(np.transpose(chw, (1, 2, 0))))


def test_touch_box_opens_8_and_27_blocks():
    # one valid pixel on the optical axis at depth 0.8 = the corner of eight blocks (block edge 8 * 0.1)
    d = np.zeros((9, 9), F)
    d[4, 4] = 0.8
    E = np.eye(4)
    k = (10.0, 10.0, 4.0, 4.0)
    small = M.ModelVolume(0.1, 0.2, depth_sampling_stride=4).touched_blocks(d, k, E, 5.0)
    assert small == {(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (0, 1)}
    big = M.ModelVolume(0.1, 0.8, depth_sampling_stride=4).touched_blocks(d, k, E, 5.0)
    assert big == {(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (0, 1, 2)}


def test_volume_refuses_a_cpu_device():
    from gaustudio_amd import ColorTSDFVolume
    with pytest.raises(RuntimeError, match="ROCm device"):
        ColorTSDFVolume(device="cpu")


# ---------------------------------------------------------------------- PLY container
def _tetra():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.25, -1.5, 3.0]], F)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2], [4, 0, 1]], np.int32)
    return v, f


def test_write_ply_mesh_without_attributes_writes_the_bytes_it_always_wrote(tmp_path):
    v, f = _tetra()
    p = tmp_path / "plain.ply"
    formats.write_ply_mesh(p, v, f, comments=("written by write_ply_mesh before it took colours",))
    golden = os.path.join(HERE, "golden", "ply_mesh_plain.ply")      # written by the writer as it was before the keywords
    assert p.read_bytes() == open(golden, "rb").read()
    v2, f2 = formats.read_ply_mesh(golden)
    assert np.array_equal(v2, v) and np.array_equal(f2, f)


def test_ply_mesh_round_trip_with_colours_and_normals(tmp_path):
    v, f = _tetra()
    colors = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.25, 1.0 / 255], [2.0, -1.0, 0.999]], F)
    normals = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0.8, 0], [0, -1, 0]], F)
    p = tmp_path / "coloured.ply"
    formats.write_ply_mesh(p, v, f, vertex_colors=colors, vertex_normals=normals)
    head = p.read_bytes().split(b"end_header\n")[0].decode().split("\n")
    assert head[3:12] == ["property float x", "property float y", "property float z", "property float nx", "property float ny",
                          "property float nz", "property uchar red", "property uchar green", "property uchar blue"]
    v2, f2, attrs = formats.read_ply_mesh(p, return_attributes=True)
    assert np.array_equal(v2, v) and np.array_equal(f2, f)
    assert attrs["colors"].dtype == np.uint8
    assert np.array_equal(attrs["colors"], [[255, 0, 0], [0, 255, 0], [0, 0, 255], [128, 64, 1], [255, 0, 255]])
    assert np.array_equal(attrs["normals"], normals)
    assert formats.read_ply_mesh(p)[0].shape == (5, 3)                # the two-value form skips the attributes
    # colours alone, given as uint8; a plain file has no attributes
    formats.write_ply_mesh(p, v, f, vertex_colors=attrs["colors"])
    _, _, a2 = formats.read_ply_mesh(p, return_attributes=True)
    assert np.array_equal(a2["colors"], attrs["colors"]) and "normals" not in a2
    formats.write_ply_mesh(p, v, f)
    assert formats.read_ply_mesh(p, return_attributes=True)[2] == {}
    with pytest.raises(formats.PlyFormatError):
        formats.write_ply_mesh(p, v, f, vertex_colors=colors[:3])
