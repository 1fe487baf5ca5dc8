"""Limit paths of TSDFVolume.integrate / extract (csrc/gsr_tsdf.hip) that no scan of a nearby sphere reaches: updates outside
the workgroup-local aggregation window (+-512 voxels around the workgroup's first active point), a block hash that is exactly
full, and the 24-bit count mark GSR_TSDF_COUNT_FULL.  The integer state is compared with oracle/tsdf_oracle.c bit for bit, as
tests/test_tsdf.py::test_integrate_matches_oracle_exactly does; what an input is meant to reach (voxels outside the window,
exactly 64 blocks, ...) is asserted on the oracle's side first.  The overflow paths are handled errors with bounded loops."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import tsdf_pyoracle as to  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
DEV = torch.device("cuda", 0)
WINDOW = 512                      # the local table addresses voxels in [first - 512, first + 512) per axis


def oracle_state(voxel, trunc, carve, scans):
    ov = to.Volume(voxel, trunc, carve)
    for pts, o in scans:
        ov.integrate(pts, o)
    c, t, w, s = ov.export()
    ov.close()
    return c, t, w, s


def gpu_volume(voxel, trunc, carve, capacity):
    from gaustudio_amd.tsdf import TSDFVolume
    return TSDFVolume(voxel, trunc, space_carving=carve, capacity_blocks=capacity)


def assert_state_equal(vol, ref):
    c, _, w, s = [x.cpu().numpy() for x in vol.export_voxels()]
    assert np.array_equal(c, ref[0]) and np.array_equal(w, ref[2]) and np.array_equal(s, ref[3])


def voxel_of(p, voxel):
    """the kernel's window centre: floor(p * (1 / voxel_size)) in float32"""
    return np.floor(np.asarray(p, F) * (F(1.0) / F(voxel))).astype(np.int64)


def canon(Vx, Tx):
    out = set()
    for a in Vx.astype(F)[Tx]:
        rows = [tuple(r) for r in a.tolist()]
        k = rows.index(min(rows))
        out.add(tuple(rows[k:] + rows[:k]))
    return out


# ------------------------------------------------------------------------------------------------------ long rays
def cone_points():
    rng = np.random.default_rng(0)
    d = np.stack([0.03 * rng.standard_normal(1024), 0.03 * rng.standard_normal(1024), np.ones(1024)], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.array([0.013, -0.021, 0.007], F)
    return (o + d * rng.uniform(2.6, 3.0, (1024, 1))).astype(F), o


@pytest.fixture(scope="module")
def cone():
    pts, o = cone_points()
    return pts, o, oracle_state(0.004, 0.016, True, [(pts, o)])


@pytest.mark.parametrize("as_map", [False, True])
def test_space_carving_rays_longer_than_the_local_window(cone, as_map):
    """Rays of 650 - 750 voxels carved from the sensor on: every workgroup's window is centred on a point at the far end, so
    the first ~150 - 230 voxels of every ray miss it and go to the volume one atomic each (4 % of the volume's voxels
    lie outside every workgroup's window, 7 % more than 512 voxels from the first point).  As a flat list (4 workgroups of
    256) and as a 32 x 32 map (one workgroup of 1024 threads with the larger table)."""
    pts, o, ref = cone
    blocks = len(np.unique(ref[0] >> 3, axis=0))
    firsts = voxel_of(pts[::256], 0.004)
    outside = (ref[0][:, 2] < firsts[:, 2].min() - WINDOW).mean()             # outside EVERY workgroup's window
    print(f"cone: {len(ref[0])} voxels in {blocks} blocks, {100 * outside:.1f} % outside every window")
    assert len(ref[0]) == 464834 and blocks == 6561 and outside > 0.04
    vol = gpu_volume(0.004, 0.016, True, 1 << 14)
    p = torch.from_numpy(pts).to(DEV)
    vol.integrate(p.reshape(32, 32, 3) if as_map else p, o)
    assert_state_equal(vol, ref)


# ------------------------------------------------------------------------------------------------------ window far away
FAR = sorted(set(range(0, 4096, 256)) | {0, 32, 2048, 2080})        # first thread of every workgroup: list and 64 x 64 map


def far_first_points():
    rng = np.random.default_rng(1)
    pts = (np.array([0.3, 0.2, 1.5]) + 0.1 * rng.standard_normal((4096, 3))).astype(F)
    pts[FAR] = (np.array([-3.0, 2.5, 1.0]) + 0.01 * rng.standard_normal((len(FAR), 3))).astype(F)
    return pts, np.zeros(3, F)


@pytest.fixture(scope="module")
def far():
    pts, o = far_first_points()
    return pts, o, oracle_state(0.004, 0.016, False, [(pts, o)])


@pytest.mark.parametrize("as_map", [False, True])
def test_window_centred_far_from_the_other_rays(far, as_map):
    """The first point of every workgroup (every 256th of the list; the corner pixel of every 32 x 32 patch of the map) lies
    ~800 voxels from all the others: no other ray of the workgroup finds a slot in the local table."""
    pts, o, ref = far
    v = voxel_of(pts, 0.004)
    near = np.setdiff1d(np.arange(4096), FAR)
    gap = np.abs(v[near, None, 0] - v[None, FAR, 0]).min()
    blocks = len(np.unique(ref[0] >> 3, axis=0))
    print(f"far window: {len(ref[0])} voxels in {blocks} blocks, nearest other point {gap} voxels from a first point")
    assert gap > WINDOW + 8 and blocks < (1 << 14) * 0.5
    vol = gpu_volume(0.004, 0.016, False, 1 << 14)
    p = torch.from_numpy(pts).to(DEV)
    vol.integrate(p.reshape(64, 64, 3) if as_map else p, o)
    assert_state_equal(vol, ref)


# ------------------------------------------------------------------------------------------------------ hash full
HASH_ORIGIN = np.array([0.0031, 0.0017, -0.9], F)


def block_centre_points(n, offset):
    """one point per block (3 g + offset), g in {0 .. n-1}^3: the centre of its voxel (4, 4, 4); voxel 0.01"""
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    blocks = 3 * g + offset
    return ((blocks * 8 + 4.5) * 0.01).astype(F), blocks


def assert_mesh_equal(vol, ref, **kw):
    V, T = vol.extract_triangle_mesh(**kw)
    _, bc = vol.occupied_blocks()
    oV, oT = to.extract_mesh(ref[0], ref[2], ref[3], 0.01, 0.01, blocks={tuple(b) for b in bc.cpu().numpy().tolist()}, **kw)
    assert canon(V, T) == canon(oV, oT) and len(V) == len(oV)
    return len(T)


def test_block_hash_exactly_full():
    """64 blocks in 64 slots: every insertion finds a slot, and the marching cubes' lookups of absent neighbour blocks probe
    a table without an empty slot and end.  A 65th block is the handled overflow."""
    pts, blocks = block_centre_points(4, -5)
    ref = oracle_state(0.01, 0.01, False, [(pts, HASH_ORIGIN)])
    assert len(ref[0]) == 176 and sorted(map(tuple, np.unique(ref[0] >> 3, axis=0).tolist())) == sorted(map(tuple, blocks.tolist()))
    assert len(blocks) == 64 and (blocks < 0).any() and (blocks > 0).any()
    vol = gpu_volume(0.01, 0.01, False, 64)
    vol.integrate(torch.from_numpy(pts).to(DEV), HASH_ORIGIN)
    assert (vol.keys != -1).all()
    assert_state_equal(vol, ref)
    assert_mesh_equal(vol, ref, min_weight=1, fill_holes=True)
    assert assert_mesh_equal(vol, ref, min_weight=0, fill_holes=True) > 0      # holes filled: the three voxels of a ray do mesh
    extra = ((np.array([[7, 7, 7]]) * 8 + 4.5) * 0.01).astype(F)
    vol.integrate(torch.from_numpy(extra).to(DEV), HASH_ORIGIN)
    with pytest.raises(RuntimeError, match="overflowed"):
        vol.extract_triangle_mesh(min_weight=1)


def test_block_hash_nearly_full():
    pts, blocks = block_centre_points(10, -14)
    ref = oracle_state(0.01, 0.01, False, [(pts, HASH_ORIGIN)])
    assert len(np.unique(ref[0] >> 3, axis=0)) == 1000
    vol = gpu_volume(0.01, 0.01, False, 1024)
    vol.integrate(torch.from_numpy(pts).to(DEV), HASH_ORIGIN)
    assert int((vol.keys != -1).sum()) == 1000
    assert_state_equal(vol, ref)
    assert assert_mesh_equal(vol, ref, min_weight=0, fill_holes=True) > 0


# ------------------------------------------------------------------------------------------------------ count mark
def test_count_mark_is_reached_exactly_and_then_refuses():
    """15 x 2^20 observations of one ray: every voxel's count is exactly GSR_TSDF_COUNT_FULL = 0xf00000, which is still
    accepted; its sum is that many times the single observation's.  256 more (one workgroup, aggregated to one add per voxel)
    would pass the mark: the adds are undone, the volume keeps what it had, and status bit 2 makes the next extraction raise."""
    p = np.array([[0.31, 0.17, 1.52]], F)
    o = np.zeros(3, F)
    oc, ot, ow, os_ = oracle_state(0.05, 0.2, False, [(p, o)])
    assert len(oc) == 10 and (ow == 1).all() and os_.max() == 32768 and os_.min() == -25527
    assert (np.abs(os_) * 0xf00000 < 1 << 39).all()
    vol = gpu_volume(0.05, 0.2, False, 64)
    many = torch.from_numpy(p).to(DEV).repeat(1 << 20, 1)
    for _ in range(15):
        vol.integrate(many, o)
    c, t, w, s = [x.cpu().numpy() for x in vol.export_voxels()]
    assert np.array_equal(c, oc) and (w == 0xf00000).all() and np.array_equal(s, os_ * 0xf00000)
    assert (np.abs(t - ot) <= 1e-7 + 0.2 / 2 ** 16).all()
    V, T = vol.extract_triangle_mesh(min_weight=1)
    before = vol.voxels.clone()
    vol.integrate(many[:256], o)
    assert torch.equal(vol.voxels, before)
    with pytest.raises(RuntimeError, match="observations"):
        vol.extract_triangle_mesh(min_weight=1)
