"""Every marching-cubes case on the device.  The three extractors -- sap.marching_cubes (csrc/gsr_psr.hip), TSDFVolume
(csrc/gsr_tsdf.hip) and ColorTSDFVolume (csrc/gsr_tsdf_rgbd.hip) -- read one generated table (csrc/gsr_mc_tables.h); the
other tests of them mesh smooth fields, which reach fewer than half of the 254 non-trivial cases, none of the 5-triangle ones
and no ambiguous face.  Here the fields are random: a dense grid of N(0,1) values, and sparse volumes whose STATE is written
(tests/volume_state.py) rather than integrated, with holes, exact zeros and an unallocated block among allocated ones.

Each test first asserts, on the model side, that its input makes all 254 cases occur among the meshed cubes (a condition on
the input, asserted where the field is large enough to meet it: the 20^3 grids, and the sparse states at the extraction
settings that keep every observed voxel; the thin grids have 39 and 58 cubes, the settings with min_weight >= 1.5 drop most
cubes on purpose).  The device output is then compared with the CPU models, which read the same generator -- bit for bit
where the model states the emission order -- and its index topology is checked: no directed edge twice, and every edge all
of whose cubes are meshed has its reverse exactly once."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import sap_model as sm  # noqa: E402
import tsdf_rgbd_model as M  # noqa: E402
import volume_state as vs  # noqa: E402
from oracle import tsdf_pyoracle as to  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
DEV = torch.device("cuda", 0)

# 3 x 2 x 2 blocks around the origin (voxel coordinates -8 .. 15, -8 .. 7, -8 .. 7), one of them never allocated
ABSENT = (0, -1, 0)
BLOCKS = [(bx, by, bz) for bx in (-1, 0, 1) for by in (-1, 0) for bz in (-1, 0) if (bx, by, bz) != ABSENT]
VOXEL, TRUNC = 0.05, 0.2


def assert_manifold(tris, node, axis, extractable):
    doubled, missing, interior = vs.edge_topology(tris, node, axis, extractable)
    assert doubled == 0 and missing == 0, f"{doubled} directed edges twice, {missing} of {interior} interior edges without one reverse"
    return interior


# ------------------------------------------------------------------------------------------------------ dense grid
def dense_field(shape, level, seed):
    """N(0,1) float32; ~5 % of the nodes exactly at the level (outside: inside iff value < level; at level 0 every other one
    of them is -0.0), ~2 % one ulp below it (inside; a vertex at the far end of its edge)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(shape).astype(F)
    u = rng.random(shape)
    at = np.argwhere(u < 0.05)
    g[tuple(at.T)] = F(level)
    if level == 0.0:
        g[tuple(at[::2].T)] = F(-0.0)
    g[(u >= 0.05) & (u < 0.07)] = np.nextafter(F(level), F(-np.inf))
    return g


@pytest.mark.parametrize("level", [0.25, 0.0, -0.3])
@pytest.mark.parametrize("shape", [(20, 20, 20), (2, 2, 40), (2, 30, 3)])
def test_dense_marching_cubes_on_random_fields(shape, level):
    from gaustudio_amd import sap
    g = dense_field(shape, level, seed=sum(shape))
    inside = g < F(level)
    assert (g == F(level)).any() and (g == np.nextafter(F(level), F(-np.inf))).any()
    if level == 0.0:
        assert (np.signbit(g) & (g == 0)).any() and (~np.signbit(g) & (g == 0)).any()
    case, node, axis = vs.dense_layout(inside)
    if shape == (20, 20, 20):
        assert len(vs.cases_present(case)) == 254
    v, f = sm.marching_cubes(g, level)
    dg = torch.from_numpy(g).to(DEV)
    gv, gf = sap.marching_cubes(dg, level)
    assert gv.dtype == torch.float32 and gf.dtype == torch.int32
    assert tuple(gv.shape) == v.shape and tuple(gf.shape) == f.shape and len(v) == len(node)
    assert np.array_equal(gv.cpu().numpy(), v), "vertices differ"
    assert np.array_equal(gf.cpu().numpy(), f), "faces differ"
    gv2, gf2 = sap.marching_cubes(dg, level)
    assert torch.equal(gv, gv2) and torch.equal(gf, gf2)
    assert_manifold(gf.cpu().numpy(), node, axis, vs.dense_extractable(shape))


# ------------------------------------------------------------------------------------------------------ the helper and the product
def test_written_keys_are_where_the_kernels_look():
    """Blocks opened by integrate() -- one point per block, in a table small enough to collide -- sit on the helper's probe
    sequence with no empty slot in front of them; a written state comes back from occupied_blocks() / export_voxels() as
    written."""
    from gaustudio_amd import ColorTSDFVolume
    from gaustudio_amd.tsdf import TSDFVolume
    rng = np.random.default_rng(7)
    blocks = sorted({tuple(b) for b in rng.integers(-40, 40, (24, 3)).tolist()} | {(-1, -1, -1), (0, 0, 0)})
    vol = TSDFVolume(0.01, 0.01, capacity_blocks=32)
    centres = ((np.asarray(blocks, np.float64) * 8 + 4.5) * 0.01).astype(F)            # centre of voxel (4, 4, 4) of each block
    origin = np.array([0.0031, 0.0017, -0.9], F)
    for p in centres:                                                                  # one ray each: +-1 voxel, inside its block
        vol.integrate(torch.from_numpy(p[None]).to(DEV), origin)
    keys = vs.unsigned_keys(vol.keys)
    assert sorted(k for k in keys if k != vs.EMPTY) == sorted(vs.block_key(b) for b in blocks)
    for b in blocks:
        s = vs.find_slot(keys, vs.block_key(b))
        assert s >= 0 and keys[s] == vs.block_key(b)
    _, bc = vol.occupied_blocks()
    assert bc.cpu().numpy().tolist() == [list(b) for b in sorted(blocks, key=vs.block_key)]

    state = tsdf_state(seed=1)
    vol = TSDFVolume(VOXEL, TRUNC, capacity_blocks=16)
    slots = vs.write_tsdf_state(vol, state)
    assert len(set(slots.values())) == len(BLOCKS)
    sl, bc = vol.occupied_blocks()
    assert bc.cpu().numpy().tolist() == [list(b) for b in sorted(BLOCKS)]
    assert sl.cpu().numpy().tolist() == [slots[b] for b in sorted(BLOCKS)]
    c, _, w, s = [x.cpu().numpy() for x in vol.export_voxels()]
    ec, ew, es = tsdf_state_voxels(state)
    assert np.array_equal(c, ec) and np.array_equal(w, ew) and np.array_equal(s, es)

    cstate = color_state(seed=1)
    cvol = ColorTSDFVolume(VOXEL, TRUNC, capacity_blocks=16)
    vs.write_color_state(cvol, cstate)
    model = M.ModelVolume(VOXEL, TRUNC)
    model.blocks = {b: [x.copy() for x in v] for b, v in cstate.items()}
    for x, y in zip(cvol.export_voxels(), model.export_voxels()):
        assert np.array_equal(x.cpu().numpy(), y)


# ------------------------------------------------------------------------------------------------------ TSDFVolume
def tsdf_state(seed):
    """{block: (count, sum_q)}: count 1 .. 5 with 3 % of the voxels unobserved; sum_q uniform in +-count * 2^15 (the mean tsdf
    in +-sdf_trunc, no smoothness at all) with 3 % of the sums exactly 0 (a mean of +0.0: outside, vertex on the voxel)."""
    rng = np.random.default_rng(seed)
    state = {}
    for b in BLOCKS:
        count = rng.integers(1, 6, 512)
        count[rng.random(512) < 0.03] = 0
        sum_q = rng.integers(-count * 32768, count * 32768 + 1)
        sum_q[rng.random(512) < 0.03] = 0
        state[b] = (count.astype(np.int64), sum_q.astype(np.int64))
    return state


def tsdf_state_voxels(state):
    """(coords, count, sum_q) of the observed voxels of a state, sorted by (z, y, x) like export_voxels()."""
    c = np.concatenate([np.asarray(b, np.int64)[None] * 8 + vs.L3 for b in state])
    w = np.concatenate([v[0] for v in state.values()])
    s = np.concatenate([v[1] for v in state.values()])
    m = w > 0
    c, w, s = c[m], w[m], s[m]
    o = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))
    return c[o].astype(np.int32), w[o].astype(np.int32), s[o]


def canon(Vx, Tx):
    out = set()
    for a in Vx.astype(F)[Tx]:
        rows = [tuple(r) for r in a.tolist()]
        k = rows.index(min(rows))
        out.add(tuple(rows[k:] + rows[:k]))                   # rotation-invariant, orientation-preserving
    return out


@pytest.fixture(scope="module")
def tsdf_volume():
    from gaustudio_amd.tsdf import TSDFVolume
    state = tsdf_state(seed=1)
    vol = TSDFVolume(VOXEL, TRUNC, capacity_blocks=16)
    vs.write_tsdf_state(vol, state)
    return state, vol


@pytest.mark.parametrize("min_weight,fill_holes", [(0, True), (0, False), (0.5, False), (1, True), (1.5, True), (2, True), (3, False)])
def test_tsdf_volume_meshes_a_written_state_like_the_oracle(tsdf_volume, min_weight, fill_holes):
    state, vol = tsdf_volume
    count = np.stack([state[b][0] for b in BLOCKS])
    inside = np.stack([state[b][1] for b in BLOCKS]) < 0                       # count 0: sum 0, the background +sdf_trunc
    min_count = 0 if min_weight <= 0 else int(np.ceil(min_weight))
    usable = (count >= min_count) & (fill_holes | (count > 0))
    case, ok, org, node, axis = vs.block_layout(BLOCKS, inside, usable)
    assert (org < 0).all() and (org + np.asarray(case.shape) > 0).all()
    if min_count <= 1:
        assert len(vs.cases_present(case)) == 254 and (case != 0).sum() > 3000
    else:
        assert (case != 0).sum() > 0

    dV, dT = vol.extract_triangle_mesh_device(fill_holes=fill_holes, min_weight=min_weight)
    dV2, dT2 = vol.extract_triangle_mesh_device(fill_holes=fill_holes, min_weight=min_weight)
    assert torch.equal(dV, dV2) and torch.equal(dT, dT2)
    V, T = vol.extract_triangle_mesh(fill_holes=fill_holes, min_weight=min_weight)
    assert V.dtype == np.float64 and T.dtype == np.int32 and np.array_equal(T, dT.cpu().numpy())
    c, w, s = tsdf_state_voxels(state)
    oV, oT = to.extract_mesh(c, w, s, VOXEL, TRUNC, min_weight=min_weight, fill_holes=fill_holes, blocks=set(BLOCKS))
    assert len(T) == len(oT) == int(sm.NTRIS[case].sum())
    assert canon(V, T) == canon(oV, oT)
    assert len(V) == len(oV) == len(node)

    # vertex i of the device is the layout's vertex i: it lies on that grid edge
    base = (node.astype(np.float64) + 0.5) * VOXEL
    off = V - base
    along = off[np.arange(len(V)), axis]
    off[np.arange(len(V)), axis] = 0
    assert np.abs(off).max() < 1e-6 and along.min() > -1e-6 and along.max() < VOXEL + 1e-6
    assert_manifold(T, node, axis, vs.region_extractable(ok, org))


# ------------------------------------------------------------------------------------------------------ ColorTSDFVolume
def color_state(seed):
    """{block: [tsdf, weight, color]} as ModelVolume.blocks holds it: tsdf uniform in (-1, 1) with 3 % +0.0 and 1 % -0.0 (both
    outside), weight in {0, 1, 2, 3} (3 % unobserved, zero like a never observed voxel), integer colours."""
    rng = np.random.default_rng(seed)
    state = {}
    for b in BLOCKS:
        tsdf = rng.uniform(-1, 1, 512).astype(F)
        u = rng.random(512)
        tsdf[u < 0.03] = F(0.0)
        tsdf[(u >= 0.03) & (u < 0.04)] = F(-0.0)
        weight = rng.integers(1, 4, 512).astype(F)
        color = rng.integers(0, 256, (512, 3)).astype(F)
        hole = rng.random(512) < 0.03
        tsdf[hole], weight[hole], color[hole] = 0, 0, 0
        state[b] = [tsdf, weight, color]
    return state


@pytest.fixture(scope="module")
def color_volume():
    from gaustudio_amd import ColorTSDFVolume
    state = color_state(seed=1)
    vol = ColorTSDFVolume(VOXEL, TRUNC, capacity_blocks=16)
    vs.write_color_state(vol, state)
    model = M.ModelVolume(VOXEL, TRUNC)
    model.blocks = {b: [x.copy() for x in v] for b, v in state.items()}
    return state, vol, model


@pytest.mark.parametrize("min_weight", [0, 1.5, 2])
def test_color_volume_meshes_a_written_state_like_the_model(color_volume, min_weight):
    state, vol, model = color_volume
    tsdf = np.stack([state[b][0] for b in BLOCKS])
    weight = np.stack([state[b][1] for b in BLOCKS])
    assert (np.signbit(tsdf) & (tsdf == 0) & (weight > 0)).any() and (~np.signbit(tsdf) & (tsdf == 0) & (weight > 0)).any()
    case, ok, org, node, axis = vs.block_layout(BLOCKS, tsdf < 0, (weight > 0) & (weight >= F(min_weight)))
    if min_weight <= 1:
        assert len(vs.cases_present(case)) == 254 and (case != 0).sum() > 3000
    else:
        assert (case != 0).sum() > 0
    mv, mt, mc = model.extract_triangle_mesh(min_weight)
    v, t, c = vol.extract_triangle_mesh_device(min_weight)
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and c.dtype == torch.float32
    assert tuple(v.shape) == mv.shape and tuple(t.shape) == mt.shape and len(mv) == len(node)
    assert np.array_equal(v.cpu().numpy(), mv), "vertices differ"
    assert np.array_equal(t.cpu().numpy(), mt), "triangles differ"
    assert np.array_equal(c.cpu().numpy(), mc), "colours differ"
    v2, t2, c2 = vol.extract_triangle_mesh_device(min_weight)
    assert torch.equal(v, v2) and torch.equal(t, t2) and torch.equal(c, c2)
    assert_manifold(t.cpu().numpy(), node, axis, vs.region_extractable(ok, org))
