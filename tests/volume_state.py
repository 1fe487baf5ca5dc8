"""Helpers of tests/test_gpu_mc_cases.py (and the table tests of tests/test_tsdf.py).  TEST INFRASTRUCTURE ONLY.

Two things live here:

  * the block hash of the sparse volumes restated on the host (csrc/gsr_block_volume.h: key = three block coordinates, each biased
    by 2^20, in 21-bit fields; empty = all bits set; home slot = mix64(key) & (capacity - 1); linear probing), so that a test
    can WRITE a volume's state -- block keys and voxel words / planes -- instead of reaching it through integrate().  A
    written state holds what no scan of a smooth surface produces: every marching-cubes case, exact zeros, holes, an
    unallocated block in the middle of allocated ones;
  * the index topology every marching-cubes output of this project must have: no directed edge twice, and every edge whose
    neighbouring cubes are all meshed has its reverse exactly once.  It is evaluated on vertex INDICES; which grid edge a
    vertex index stands for comes from the emission order (dense_layout / block_layout), which the callers tie to the
    device's output.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaustudio_amd", "csrc"))
import gen_mc_tables as _tables  # noqa: E402

_M64 = (1 << 64) - 1
BIAS = 1 << 20
EMPTY = _M64
OWNER = [0, 1, 3, 0, 4, 5, 7, 4, 0, 1, 2, 3]      # per cube edge: the corner that owns it (the edge's minimum corner)
AXIS = [0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2]       # and its axis
_LOCAL = np.arange(512)
L3 = np.stack([_LOCAL & 7, (_LOCAL >> 3) & 7, _LOCAL >> 6], axis=1)          # local index -> (lx, ly, lz)


# ------------------------------------------------------------------------------------------------------ block hash
def block_key(b):
    return ((int(b[0]) + BIAS) << 42) | ((int(b[1]) + BIAS) << 21) | (int(b[2]) + BIAS)


def mix64(x):
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & _M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & _M64
    x ^= x >> 31
    return x


def probe_sequence(key, capacity):
    """The slots a lookup of `key` visits, in order."""
    h = mix64(key) & (capacity - 1)
    for i in range(capacity):
        yield (h + i) & (capacity - 1)


def find_slot(keys, key):
    """tsdf_find_slot on a host copy of the key table (a sequence of unsigned ints): the slot of `key`, -1 when absent."""
    for s in probe_sequence(key, len(keys)):
        if keys[s] == key:
            return s
        if keys[s] == EMPTY:
            return -1
    return -1


def place_blocks(blocks, capacity):
    """Inserts the blocks in the given order: (list of unsigned keys [capacity], {block: slot})."""
    assert capacity & (capacity - 1) == 0 and len(blocks) <= capacity
    keys = [EMPTY] * capacity
    slots = {}
    for b in blocks:
        k = block_key(b)
        for s in probe_sequence(k, capacity):
            assert keys[s] != k, f"block {b} twice"
            if keys[s] == EMPTY:
                keys[s] = k
                slots[tuple(b)] = s
                break
    return keys, slots


def unsigned_keys(key_tensor):
    """A volume's int64 key tensor as a list of unsigned ints."""
    return [int(k) & _M64 for k in key_tensor.cpu().tolist()]


def _write_keys(vol, blocks):
    import torch
    keys, slots = place_blocks(blocks, vol.capacity)
    signed = np.array([k - (1 << 64) if k >> 63 else k for k in keys], np.int64)
    vol.keys.copy_(torch.from_numpy(signed))
    return slots


def write_tsdf_state(vol, state):
    """state: {block: (count int64 [512], sum_q int64 [512])}, local index (lz << 6) | (ly << 3) | lx.  Writes the keys and
    the words (sum_q << 24) | count into a fresh TSDFVolume."""
    import torch
    slots = _write_keys(vol, list(state))
    for b, (count, sum_q) in state.items():
        count, sum_q = np.asarray(count, np.int64), np.asarray(sum_q, np.int64)
        assert ((count >= 0) & (count < 1 << 24)).all() and (np.abs(sum_q) < 1 << 39).all()
        vol.voxels[slots[tuple(b)]] = torch.from_numpy(sum_q * (1 << 24) + count).to(vol.voxels.device)
    return slots


def write_color_state(vol, state):
    """state: {block: (tsdf [512], weight [512], color [512, 3])} float32 (what tsdf_rgbd_model.ModelVolume.blocks holds).
    Writes the keys and the five planes tsdf, weight, r, g, b into a fresh ColorTSDFVolume."""
    import torch
    slots = _write_keys(vol, list(state))
    for b, (tsdf, weight, color) in state.items():
        planes = np.concatenate([np.asarray(tsdf, np.float32)[None], np.asarray(weight, np.float32)[None],
                                 np.asarray(color, np.float32).T], axis=0)
        vol.voxels[slots[tuple(b)]] = torch.from_numpy(np.ascontiguousarray(planes)).to(vol.voxels.device)
    return slots


# ------------------------------------------------------------------------------------------------------ emission order
def _cases(inside, n):
    case = np.zeros(tuple(n), np.int64)
    for i, (dx, dy, dz) in enumerate(_tables.CORNERS):
        case |= inside[dx:dx + n[0], dy:dy + n[1], dz:dz + n[2]].astype(np.int64) << i
    return case


def dense_layout(inside):
    """Dense grid (sap.marching_cubes): (case [R0-1,R1-1,R2-1] of every cube, node [nv,3] and axis [nv] of every vertex in
    emission order = (linear index of the edge's lower node, axis))."""
    inside = np.asarray(inside, bool)
    R = inside.shape
    flags = np.zeros(R + (3,), bool)
    flags[:-1, :, :, 0] = inside[:-1] != inside[1:]
    flags[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    flags[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    hit = np.nonzero(flags.reshape(-1))[0]
    node = np.stack(np.unravel_index(hit // 3, R), axis=1).astype(np.int64)
    return _cases(inside, np.asarray(R) - 1), node, (hit % 3).astype(np.int64)


def dense_extractable(shape):
    hi = np.asarray(shape, np.int64) - 1
    return lambda c: ((c >= 0) & (c < hi)).all(axis=1)


def block_layout(blocks, inside, usable):
    """Block-sparse volume.  blocks: block coordinates; inside, usable: bool [len(blocks), 512] per voxel (usable: the voxel
    may be a cube corner under the extraction's min_weight / fill_holes).  A cube is meshed iff its 8 corners lie in
    allocated blocks and are usable, and its case is neither 0 nor 255.  Returns (case [n0,n1,n2] with 0 for cubes that are
    not meshed, ok [n0,n1,n2] = all corners usable, org [3] = voxel coordinates of element [0,0,0], node [nv,3] (voxel
    coordinates) and axis [nv] of every vertex in emission order = (block key, local index of the owning voxel, axis))."""
    _, edge_mask = _tables.build()
    order = sorted(range(len(blocks)), key=lambda i: tuple(blocks[i]))          # key order = lexicographic (bx, by, bz)
    bl = np.asarray([blocks[i] for i in order], np.int64)
    org = bl.min(0) * 8
    dim = (bl.max(0) - bl.min(0) + 1) * 8 + 1
    ins, use, rank = np.zeros(dim, bool), np.zeros(dim, bool), np.full(dim, -1, np.int64)
    for r, i in enumerate(order):
        o = bl[r] * 8 - org
        idx = (o[0] + L3[:, 0], o[1] + L3[:, 1], o[2] + L3[:, 2])
        ins[idx], use[idx], rank[idx] = inside[i], usable[i], r * 512 + _LOCAL
    n = dim - 1
    ok = np.ones(n, bool)
    for dx, dy, dz in _tables.CORNERS:
        ok &= use[dx:dx + n[0], dy:dy + n[1], dz:dz + n[2]]
    case = _cases(ins, n)
    case[~ok | (case == 255)] = 0
    flags = np.zeros(dim, np.int64)
    em = np.asarray(edge_mask)[case]
    for e in range(12):
        dx, dy, dz = _tables.CORNERS[OWNER[e]]
        flags[dx:dx + n[0], dy:dy + n[1], dz:dz + n[2]] |= ((em >> e) & 1) << AXIS[e]
    own = np.argwhere(flags != 0)
    own = own[np.argsort(rank[tuple(own.T)], kind="stable")]
    assert (rank[tuple(own.T)] >= 0).all()
    node, axis = [], []
    for a in range(3):
        m = (flags[tuple(own.T)] >> a) & 1 == 1
        node.append(own[m])
        axis.append(np.stack([rank[tuple(own[m].T)], np.full(m.sum(), a)], axis=1))
    node, axis = np.concatenate(node), np.concatenate(axis)
    o = np.lexsort((axis[:, 1], axis[:, 0]))
    return case, ok, org, node[o] + org, axis[o, 1]


def region_extractable(ok, org):
    """extractable(cubes [k,3] voxel coordinates of their minimum corners) for block_layout's `ok`."""
    hi = np.asarray(ok.shape, np.int64)

    def f(c):
        c = c - org
        inb = ((c >= 0) & (c < hi)).all(axis=1)
        out = np.zeros(len(c), bool)
        out[inb] = ok[tuple(c[inb].T)]
        return out
    return f


# ------------------------------------------------------------------------------------------------------ topology
def edge_topology(tris, node, axis, extractable):
    """tris [nt,3] vertex indices; vertex i sits on the grid edge that leaves node[i] along axis[i].  Returns
    (doubled, missing, interior):
      doubled  = directed edges (a, b) that occur more than once;
      interior = directed edges all of whose cubes are extractable: a triangle edge either joins two grid edges of one cube
                 face -- it lies in that face, its cubes are the two that share the face -- or it is a diagonal through the
                 inside of the one cube that emitted it;
      missing  = interior edges whose reverse (b, a) does not occur exactly once.
    A closed, consistently oriented 2-manifold away from the boundary of the meshed region has doubled == missing == 0."""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    node, axis = np.asarray(node, np.int64), np.asarray(axis, np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    if len(e) == 0:
        return 0, 0, 0
    V = len(node)
    assert e.min() >= 0 and e.max() < V
    uniq, cnt = np.unique(e[:, 0] * V + e[:, 1], return_counts=True)
    back = e[:, 1] * V + e[:, 0]
    pos = np.minimum(np.searchsorted(uniq, back), len(uniq) - 1)
    rev = np.where(uniq[pos] == back, cnt[pos], 0)
    n1, n2, a1, a2 = node[e[:, 0]], node[e[:, 1]], axis[e[:, 0]], axis[e[:, 1]]
    interior = np.ones(len(e), bool)
    for d in range(3):
        face = (a1 != d) & (a2 != d) & (n1[:, d] == n2[:, d])
        upper = np.minimum(n1, n2)[face]                    # minimum corner of the face = of the cube on its far side
        lower = upper.copy()
        lower[:, d] -= 1
        interior[face] = extractable(upper) & extractable(lower)
    return int((cnt > 1).sum()), int((interior & (rev != 1)).sum()), int(interior.sum())


def cases_present(case):
    """the set of non-trivial cases among the meshed cubes"""
    return set(np.unique(case).tolist()) - {0, 255}
