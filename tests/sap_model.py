"""CPU model of gaustudio_amd.sap (csrc/gsr_psr.hip), written from the contract in INTEGRATION.md s17 -- not from the reference's
program text.  numpy only (dpsr32_cpu: scipy.fft, for an FFT that stays in single precision).

  * corners(): the per-axis index / weight arithmetic in float32, operation for operation as the contract states it;
  * rasterize(): per node the float32 terms w * val added in float64 (`sum64`), the pair count `k`, sum |term| (`abs64`);
  * interp(): the 8 float32 terms grid[corner] * w added in float64 in corner order;
  * spectral32(): the spectral solve in the device's float32 chain; dpsr64(): the whole solver in float64 (only the weights
    stay float32), the yardstick E_ref is measured against; normalize32(): the float32 chain of normalize_grid;
    dpsr32_cpu(): the whole solver in float32 on the CPU, whose distance from dpsr64 is E_ref where no fixture records one;
  * near_node_coords(): the float32 coordinates beside the nodes of an axis, where the index chain can go wrong;
  * marching_cubes(): the dense indexed marching cubes with the derived tables of gaustudio_amd/csrc/gen_mc_tables.py.
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "gaustudio_amd", "csrc"))
import gen_mc_tables as _tables  # noqa: E402

f32 = np.float32
U = 2.0 ** -24          # unit roundoff of float32


# ------------------------------------------------------------------------------------------------------ indices, weights
def _axis(p, size):
    p = np.asarray(p, f32)
    cs = f32(1.0) / f32(size)
    q = p / cs
    f0 = np.floor(q)
    i0 = f0.astype(np.int64)
    i1 = np.fmod(np.ceil(q), f32(size)).astype(np.int64)
    x0 = f0 * cs
    x1 = (f0 + f32(1.0)) * cs
    w0 = np.abs(p - x1) / cs        # weight of node i0: distance to the opposite corner
    w1 = np.abs(p - x0) / cs        # weight of node i1
    assert q.dtype == f32 and w0.dtype == f32 and w1.dtype == f32
    return (i0, i1), (w0, w1)


def valid(pts, size):
    pts = np.asarray(pts, f32)
    ok = np.isfinite(pts).all(1) & (pts >= 0).all(1) & (pts < 1).all(1)
    for d in range(3):
        with np.errstate(invalid="ignore"):
            ok &= ~(np.floor(pts[:, d] / (f32(1.0) / f32(size[d]))) >= size[d])
    return ok


def near_node_coords(r):
    """The float32 coordinates beside the nodes of an axis of r cells: float32(k / r) for k = 0 .. r and its three float32
    neighbours on each side, those in [0, 1), ascending.  Where 1 / r is no float32 this set holds the coordinates whose
    quotient p / cubesize rounds to an integer off the node, and (r = 100, 129) one below 1 whose quotient rounds up to r."""
    c = (np.arange(r + 1, dtype=np.float64) / r).astype(f32)
    out = [c]
    lo, hi = c, c
    for _ in range(3):
        lo, hi = np.nextafter(lo, f32(-1)), np.nextafter(hi, f32(2))
        out += [lo, hi]
    out = np.unique(np.concatenate(out))
    assert out.dtype == f32
    return out[(out >= 0) & (out < 1)]


def corners(pts, size):
    """node linear index [N,8] (int64) and weight [N,8] (float32) of the 8 corners, corner c = (k0, k1, k2), k0 slowest."""
    pts = np.asarray(pts, f32)
    assert valid(pts, size).all()
    ax = [_axis(pts[:, d], size[d]) for d in range(3)]
    idx = np.empty((len(pts), 8), np.int64)
    w = np.empty((len(pts), 8), f32)
    for c in range(8):
        k = (c >> 2, (c >> 1) & 1, c & 1)
        idx[:, c] = (ax[0][0][k[0]] * size[1] + ax[1][0][k[1]]) * size[2] + ax[2][0][k[2]]
        w[:, c] = (ax[0][1][k[0]] * ax[1][1][k[1]]) * ax[2][1][k[2]]
    return idx, w


# ------------------------------------------------------------------------------------------------------ rasterize, interp
def rasterize(pts, vals, size):
    """-> sum64 [C,R0,R1,R2] float64, k [R0,R1,R2] int64 pairs per node, abs64 [C,...] = sum |term|."""
    vals = np.asarray(vals, f32)
    idx, w = corners(pts, size)
    nn = size[0] * size[1] * size[2]
    C = vals.shape[1]
    k = np.bincount(idx.ravel(), minlength=nn)
    s = np.empty((C, nn))
    a = np.empty((C, nn))
    for c in range(C):
        t = w * vals[:, c:c + 1]
        assert t.dtype == f32
        s[c] = np.bincount(idx.ravel(), weights=t.ravel().astype(np.float64), minlength=nn)
        a[c] = np.bincount(idx.ravel(), weights=np.abs(t).ravel().astype(np.float64), minlength=nn)
    return s.reshape((C,) + tuple(size)), k.reshape(size), a.reshape((C,) + tuple(size))


def rasterize32(pts, vals, size, weighted):
    """what the device returns up to the order of its float64 additions: float32(sum64) [/ float32(max(k, 1)) in float32]."""
    s, k, _ = rasterize(pts, vals, size)
    out = s.astype(f32)
    if weighted:
        out = out / np.maximum(k, 1).astype(f32)[None]
    assert out.dtype == f32
    return out, k


def interp(grid, pts, dtype=f32):
    """-> (samples float64 [N] = sum of the 8 terms, abs64 [N]); terms are float32 products for dtype float32, float64
    products (float32 weights) for a float64 grid."""
    size = grid.shape
    idx, w = corners(pts, size)
    lat = np.asarray(grid, dtype).ravel()[idx]
    t = lat * (w if dtype == f32 else w.astype(np.float64))
    assert t.dtype == dtype
    t = t.astype(np.float64)
    s = np.zeros(len(pts))
    for c in range(8):
        s = s + t[:, c]
    return s, np.abs(t).sum(1)


# ------------------------------------------------------------------------------------------------------ spectral solve
def _freqs(size):
    k0 = np.fft.fftfreq(size[0], d=1.0 / size[0])
    k1 = np.fft.fftfreq(size[1], d=1.0 / size[1])
    k2 = np.fft.rfftfreq(size[2], d=1.0 / size[2])
    return np.meshgrid(k0, k1, k2, indexing="ij")


def gaussian_filter32(size, sig):
    K = _freqs(size)
    dis = np.sqrt(K[0] ** 2 + K[1] ** 2 + K[2] ** 2)
    t = (sig * 2.0) * dis / float(size[0])
    return np.exp(-0.5 * (t * t)).astype(f32)


def spectral32(spec, size, sig):
    """spec complex64 [3,R0,R1,R2h] -> (Phi complex64 [R0,R1,R2h], scale float64 [R0,R1,R2h] = sum_d |N_d| G |w_d| / |Lap + 1e-6|:
    what one float32 rounding of a term is measured against)."""
    spec = np.asarray(spec, np.complex64)
    G = gaussian_filter32(size, sig)
    K = _freqs(size)
    dr = di = lap = None
    scale = np.zeros(G.shape)
    for d in range(3):
        om = (K[d].astype(f32) * f32(2.0)) * f32(np.pi)
        nr, ni = spec[d].real * G, spec[d].imag * G
        tr, ti = ni * om, (-nr) * om
        o2 = om * om
        dr, di, lap = (tr, ti, o2) if d == 0 else (dr + tr, di + ti, lap + o2)
        scale += (np.abs(nr.astype(np.float64)) + np.abs(ni.astype(np.float64))) * np.abs(om.astype(np.float64))
    den = (-lap) + f32(1e-6)
    assert dr.dtype == f32 and den.dtype == f32
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.empty(dr.shape, np.complex64)
        out.real = dr / den
        out.imag = di / den
    out[0, 0, 0] = 0
    return out, scale / np.abs(den.astype(np.float64))


def dpsr64(V, N, size, sig, scale=True, shift=True, weighted=False):
    """The solver in float64 (float32 only in the weights): phi float64 [R0,R1,R2]."""
    s, k, _ = rasterize(V, N, size)
    if weighted:
        s = s / np.maximum(k, 1)[None]
    spec = np.fft.rfftn(s, axes=(1, 2, 3))
    K = _freqs(size)
    dis = np.sqrt(K[0] ** 2 + K[1] ** 2 + K[2] ** 2)
    G = np.exp(-0.5 * ((sig * 2.0) * dis / float(size[0])) ** 2)
    div = np.zeros(G.shape, np.complex128)
    lap = np.zeros(G.shape)
    for d in range(3):
        om = K[d] * 2.0 * np.pi
        div += -1j * spec[d] * G * om          # (Im N w, -Re N w)
        lap -= om * om
    Phi = div / (lap + 1e-6)
    Phi[0, 0, 0] = 0
    phi = np.fft.irfftn(Phi, s=size, axes=(0, 1, 2))
    if shift:
        phi = phi - interp(phi, V, np.float64)[0].mean()
    if scale:
        phi = -phi / abs(phi[0, 0, 0]) * 0.5
    return phi


def normalize32(grid, mean64=None, scale=True, shift=True):
    """normalize_grid without the tanh, in the device's float32 chain (correctly rounded division, no contraction: bit for
    bit): off = float32(mean64); v = grid - off; a = |v[0,0,0]|; (-v) / a * 0.5.  shift=False (or no mean): no offset."""
    v = np.asarray(grid, f32)
    if shift and mean64 is not None:
        v = v - f32(np.float64(mean64))
    if scale:
        a = np.abs(v.reshape(-1)[0])
        with np.errstate(divide="ignore", invalid="ignore"):
            v = (-v) / a * f32(0.5)
    assert v.dtype == f32
    return v


def dpsr32_cpu(V, N, size, sig, scale=True, shift=True):
    """The whole solver in float32 on the CPU: rasterize32 -> scipy rfftn (single precision) -> spectral32 -> scipy irfftn ->
    the mean of the float32 samples -> normalize32.  Its distance from dpsr64 is E_ref of a shape without a recorded fixture:
    the error of a float32 run of the same chain around a different float32 FFT than the device's."""
    import scipy.fft
    size = tuple(size)
    ras, _ = rasterize32(V, N, size, False)
    spec = scipy.fft.rfftn(ras, axes=(1, 2, 3))
    assert spec.dtype == np.complex64, spec.dtype
    Phi, _ = spectral32(spec, size, sig)
    phi = scipy.fft.irfftn(Phi, s=size, axes=(0, 1, 2))
    assert phi.dtype == f32, phi.dtype
    mean = interp(phi, V)[0].astype(f32).astype(np.float64).mean() if shift else None
    return normalize32(phi, mean, scale, shift)


# ------------------------------------------------------------------------------------------------------ marching cubes
_TABLE, _ = _tables.build()
NTRIS = np.array([len(t) for t in _TABLE], np.int64)
TRIS = np.full((256, 5, 3), -1, np.int64)
for _c, _t in enumerate(_TABLE):
    for _q, _tri in enumerate(_t):
        TRIS[_c, _q] = _tri
CORNERS = np.array(_tables.CORNERS, np.int64)                       # offsets along (axis 0, axis 1, axis 2)
EDGE_OWNER = np.array([min(a, b, key=lambda c: tuple(CORNERS[c])) for a, b in _tables.EDGES], np.int64)
EDGE_AXIS = np.array([int(np.nonzero(CORNERS[a] != CORNERS[b])[0][0]) for a, b in _tables.EDGES], np.int64)


def marching_cubes(grid, level=0.0):
    """grid float32 [R0,R1,R2] -> (verts float32 [nv,3] index units, faces int32 [nf,3]).  Inside iff value < level; one
    vertex per crossing edge, owned by the edge's lower node, ordered by (node linear index, axis); triangles by (cube lower
    node linear index, table order)."""
    g = np.ascontiguousarray(grid, f32)
    R = g.shape
    level = f32(level)
    inside = g < level
    stride = (R[1] * R[2], R[2], 1)
    flags = np.zeros(R + (3,), bool)
    flags[:-1, :, :, 0] = inside[:-1] != inside[1:]
    flags[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    flags[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    ff = flags.reshape(-1)
    vid = np.cumsum(ff, dtype=np.int64) - ff                          # exclusive: index of (node, axis) where flagged
    hit = np.nonzero(ff)[0]
    node, axis = hit // 3, hit % 3
    gf = g.reshape(-1)
    a = gf[node]
    b = gf[node + np.asarray(stride)[axis]]
    t = (level - a) / (b - a)
    assert t.dtype == f32
    verts = np.stack([node // stride[0], (node // stride[1]) % R[1], node % R[2]], 1).astype(f32)
    verts[np.arange(len(node)), axis] = verts[np.arange(len(node)), axis] + t

    case = np.zeros((R[0] - 1, R[1] - 1, R[2] - 1), np.int64)
    for c, (dx, dy, dz) in enumerate(CORNERS):
        case |= inside[dx:R[0] - 1 + dx, dy:R[1] - 1 + dy, dz:R[2] - 1 + dz].astype(np.int64) << c
    ci, cj, ck = np.nonzero(NTRIS[case] > 0)                          # C order = ascending linear index of the lower node
    cs = case[ci, cj, ck]
    lin = (ci * R[1] + cj) * R[2] + ck
    tri = TRIS[cs]                                                    # [n,5,3] edges, -1 padded
    ok = tri[:, :, 0] >= 0
    e = np.where(tri >= 0, tri, 0)
    o = EDGE_OWNER[e]
    owner = lin[:, None, None] + CORNERS[o] @ np.asarray(stride)
    faces = vid[owner * 3 + EDGE_AXIS[e]][ok]
    return verts, faces.astype(np.int32)


def edge_counts(faces):
    """directed-edge multiset of a triangle list: {(a, b): n}."""
    import collections
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return collections.Counter(map(tuple, e.tolist()))


def is_closed(faces):
    """every undirected edge in exactly two faces, once in each direction (closed, consistently oriented)."""
    f = np.asarray(faces, np.int64)
    if len(f) == 0:
        return False
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    V = int(f.max()) + 1
    fwd = np.unique(e[:, 0] * V + e[:, 1], return_counts=True)
    if (fwd[1] != 1).any():
        return False
    back = e[:, 1] * V + e[:, 0]
    return bool(np.array_equal(np.sort(back), fwd[0]))


def euler_characteristic(verts, faces):
    f = np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    E = len(np.unique(e[:, 0] * (int(f.max()) + 1) + e[:, 1]))
    return len(np.unique(f)) - E + len(f)


def ellipsoid_cloud(n, seed=0, axes=(1.0, 0.7, 0.5), noise=0.01):
    """noisy ellipsoid surface samples with outward normals (float32)."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    A = np.asarray(axes)
    p = u * A
    nrm = u / A
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    p = p + rng.normal(size=p.shape) * noise
    return p.astype(f32), nrm.astype(f32)


def unit_cube(points):
    """ShapeAsPoints.from_pointcloud's map in float32: center = mean, scale = max|p - center| * 1.2, (p - c) / s -> (x + 1) / 2."""
    p = np.asarray(points, f32)
    center = p.mean(0, dtype=f32)
    scale = f32(np.abs(p - center).max() * f32(1.2))
    return ((p - center) / scale + f32(1.0)) / f32(2.0), center, scale
