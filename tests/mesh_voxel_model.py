"""TEST INFRASTRUCTURE: the float64 numpy model of csrc/gsr_voxel.hip (gaustudio_amd/voxelize.py) -- the specification of the
mesh voxelizer behind the reference's VoxelInitializer (gaustudio/pipelines/initializers/mesh.py:252-442).  The kernels perform
these operations in this order; the GPU tests compare exactly.  Every product and sum is written out and evaluated left to
right (no np.dot / einsum / cross): numpy's elementwise float64 +, -, *, / are the IEEE operations the device performs.

  * normalize_mesh      mesh.py:327-352 in float64 from float32 vertices
  * grid_shape          n_d = round((max_bound_d - min_bound_d) / voxel_size), halves away from zero
  * box_centre          the centre the OVERLAP test uses:  (min_bound + h) + i * voxel_size,  h = voxel_size / 2
  * voxel_centre        the centre that is RETURNED:       ((i + 0.5) * voxel_size) + min_bound
                        (Open3D's two formulas as recalled; they coincide when voxel_size is a power of two)
  * tribox              Akenine-Moller's triangle / box separating-axis test with its exact comparisons; touching overlaps
  * tri_box_range       the index-space AABB of a triangle, widened by one voxel, clamped to the grid
  * plane_range         the conservative i2 range of one column from the triangle's plane (a filter only: tribox decides)
  * voxelize_brute      every voxel against every triangle
  * voxelize_boxed      per triangle only the voxels of tri_box_range (optionally narrowed by plane_range)
  * closest_point       Ericson's closest point on a triangle, region tests in his order -> (v, w, d2)
  * closest             per occupied voxel the winner among the triangles of the 27 voxels around it (or among all triangles)
  * seeds               xyz / scale / opacity / f_dc / f_rest of the Gaussians (mesh.py:308-323, 381-442 into
                        models/vanilla_sg.py:69-97), rotations excluded

A voxelization is the dict(voxel_index [nvox] int64 ascending linear indices (i0 n1 + i1) n2 + i2, pair_start [nvox + 1],
pair_tri [npairs] triangles ascending within a voxel, grid_index [nvox, 3])."""
import math

import numpy as np

F = np.float32
D = np.float64
C0 = 0.28209479177387814          # gaustudio/utils/sh_utils.py


# ------------------------------------------------------------------------------------------------------ normalisation / grid
def normalize_mesh(vertices):
    """(vn float64 [nv,3], scale, center [3]) of float32 vertices; ValueError for an extent of zero."""
    v = np.asarray(vertices, dtype=F).astype(D)
    lo, hi = v.min(axis=0), v.max(axis=0)
    center = (lo + hi) / 2
    scale = (hi - lo).max()
    if not scale > 0:
        raise ValueError("the mesh has no extent (scale == 0)")
    vn = np.clip((v - center) / scale, -0.5 + 1e-6, 0.5 - 1e-6)
    return vn, float(scale), center


def grid_shape(voxel_size, min_bound=(-0.5,) * 3, max_bound=(0.5,) * 3):
    return tuple(int(math.floor((float(b) - float(a)) / float(voxel_size) + 0.5)) for a, b in zip(min_bound, max_bound))


def box_centre(i, d, voxel_size, min_bound):
    return (D(min_bound[d]) + D(voxel_size) / 2) + np.asarray(i, dtype=D) * D(voxel_size)


def voxel_centre(i, d, voxel_size, min_bound):
    return ((np.asarray(i, dtype=D) + 0.5) * D(voxel_size)) + D(min_bound[d])


def centres(grid_index, voxel_size, min_bound):
    return np.stack([voxel_centre(grid_index[:, d], d, voxel_size, min_bound) for d in range(3)], axis=1)


# ------------------------------------------------------------------------------------------------------ overlap
def _axis(pa, pb, rad):
    return (np.minimum(pa, pb) > rad) | (np.maximum(pa, pb) < -rad)


def tribox(c, h, t0, t1, t2):
    """Overlap of the box (centre c [...,3], half edge h) and the triangle (t0, t1, t2 [...,3]); broadcasts."""
    c, t0, t1, t2 = (np.asarray(a, dtype=D) for a in (c, t0, t1, t2))
    h = D(h)
    X, Y, Z = 0, 1, 2
    v0 = [t0[..., k] - c[..., k] for k in range(3)]
    v1 = [t1[..., k] - c[..., k] for k in range(3)]
    v2 = [t2[..., k] - c[..., k] for k in range(3)]
    e0 = [v1[k] - v0[k] for k in range(3)]
    e1 = [v2[k] - v1[k] for k in range(3)]
    e2 = [v0[k] - v2[k] for k in range(3)]
    out = np.zeros(np.broadcast(v0[0], v1[0], v2[0]).shape, dtype=bool)      # True = separated

    def x_test(e, va, vb):          # AXISTEST_X: a = e[Z], b = e[Y]
        a, b = e[Z], e[Y]
        rad = np.abs(a) * h + np.abs(b) * h
        return _axis(a * va[Y] - b * va[Z], a * vb[Y] - b * vb[Z], rad)

    def y_test(e, va, vb):          # AXISTEST_Y: a = e[Z], b = e[X]
        a, b = e[Z], e[X]
        rad = np.abs(a) * h + np.abs(b) * h
        return _axis(-a * va[X] + b * va[Z], -a * vb[X] + b * vb[Z], rad)

    def z_test(e, va, vb):          # AXISTEST_Z: a = e[Y], b = e[X]
        a, b = e[Y], e[X]
        rad = np.abs(a) * h + np.abs(b) * h
        return _axis(a * va[X] - b * va[Y], a * vb[X] - b * vb[Y], rad)

    out |= x_test(e0, v0, v2); out |= y_test(e0, v0, v2); out |= z_test(e0, v1, v2)
    out |= x_test(e1, v0, v2); out |= y_test(e1, v0, v2); out |= z_test(e1, v0, v1)
    out |= x_test(e2, v0, v1); out |= y_test(e2, v0, v1); out |= z_test(e2, v1, v2)
    for k in range(3):
        mn = np.minimum(np.minimum(v0[k], v1[k]), v2[k])
        mx = np.maximum(np.maximum(v0[k], v1[k]), v2[k])
        out |= (mn > h) | (mx < -h)
    n = [e0[Y] * e1[Z] - e0[Z] * e1[Y], e0[Z] * e1[X] - e0[X] * e1[Z], e0[X] * e1[Y] - e0[Y] * e1[X]]
    vmin = [np.where(n[k] > 0, -h - v0[k], h - v0[k]) for k in range(3)]
    vmax = [np.where(n[k] > 0, h - v0[k], -h - v0[k]) for k in range(3)]
    dmin = n[0] * vmin[0] + n[1] * vmin[1] + n[2] * vmin[2]
    dmax = n[0] * vmax[0] + n[1] * vmax[1] + n[2] * vmax[2]
    out |= dmin > 0
    out |= ~(dmax >= 0)
    return ~out


def tri_box_range(t0, t1, t2, voxel_size, min_bound, shape):
    """(lo [3], hi [3]) voxel indices, inclusive; lo > hi on an axis = no voxel."""
    lo, hi = [], []
    for d in range(3):
        mn = min(t0[d], t1[d], t2[d])
        mx = max(t0[d], t1[d], t2[d])
        flo = np.floor((D(mn) - D(min_bound[d])) / D(voxel_size)) - 1.0
        fhi = np.floor((D(mx) - D(min_bound[d])) / D(voxel_size)) + 1.0
        lo.append(int(min(max(flo, 0.0), float(shape[d]))))
        hi.append(int(min(max(fhi, -1.0), float(shape[d] - 1))))
    return lo, hi


def plane_range(t0, t1, t2, i0, i1, lo2, hi2, voxel_size, min_bound):
    """Inclusive i2 range [klo, khi] of the columns (i0, i1) (arrays) inside [lo2, hi2] that the triangle's plane can reach.
    The whole range when the normal's component along the column is too small to trust."""
    vs, h = D(voxel_size), D(voxel_size) / 2
    e0 = [D(t1[k]) - D(t0[k]) for k in range(3)]
    e1 = [D(t2[k]) - D(t1[k]) for k in range(3)]
    n = [e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]]
    L = max(max(abs(e0[k]), abs(e1[k])) for k in range(3))
    M = max(max(abs(D(t0[k])), abs(D(t1[k])), abs(D(t2[k]))) for k in range(3))
    nerr = (2.0 ** -40 * L) * (M + L)
    i0, i1 = np.asarray(i0), np.asarray(i1)
    klo = np.full(i0.shape, lo2, dtype=np.int64)
    khi = np.full(i0.shape, hi2, dtype=np.int64)
    if not abs(n[2]) * vs > (32.0 * L) * nerr:
        return klo, khi
    dx = box_centre(i0, 0, voxel_size, min_bound) - D(t0[0])
    dy = box_centre(i1, 1, voxel_size, min_bound) - D(t0[1])
    s = n[0] * dx + n[1] * dy
    zc = D(t0[2]) - s / n[2]
    r = ((abs(n[0]) + abs(n[1])) * h) / abs(n[2])
    flo = np.floor(((zc - r) - D(min_bound[2])) / vs) - 1.0
    fhi = np.floor(((zc + r) - D(min_bound[2])) / vs) + 1.0
    klo = np.minimum(np.maximum(flo, float(lo2)), float(hi2 + 1)).astype(np.int64)
    khi = np.minimum(np.maximum(fhi, float(lo2 - 1)), float(hi2)).astype(np.int64)
    return klo, khi


# ------------------------------------------------------------------------------------------------------ voxelizers
def _result(lin, tri, shape):
    lin, tri = np.asarray(lin, dtype=np.int64), np.asarray(tri, dtype=np.int64)
    order = np.lexsort((tri, lin))
    lin, tri = lin[order], tri[order]
    head = np.ones(lin.shape[0], dtype=bool)
    head[1:] = lin[1:] != lin[:-1]
    voxel_index = lin[head]
    pair_start = np.concatenate([np.flatnonzero(head), [lin.shape[0]]]).astype(np.int64)
    n1, n2 = shape[1], shape[2]
    grid_index = np.stack([voxel_index // (n1 * n2), (voxel_index // n2) % n1, voxel_index % n2], axis=1)
    return dict(voxel_index=voxel_index, pair_start=pair_start, pair_tri=tri, grid_index=grid_index, shape=tuple(shape))


def voxelize_brute(vertices, faces, voxel_size, min_bound, shape):
    v, f = np.asarray(vertices, dtype=D), np.asarray(faces, dtype=np.int64)
    n0, n1, n2 = shape
    i0, i1, i2 = np.meshgrid(np.arange(n0), np.arange(n1), np.arange(n2), indexing="ij")
    c = np.stack([box_centre(i.ravel(), d, voxel_size, min_bound) for d, i in enumerate((i0, i1, i2))], axis=1)
    lin, tri = [], []
    for t in range(f.shape[0]):
        hit = np.flatnonzero(tribox(c, D(voxel_size) / 2, v[f[t, 0]], v[f[t, 1]], v[f[t, 2]]))
        lin.append(hit)
        tri.append(np.full(hit.shape[0], t))
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, dtype=np.int64)
    return _result(cat(lin), cat(tri), shape)


def voxelize_boxed(vertices, faces, voxel_size, min_bound, shape, plane_filter=False, slab=8):
    v, f = np.asarray(vertices, dtype=D), np.asarray(faces, dtype=np.int64)
    n0, n1, n2 = shape
    lin, tri = [], []
    for t in range(f.shape[0]):
        t0, t1, t2 = v[f[t, 0]], v[f[t, 1]], v[f[t, 2]]
        lo, hi = tri_box_range(t0, t1, t2, voxel_size, min_bound, shape)
        if any(l > h_ for l, h_ in zip(lo, hi)):
            continue
        for a in range(lo[0], hi[0] + 1, slab):          # slabs of i0: a large triangle's box in pieces
            i0, i1, i2 = np.meshgrid(np.arange(a, min(a + slab, hi[0] + 1)), np.arange(lo[1], hi[1] + 1),
                                     np.arange(lo[2], hi[2] + 1), indexing="ij")
            i0, i1, i2 = i0.ravel(), i1.ravel(), i2.ravel()
            if plane_filter:
                klo, khi = plane_range(t0, t1, t2, i0, i1, lo[2], hi[2], voxel_size, min_bound)
                keep = (i2 >= klo) & (i2 <= khi)
                i0, i1, i2 = i0[keep], i1[keep], i2[keep]
            c = np.stack([box_centre(i, d, voxel_size, min_bound) for d, i in enumerate((i0, i1, i2))], axis=1)
            hit = tribox(c, D(voxel_size) / 2, t0, t1, t2)
            lin.append(((i0 * n1 + i1) * n2 + i2)[hit])
            tri.append(np.full(int(hit.sum()), t))
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, dtype=np.int64)
    return _result(cat(lin), cat(tri), shape)


# ------------------------------------------------------------------------------------------------------ closest point
def closest_point(p, a, b, c):
    """Ericson, Real-Time Collision Detection 5.1.5, for points p [...,3] and triangles (a, b, c [...,3]): (v, w, d2) with
    the closest point q = a (1 - v - w) + b v + c w evaluated the way his region returns it, d2 = |p - q|^2."""
    p, a, b, c = (np.asarray(x, dtype=D) for x in (p, a, b, c))
    P = [p[..., k] for k in range(3)]
    A = [a[..., k] for k in range(3)]
    B = [b[..., k] for k in range(3)]
    Cc = [c[..., k] for k in range(3)]
    dot = lambda x, y: x[0] * y[0] + x[1] * y[1] + x[2] * y[2]
    sub = lambda x, y: [x[k] - y[k] for k in range(3)]
    ab, ac, ap = sub(B, A), sub(Cc, A), sub(P, A)
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = sub(P, B)
    d3, d4 = dot(ab, bp), dot(ac, bp)
    vc = d1 * d4 - d3 * d2
    cp = sub(P, Cc)
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        # region 7 (interior) first, the earlier regions written over it in reverse order: the first test that holds wins
        denom = 1.0 / ((va + vb) + vc)
        v, w = vb * denom, vc * denom
        q = [(A[k] + ab[k] * v) + ac[k] * w for k in range(3)]
        m = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)                    # edge BC
        wbc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v, w = np.where(m, 1.0 - wbc, v), np.where(m, wbc, w)
        q = [np.where(m, B[k] + wbc * (Cc[k] - B[k]), q[k]) for k in range(3)]
        m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)                                    # edge AC
        wac = d2 / (d2 - d6)
        v, w = np.where(m, 0.0, v), np.where(m, wac, w)
        q = [np.where(m, A[k] + wac * ac[k], q[k]) for k in range(3)]
        m = (d6 >= 0) & (d5 <= d6)                                               # vertex C
        v, w = np.where(m, 0.0, v), np.where(m, 1.0, w)
        q = [np.where(m, Cc[k], q[k]) for k in range(3)]
        m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)                                    # edge AB
        vab = d1 / (d1 - d3)
        v, w = np.where(m, vab, v), np.where(m, 0.0, w)
        q = [np.where(m, A[k] + vab * ab[k], q[k]) for k in range(3)]
        m = (d3 >= 0) & (d4 <= d3)                                               # vertex B
        v, w = np.where(m, 1.0, v), np.where(m, 0.0, w)
        q = [np.where(m, B[k], q[k]) for k in range(3)]
        m = (d1 <= 0) & (d2 <= 0)                                                # vertex A
        v, w = np.where(m, 0.0, v), np.where(m, 0.0, w)
        q = [np.where(m, A[k], q[k]) for k in range(3)]
        dx, dy, dz = P[0] - q[0], P[1] - q[1], P[2] - q[2]
        dd = dx * dx + dy * dy + dz * dz
    return v, w, dd


def closest(vox, vertices, faces, voxel_size, min_bound, vertex_colors=None, neighbourhood=True):
    """dict(closest_tri [nvox] (-1: no candidate with a finite d2), closest_uvw [nvox,3] float64 (0 then), d2 [nvox],
    color [nvox,3] float32 (0.5 then; absent without vertex_colors))."""
    v, f = np.asarray(vertices, dtype=D), np.asarray(faces, dtype=np.int64)
    vi, ps, pt, gi = vox["voxel_index"], vox["pair_start"], vox["pair_tri"], vox["grid_index"]
    n0, n1, n2 = vox["shape"]
    nvox = vi.shape[0]
    q = centres(gi, voxel_size, min_bound)
    if neighbourhood:
        qs, ts = [], []
        for o0 in (-1, 0, 1):
            for o1 in (-1, 0, 1):
                for o2 in (-1, 0, 1):
                    g = gi + np.array([o0, o1, o2])
                    ok = ((g >= 0) & (g < np.array([n0, n1, n2]))).all(axis=1)
                    lin = (g[:, 0] * n1 + g[:, 1]) * n2 + g[:, 2]
                    s = np.searchsorted(vi, lin)
                    ok &= (s < nvox) & (vi[np.minimum(s, nvox - 1)] == lin)
                    for k in np.flatnonzero(ok):
                        tr = pt[ps[s[k]]:ps[s[k] + 1]]
                        qs.append(np.full(tr.shape[0], k))
                        ts.append(tr)
        qs, ts = np.concatenate(qs), np.concatenate(ts)
    else:
        qs = np.repeat(np.arange(nvox), f.shape[0])
        ts = np.tile(np.arange(f.shape[0]), nvox)
    vv, ww, dd = closest_point(q[qs], v[f[ts, 0]], v[f[ts, 1]], v[f[ts, 2]])
    fin = np.isfinite(dd)
    qs, ts, vv, ww, dd = qs[fin], ts[fin], vv[fin], ww[fin], dd[fin]
    order = np.lexsort((ts, dd, qs))                      # by voxel, then d2, then triangle
    qs, ts, vv, ww, dd = qs[order], ts[order], vv[order], ww[order], dd[order]
    first = np.ones(qs.shape[0], dtype=bool)
    first[1:] = qs[1:] != qs[:-1]
    tri = np.full(nvox, -1, dtype=np.int64)
    uvw = np.zeros((nvox, 3), dtype=D)
    best = np.full(nvox, np.inf)
    k = qs[first]
    tri[k] = ts[first]
    best[k] = dd[first]
    uvw[k, 1], uvw[k, 2] = vv[first], ww[first]
    uvw[k, 0] = (1.0 - vv[first]) - ww[first]
    out = dict(closest_tri=tri, closest_uvw=uvw, d2=best)
    if vertex_colors is not None:
        col = np.asarray(vertex_colors, dtype=F).astype(D)
        c = np.full((nvox, 3), 0.5, dtype=D)
        fk = f[tri[k]]
        for ch in range(3):
            c[k, ch] = (col[fk[:, 0], ch] * uvw[k, 0] + col[fk[:, 1], ch] * uvw[k, 1]) + col[fk[:, 2], ch] * uvw[k, 2]
        out["color"] = c.astype(F)
    return out


# ------------------------------------------------------------------------------------------------------ seeds
def rgb2sh(rgb):
    """RGB2SH (sh_utils.py) in float32: (rgb - 0.5) / C0, one rounding per operation."""
    return (np.asarray(rgb, dtype=F) - F(0.5)) / F(C0)


def inverse_sigmoid(x):
    with np.errstate(divide="ignore"):
        return np.log(D(x) / (1.0 - D(x)))


def seeds(centres_normalized, scale, center, voxel_size, rgb=None, sh_degree=3, opacity=1.0):
    """dict(xyz, scale, opacity, f_dc [P,1,3], f_rest [P,(deg+1)^2-1,3]) float32, the raw values the reference stores:
    xyz = float32(centre * scale + center); scale = log(float32(voxel_size * scale * 0.8) + 1e-7) in float32;
    opacity = inverse_sigmoid(opacity) (float64, cast; +inf for the reference's 1.0); f_dc = RGB2SH(rgb), rgb None = ones."""
    c = np.asarray(centres_normalized, dtype=D)
    P = c.shape[0]
    xyz = (c * D(scale) + np.asarray(center, dtype=D)).astype(F)
    s = np.log(F(D(voxel_size) * D(scale) * 0.8) + F(1e-7))
    assert s.dtype == F
    rgb = np.ones((P, 3), dtype=F) if rgb is None else np.asarray(rgb, dtype=F)
    return dict(xyz=xyz, scale=np.full((P, 3), s, dtype=F), opacity=np.full((P, 1), F(inverse_sigmoid(opacity)), dtype=F),
                f_dc=rgb2sh(rgb).reshape(P, 1, 3), f_rest=np.zeros((P, (int(sh_degree) + 1) ** 2 - 1, 3), dtype=F))


# ------------------------------------------------------------------------------------------------------ meshes of the tests
def icosphere(subdivisions=1, radius=1.0):
    """(vertices float32 [nv,3], faces int32 [nf,3]): 20 * 4^subdivisions triangles."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=D) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(F), np.array(f, dtype=np.int32)


def ellipsoid():
    """320 triangles, stretched and shifted."""
    v, f = icosphere(2)
    return (v.astype(D) * np.array([1.7, 0.9, 0.6]) + np.array([0.3, -2.0, 5.0])).astype(F), f


def soup(seed=7, n=40):
    """A seeded soup of n random triangles of mixed sizes."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, (n, 1, 3))
    size = rng.choice([0.05, 0.3, 1.0], (n, 1, 1))
    v = (base + size * rng.uniform(-1, 1, (n, 3, 3))).reshape(-1, 3).astype(F)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def cube(interior_quad=False):
    """The axis-aligned cube [-1, 1]^3 of 12 triangles; interior_quad adds the quad x = 0 (2 triangles)."""
    v = [(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
         (1, 5, 7), (1, 7, 3)]
    if interior_quad:
        v += [(0, -1, -1), (0, 1, -1), (0, 1, 1), (0, -1, 1)]
        f += [(8, 9, 10), (8, 10, 11)]
    return np.array(v, dtype=F), np.array(f, dtype=np.int32)


def cube_shell(n):
    """grid_index [n^3 - (n-2)^3, 3] of the boundary layer of an n^3 grid, in linear-index order."""
    i = np.arange(n)
    full = np.stack(np.meshgrid(i, i, indexing="ij"), axis=-1).reshape(-1, 2)
    ring = full[((full == 0) | (full == n - 1)).any(axis=1)]
    slabs = [np.concatenate([np.full((p.shape[0], 1), a), p], axis=1) for a in range(n) for p in (full if a in (0, n - 1) else ring,)]
    return np.concatenate(slabs)


def colored_sphere(subdivisions=3):
    """(vertices, faces, colors float32 [nv,3]): a unit icosphere coloured by position."""
    v, f = icosphere(subdivisions)
    return v, f, (v.astype(D) * 0.5 + 0.5).astype(F)


def vertex_colors(vertices, seed=3):
    return np.random.default_rng(seed).random((np.asarray(vertices).shape[0], 3)).astype(F)
