"""The contract of the mesh rasterizer (csrc/gsr_mesh.hip) restated in numpy.

rasterize(..., dtype=np.float64) is the model: the same formulas in float64 from the float32 inputs.  With
dtype=np.float32 it is the kernel's replay: every value computed in the kernel's operation order, one IEEE operation at a
time (numpy never contracts a multiply and an add), so the kernel must match it to the bit.  Everything is float32 but two
per-face steps that the kernel takes in float64 from the float32 camera-space vertices: the edge functions' cross
products (rounded to float32 once) and the padded pixel rectangle outside which a face hits nothing (pixel_rect).
"""
import numpy as np


def _f(x, dt):
    return np.asarray(x, dtype=np.float32).astype(dt)


def camera_space(verts, extrinsics, dt):
    """x_c = ((R00 x + R01 y) + R02 z) + t0, ... in dtype dt (the kernel: float32)."""
    v = _f(verts, dt).reshape(-1, 3)
    E = _f(extrinsics, dt)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([((E[r, 0] * x + E[r, 1] * y) + E[r, 2] * z) + E[r, 3] for r in range(3)], axis=1)


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def pixel_rays(intrinsics, height, width, dt, pixels=None):
    """(dx, dy) of the pixels (flat indices i * W + j; default all): ((j + 0.5) - cx) / fx, ((i + 0.5) - cy) / fy."""
    K = _f(intrinsics, dt)
    p = np.arange(height * width) if pixels is None else np.asarray(pixels)
    i, j = (p // width).astype(dt), (p % width).astype(dt)
    half = dt(0.5)
    return ((j + half) - K[0, 2]) / K[0, 0], ((i + half) - K[1, 2]) / K[1, 1]


def cross_rounded(u, v, dt):
    """u x v for face_setup's edge functions.  float32: each component is formed in float64 from the float32 inputs (the
    products are exact there, the one subtraction rounds) and rounded to float32 once, as the kernel does; v x u is still
    the exact negative of u x v.  float64: the plain cross product."""
    if dt is np.float32 or dt == np.float32:
        return cross(u.astype(np.float64), v.astype(np.float64)).astype(np.float32)
    return cross(u, v)


def face_setup(verts, faces, extrinsics, cull_backfaces, dt):
    """Edge functions e [F,3,3] (e_a = b x c, e_b = c x a, e_c = a x b), vertex z [F,3] and the mask of faces that can be
    hit at all (finite vertices; front-facing when culling: ((b - a) x (c - a)) . a < 0, in dt throughout)."""
    vc = camera_space(verts, extrinsics, dt)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = vc[faces[:, 0]], vc[faces[:, 1]], vc[faces[:, 2]]
    e = np.stack([cross_rounded(b, c, dt), cross_rounded(c, a, dt), cross_rounded(a, b, dt)], axis=1)
    ok = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
    if cull_backfaces:
        n = cross(b - a, c - a)
        with np.errstate(invalid="ignore"):
            ok &= ((n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2]) < 0
    z = np.stack([a[:, 2], b[:, 2], c[:, 2]], axis=1)
    return e, z, ok


def _key_factors(dt):
    one, eps = dt(1), dt(1) / dt(65536)
    return one - eps, one + eps


def face_key(vc, faces, z_near):
    """The sort key of face_setup, in vc's dtype (the kernel: float32): min z_k shrunk by 2^-16 relative (grown when
    negative), at least z_near, with -0 turned into +0.  A lower bound of every z the face can produce."""
    dt = vc.dtype.type
    shrink, grow = _key_factors(dt)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    zmin = vc[faces, 2].min(axis=1)
    with np.errstate(all="ignore"):
        return np.maximum(np.where(zmin > 0, zmin * shrink, zmin * grow), np.float32(z_near).astype(dt)) + dt(0)


def _extent_add(lo, hi, m, p, z, f, c, tol):
    """extent_add of the kernel on the faces of mask m: u = f (p / z) + c for z > 0, else a direction to infinity."""
    front = z > 0.0
    u = f * (p / z) + c
    s = f * p
    mf, mi = m & front, m & ~front
    lo = np.where(mf, np.fmin(lo, u), lo)
    hi = np.where(mf, np.fmax(hi, u), hi)
    hi = np.where(mi & ~(s < tol), np.inf, hi)
    lo = np.where(mi & ~(s > -tol), -np.inf, lo)
    return lo, hi


def _pixel_span(lo, hi, n):
    """First pixel whose centre is >= lo - 1 and last whose centre is <= hi + 1, clamped to [0, n - 1]; (1, 0) if none."""
    a = np.fmax(np.ceil(lo - 1.5), 0.0)
    b = np.fmin(np.floor(hi + 0.5), float(n - 1))
    ok = a <= b
    return np.where(ok, a, 1.0).astype(np.int64), np.where(ok, b, 0.0).astype(np.int64)


def pixel_rect(vc, faces, intrinsics, height, width, z_near):
    """face_setup's padded pixel rectangle, operation for operation in float64 from the camera-space vertices vc (the
    kernel's: float32): the face clipped against z = z_near (1 - 2^-12), its projected extent, one pixel of padding.
    Returns rect [F,4] int64 = (x0, y0, x1, y1), inclusive, and the mask of faces that are binned at all: finite,
    no two coincident vertices, not wholly at or below z_near (max z_k grown by 2^-16), a non-empty rectangle.
    A face can hit only pixels x0 <= j <= x1, y0 <= i <= y1."""
    dt = vc.dtype.type
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    K = _f(intrinsics, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    zn = np.float32(z_near)
    with np.errstate(all="ignore"):
        P = vc[faces]                                             # [F,3,3] in dt
        ok = np.isfinite(P).all((1, 2))
        for k in range(3):
            ok &= ~(P[:, k] == P[:, (k + 1) % 3]).all(1)
        zmax = P[:, :, 2].max(1)
        grow = _key_factors(dt)[1]
        ok &= np.where(zmax > 0, zmax * grow, zmax) > zn.astype(dt)
        P = np.where(ok[:, None, None], P, dt(1)).astype(np.float64)
        zc = float(zn) * (1.0 - 1.0 / 4096.0)
        F = P.shape[0]
        xlo, xhi = np.full(F, np.inf), np.full(F, -np.inf)
        ylo, yhi = np.full(F, np.inf), np.full(F, -np.inf)
        for k in range(3):
            p, q = P[:, k], P[:, (k + 1) % 3]
            pin, qin = p[:, 2] > zc, q[:, 2] > zc
            xlo, xhi = _extent_add(xlo, xhi, pin, p[:, 0], p[:, 2], fx, cx, 0.0)
            ylo, yhi = _extent_add(ylo, yhi, pin, p[:, 1], p[:, 2], fy, cy, 0.0)
            cr = pin != qin                                       # the edge crosses the plane
            t = (zc - p[:, 2]) / (q[:, 2] - p[:, 2])
            x, y = p[:, 0] + t * (q[:, 0] - p[:, 0]), p[:, 1] + t * (q[:, 1] - p[:, 1])
            tx = 1e-9 * (np.abs(p[:, 0]) + np.abs(q[:, 0])) * abs(fx)
            ty = 1e-9 * (np.abs(p[:, 1]) + np.abs(q[:, 1])) * abs(fy)
            zcv = np.full(F, zc)
            xlo, xhi = _extent_add(xlo, xhi, cr, x, zcv, fx, cx, tx)
            ylo, yhi = _extent_add(ylo, yhi, cr, y, zcv, fy, cy, ty)
        x0, x1 = _pixel_span(xlo, xhi, width)
        y0, y1 = _pixel_span(ylo, yhi, height)
    ok &= (x0 <= x1) & (y0 <= y1)
    return np.stack([x0, y0, x1, y1], axis=1), ok


def hits(e, z, dx, dy, z_near, dt):
    """Per (pixel, face) of the given arrays (broadcast), the rectangle ignored: E [..,3], the hit mask, barycentrics
    [..,3] and z."""
    E = np.stack([(e[..., k, 0] * dx + e[..., k, 1] * dy) + e[..., k, 2] for k in range(3)], axis=-1)
    pos = (E >= 0).all(-1)
    neg = (E <= 0).all(-1)
    S = (E[..., 0] + E[..., 1]) + E[..., 2]
    cov = (pos | neg) & (S != 0)
    Ss = np.where(cov, S, dt(1))
    lam = E / Ss[..., None]
    zz = (lam[..., 0] * z[..., 0] + lam[..., 1] * z[..., 1]) + lam[..., 2] * z[..., 2]
    ok = cov & (zz > np.float32(z_near).astype(dt)) & (zz < np.inf)
    return E, ok, lam, zz


def in_rect(rect, i, j):
    """[pixels, faces]: pixel (i, j) lies in the face's rectangle."""
    i, j = np.asarray(i)[:, None], np.asarray(j)[:, None]
    return (j >= rect[None, :, 0]) & (j <= rect[None, :, 2]) & (i >= rect[None, :, 1]) & (i <= rect[None, :, 3])


def rasterize(verts, faces, intrinsics, extrinsics, height, width, cull_backfaces=False, z_near=0.0, dtype=np.float32,
              pixels=None, chunk=1 << 21):
    """(pix_to_face, zbuf, bary) as flat arrays over `pixels` (default: the whole image, reshaped [H,W], [H,W], [H,W,3]).
    A face hits only inside its pixel_rect; the least (z, face id) wins; -1 on background.  Brute force over every
    (face, pixel of its rectangle) pair."""
    dt = dtype
    with np.errstate(all="ignore"):
        e, z, okf = face_setup(verts, faces, extrinsics, cull_backfaces, dt)
        rect, okr = pixel_rect(camera_space(verts, extrinsics, dt), faces, intrinsics, height, width, z_near)
        ids = np.flatnonzero(okf & okr)       # ascending: only these can hit
        e, z, rect = e[ids], z[ids], rect[ids]
        want = np.arange(height * width) if pixels is None else np.asarray(pixels, dtype=np.int64)
        p, inverse = np.unique(want, return_inverse=True)
        dx, dy = pixel_rays(intrinsics, height, width, dt, p)
        n = p.shape[0]
        slot = np.full(height * width, -1, dtype=np.int64)      # where a pixel's result goes
        slot[p] = np.arange(n)
        bz = np.full(n, np.inf, dtype=dt)
        bf = np.full(n, -1, dtype=np.int64)
        bl = np.full((n, 3), -1, dtype=dt)
        w = rect[:, 2] - rect[:, 0] + 1
        end = np.cumsum(w * (rect[:, 3] - rect[:, 1] + 1))
        f0, F = 0, e.shape[0]
        while f0 < F:                          # faces in ascending id order, about `chunk` pairs at a time
            f1 = max(f0 + 1, int(np.searchsorted(end, (end[f0 - 1] if f0 else 0) + chunk, side="right")))
            cnt = np.diff(end[f0:f1], prepend=end[f0 - 1] if f0 else 0)
            fi = np.repeat(np.arange(f0, f1), cnt)
            k = np.arange(fi.shape[0]) - np.repeat(end[f0:f1] - cnt - (end[f0 - 1] if f0 else 0), cnt)
            q = slot[(rect[fi, 1] + k // w[fi]) * width + rect[fi, 0] + k % w[fi]]
            fi, q = fi[q >= 0], q[q >= 0]
            _, ok, lam, zz = hits(e[fi], z[fi], dx[q], dy[q], z_near, dt)
            fi, q, lam, zz = fi[ok], q[ok], lam[ok], zz[ok]
            order = np.lexsort((fi, zz, q))                 # per pixel the least (z, id) of the chunk first
            first = order[np.flatnonzero(np.diff(q[order], prepend=-1))]
            first = first[zz[first] < bz[q[first]]]         # a strict < keeps the lower id of an earlier chunk on a z tie
            bz[q[first]], bf[q[first]], bl[q[first]] = zz[first], ids[fi[first]], lam[first]
            f0 = f1
    zbuf = np.where(bf >= 0, bz, dt(-1)).astype(np.float32)[inverse]
    p2f = bf.astype(np.int32)[inverse]
    bary = bl.astype(np.float32)[inverse]
    if pixels is None:
        return p2f.reshape(height, width), zbuf.reshape(height, width), bary.reshape(height, width, 3)
    return p2f, zbuf, bary


def interpolate(faces, p2f, bary, attr):
    """(b0 A[f0] + b1 A[f1]) + b2 A[f2] in float32, 0 on background."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    A = np.asarray(attr, dtype=np.float32)
    A = A.reshape(A.shape[0], -1)
    m = p2f >= 0
    out = np.zeros(p2f.shape + (A.shape[1],), dtype=np.float32)
    fc = faces[p2f[m]]
    w = bary[m].astype(np.float32)
    out[m] = (w[:, 0:1] * A[fc[:, 0]] + w[:, 1:2] * A[fc[:, 1]]) + w[:, 2:3] * A[fc[:, 2]]
    return out


def vertex_normals(verts, faces):
    """Meshes.verts_normals_packed with the sum in ascending (face, corner) order, float32: corner k adds
    (v[k+1] - v[k]) x (v[k+2] - v[k]); n / max(|n|, 1e-6)."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    contrib = np.empty((faces.shape[0], 3, 3), dtype=np.float32)
    for k in range(3):
        p0, p1, p2 = v[faces[:, k]], v[faces[:, (k + 1) % 3]], v[faces[:, (k + 2) % 3]]
        contrib[:, k] = cross(p1 - p0, p2 - p0)
    acc = np.zeros_like(v)
    np.add.at(acc, faces.reshape(-1), contrib.reshape(-1, 3))     # unbuffered, in order of appearance
    d = np.maximum(np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2]), np.float32(1e-6))
    return acc / d[:, None]


def normal_map(faces, p2f, vnormals, extrinsics):
    """render_mesh.py:348-353 in float64 over get_normals_from_fragments (:65-74), which interpolates with barycentrics of
    ones: the sum of the hit face's three vertex normals (float32, in corner order), normalize, @ c2w R, negate y and z."""
    n = interpolate(faces, p2f, np.ones(p2f.shape + (3,), np.float32), vnormals).astype(np.float64)
    ln = np.linalg.norm(n, axis=-1, keepdims=True)
    n = n / np.maximum(ln, 1e-12)
    c2w_R = np.linalg.inv(np.asarray(extrinsics, dtype=np.float64))[:3, :3]
    n = n @ c2w_R
    return n * np.array([1.0, -1.0, -1.0])


def visible_faces(p2f, num_faces):
    vis = np.zeros(num_faces, dtype=bool)
    vis[p2f[p2f >= 0]] = True
    return vis


# ------------------------------------------------------------------------------------------------ test meshes
def icosphere(subdiv):
    """Unit icosphere, outward winding ((b - a) x (c - a) points out); 20 * 4^subdiv faces."""
    t = (1.0 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    faces = f
    for _ in range(subdiv):
        cache = {}

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in cache:
                m = verts[i] + verts[j]
                verts.append(m / np.linalg.norm(m))
                cache[key] = len(verts) - 1
            return cache[key]
        nf = []
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nf
    return np.array(verts, dtype=np.float32), np.array(faces, dtype=np.int32)


def grid_mesh(nx, ny, x0, y0, step, z, flip=False):
    """A z = const grid of (nx x ny) quads, two triangles each; vertex (ix, iy) at (x0 + ix step, y0 + iy step, z)."""
    ix, iy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    verts = np.stack([x0 + ix * step, y0 + iy * step, np.full(ix.shape, z)], axis=-1).reshape(-1, 3).astype(np.float32)
    faces = []
    for y in range(ny):
        for x in range(nx):
            a = y * (nx + 1) + x
            b, c, d = a + 1, a + nx + 1, a + nx + 2
            faces += [(a, c, b), (b, c, d)] if not flip else [(a, b, c), (b, d, c)]
    return verts, np.array(faces, dtype=np.int32)


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """World-to-camera 4x4 in OpenCV axes (x right, y down, z forward) for a camera at `eye` looking at `target`."""
    eye, target, up = (np.asarray(x, dtype=np.float64) for x in (eye, target, up))
    zc = target - eye
    zc /= np.linalg.norm(zc)
    xc = np.cross(zc, up)
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    R = np.stack([xc, yc, zc])
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ eye
    return E


def random_scene(rng, F, crossing=False):
    """F random faces over 2 F vertices: in front of the camera, or (crossing) a cloud around it, where many faces cross
    the camera plane."""
    V = 2 * F
    if crossing:
        v = rng.uniform(-2, 2, size=(V, 3)) + [0, 0, 0.8]
    else:
        v = rng.uniform(-1, 1, size=(V, 3)) * [1.2, 1.0, 0.7] + [0, 0, 3]
    f = rng.integers(0, V, size=(F, 3))
    return v.astype(np.float32), f.astype(np.int32)


def sphere_grid(nu, nv, seed=0):
    """A bumpy closed-ish sphere from an nu x nv lat-long grid: 2 nu nv faces."""
    rng = np.random.default_rng(seed)
    th = (np.arange(nv + 1) + 0.5) / (nv + 1) * np.pi
    ph = np.arange(nu) / nu * 2 * np.pi
    T, P = np.meshgrid(th, ph, indexing="ij")
    r = 1 + 0.05 * np.sin(7 * P) * np.sin(5 * T) + 0.002 * rng.random(T.shape)
    v = np.stack([r * np.sin(T) * np.cos(P), r * np.cos(T), r * np.sin(T) * np.sin(P)], -1).reshape(-1, 3)
    iv, iu = np.meshgrid(np.arange(nv), np.arange(nu), indexing="ij")
    a = iv * nu + iu
    b = iv * nu + (iu + 1) % nu
    c, d = a + nu, b + nu
    f = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)])
    return v.astype(np.float32), f.astype(np.int32)


def _soup(a, b, c):
    F = len(a)
    v = np.concatenate([a, b, c]).astype(np.float32)
    return v, np.stack([np.arange(F), F + np.arange(F), 2 * F + np.arange(F)], axis=1).astype(np.int32)


def intrinsics(fx, cx, cy, fy=None):
    return np.array([[fx, 0, cx], [0, fx if fy is None else fy, cy], [0, 0, 1]], dtype=np.float64)


# (fx = fy, cx = cy offset pair, short, z0, spread): the needle sets of tests/test_mesh_raster_model.py.  The first five
# are well conditioned for float64-then-rounded edge functions (no hit outside the padded rectangle); in the last two the
# rectangle clips hits.
NEEDLES_WELL = [(1500, (40, 32), 0.2, 3, 0.1), (1500, (-1000, -800), 0.2, 3, 0.1), (1500, (-1000, -800), 0.05, 50, 0.3),
                (4000, (-3000, -2500), 0.2, 3, 0.1), (4000, (-3000, -2500), 0.05, 3, 0.3)]
NEEDLES_PATHOLOGICAL = [(4000, (-8000, -8000), 0.005, 3, 0.3), (12000, (-8000, -8000), 0.001, 100, 0.5)]


def needles(rng, F, height, width, f, c, short, z0, spread):
    """F thin triangles for an identity camera with fx = fy = f, (cx, cy) = c: the apex in the image, 3..25 px long, the
    short edge 0.1..1 x `short` px, each vertex at depth z0 (1 +- spread).  Returns verts, faces, intrinsics."""
    cx, cy = c
    pa = rng.uniform([4, 4], [width - 4, height - 4], (F, 2))
    ang = rng.uniform(0, 2 * np.pi, F)
    d = np.stack([np.cos(ang), np.sin(ang)], 1)
    mid = pa + d * rng.uniform(3, 25, (F, 1))
    nrm = np.stack([-d[:, 1], d[:, 0]], 1)
    ls = short * 10.0 ** rng.uniform(-1, 0, (F, 1))

    def unproject(p):
        z = z0 * (1 + spread * rng.uniform(-1, 1, (len(p), 1)))
        return np.concatenate([(p[:, 0:1] - cx) / f * z, (p[:, 1:2] - cy) / f * z, z], 1)
    v, faces = _soup(unproject(pa), unproject(mid + nrm * ls / 2), unproject(mid - nrm * ls / 2))
    return v, faces, intrinsics(f, cx, cy)


def radial_edge_faces(rng, F, scale=1.0):
    """Faces whose edge (b, c) lies on one ray through the camera centre up to noise of 1e-5..0.3."""
    a = rng.uniform(-1, 1, (F, 3)) * [1.5, 1.2, 0] + [0, 0, 1]
    a *= rng.uniform(0.5, 4, (F, 1))
    d = rng.uniform(-1, 1, (F, 3)) * [0.6, 0.5, 0] + [0, 0, 1]
    b = d * rng.uniform(0.5, 3, (F, 1))
    c = d * rng.uniform(3, 50, (F, 1)) + rng.normal(size=(F, 3)) * 10.0 ** rng.uniform(-5, -0.5, (F, 1))
    return _soup(a * scale, b * scale, c * scale)


def camera_plane_faces(rng, F):
    """Random faces around the camera, many crossing its plane, with vertices at camera z = 0 and +-1e-30."""
    v = (rng.uniform(-2, 2, (3 * F, 3)) + [0, 0, 0.3]).astype(np.float32)
    v[rng.random(3 * F) < 0.15, 2] = 0.0
    v[rng.random(3 * F) < 0.1, 2] = np.float32(1e-30)
    v[rng.random(3 * F) < 0.1, 2] = np.float32(-1e-30)
    return v, rng.integers(0, 3 * F, (F, 3)).astype(np.int32)


def edge_on_faces(rng, F):
    """Faces whose plane passes within 1e-8..1e-4 of the camera centre."""
    n = rng.normal(size=(F, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)

    def in_plane():
        x = rng.uniform(-1, 1, (F, 3)) * [3, 3, 0] + [0, 0, 1]
        x *= rng.uniform(0.3, 20, (F, 1))
        x -= n * (x * n).sum(1, keepdims=True)
        return x + n * rng.normal(size=(F, 1)) * 10.0 ** rng.uniform(-8, -4, (F, 1))
    return _soup(in_plane(), in_plane(), in_plane())


def sliver_sphere(nlon, nlat, radius=1.0):
    """A closed lat-long sphere, outward winding: nlat rings of nlon vertices, two triangles per quad between rings and a
    fan to each pole: 2 nlon nlat faces, all of them slivers for nlon >> nlat."""
    th = (np.arange(nlat) + 1) / (nlat + 1) * np.pi
    ph = np.arange(nlon) / nlon * 2 * np.pi
    T, P = np.meshgrid(th, ph, indexing="ij")
    ring = np.stack([np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)], -1).reshape(-1, 3)
    v = np.concatenate([ring, [[0, 1, 0], [0, -1, 0]]]) * radius
    north, south = nlat * nlon, nlat * nlon + 1
    iv, iu = np.meshgrid(np.arange(nlat - 1), np.arange(nlon), indexing="ij")
    a = (iv * nlon + iu).ravel()
    b = (iv * nlon + (iu + 1) % nlon).ravel()
    c, d = a + nlon, b + nlon
    u = np.arange(nlon)
    un = (u + 1) % nlon
    last = (nlat - 1) * nlon
    f = np.concatenate([np.stack([a, b, c], -1), np.stack([b, d, c], -1),
                        np.stack([np.full(nlon, north), un, u], -1), np.stack([np.full(nlon, south), last + u, last + un], -1)])
    return v.astype(np.float32), f.astype(np.int32)
