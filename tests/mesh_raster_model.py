"""The contract of the mesh rasterizer (csrc/gsr_mesh.hip) restated in numpy.

rasterize(..., dtype=np.float64) is the model: the same formulas in float64 from the float32 inputs.  With
dtype=np.float32 it is the kernel's replay: every value computed in the kernel's operation order, one IEEE float32
operation at a time (numpy never contracts a multiply and an add), so the kernel must match it to the bit.
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


def face_setup(verts, faces, extrinsics, cull_backfaces, dt):
    """Edge functions e [F,3,3] (e_a = b x c, e_b = c x a, e_c = a x b), vertex z [F,3] and the mask of faces that can be
    hit at all (finite vertices; front-facing when culling: ((b - a) x (c - a)) . a < 0)."""
    vc = camera_space(verts, extrinsics, dt)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = vc[faces[:, 0]], vc[faces[:, 1]], vc[faces[:, 2]]
    e = np.stack([cross(b, c), cross(c, a), cross(a, b)], axis=1)
    ok = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
    if cull_backfaces:
        n = cross(b - a, c - a)
        with np.errstate(invalid="ignore"):
            ok &= ((n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2]) < 0
    z = np.stack([a[:, 2], b[:, 2], c[:, 2]], axis=1)
    return e, z, ok


def hits(e, z, dx, dy, z_near, dt):
    """Per (pixel, face) of the given arrays (broadcast): E [..,3], the hit mask, barycentrics [..,3] and z."""
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


def rasterize(verts, faces, intrinsics, extrinsics, height, width, cull_backfaces=False, z_near=0.0, dtype=np.float32,
              pixels=None, chunk=1 << 22):
    """(pix_to_face, zbuf, bary) as flat arrays over `pixels` (default: the whole image, reshaped [H,W], [H,W], [H,W,3]).
    The least (z, face id) wins; -1 on background."""
    dt = dtype
    with np.errstate(all="ignore"):
        e, z, okf = face_setup(verts, faces, extrinsics, cull_backfaces, dt)
        dx, dy = pixel_rays(intrinsics, height, width, dt, pixels)
        n = dx.shape[0]
        bz = np.full(n, np.inf, dtype=dt)
        bf = np.full(n, -1, dtype=np.int64)
        bl = np.full((n, 3), -1, dtype=dt)
        F = e.shape[0]
        step = max(1, chunk // max(n, 1))
        for f0 in range(0, F, step):      # faces in ascending id order: a strict < keeps the lower id on a z tie
            f1 = min(F, f0 + step)
            _, ok, lam, zz = hits(e[None, f0:f1], z[None, f0:f1], dx[:, None], dy[:, None], z_near, dt)
            ok &= okf[None, f0:f1]
            zz = np.where(ok, zz, np.inf)
            k = np.argmin(zz, axis=1)                     # first (lowest id) minimum within the chunk
            zk = zz[np.arange(n), k]
            better = np.isfinite(zk) & (zk < bz)
            bz = np.where(better, zk, bz)
            bf = np.where(better, f0 + k, bf)
            bl = np.where(better[:, None], lam[np.arange(n), k], bl)
    zbuf = np.where(bf >= 0, bz, dt(-1)).astype(np.float32)
    p2f = bf.astype(np.int32)
    bary = bl.astype(np.float32)
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
