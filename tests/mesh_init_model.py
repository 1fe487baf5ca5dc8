"""The float32 numpy model of gsr_mesh_seeds (csrc/gsr_mesh_bake.hip): MeshInitializer.build_model,
operation for operation -- every intermediate float32, every sum in the kernel's order; the only fused multiply-adds are
the explicit ones of norm3 and cross (the form torch's CPU kernels evaluate); the two logarithms are float32(log(float64(x))).  The GPU tests compare with it exactly; tests/test_mesh_init_model.py compares it with the
reference's own functions (tests/golden/py_mesh_init.npz)."""
import numpy as np

F32 = np.float32
C0 = 0.28209479177387814
S3 = np.sqrt(3.0)

BARY = {
    1: [[1 / 3, 1 / 3, 1 / 3]],
    3: [[1 / 2, 1 / 4, 1 / 4], [1 / 4, 1 / 2, 1 / 4], [1 / 4, 1 / 4, 1 / 2]],
    4: [[1 / 3, 1 / 3, 1 / 3], [2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3]],
    6: [[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3],
        [1 / 6, 5 / 12, 5 / 12], [5 / 12, 1 / 6, 5 / 12], [5 / 12, 5 / 12, 1 / 6]],
}
RADIUS = {1: 1. / 2. / S3, 3: 1. / 2. / (S3 + 1.), 4: 1 / (4. * S3), 6: 1 / (4. + 2. * S3)}


def bary_table(n):
    return np.asarray(BARY[n], dtype=np.float64).astype(F32)


def fma(a, b, c):
    """fmaf: the float64 product of two float32 values is exact, and so is its sum with a float32 except for a double rounding
    that needs a tie at bit 29 of the float64 sum."""
    return (np.asarray(a, dtype=F32).astype(np.float64) * np.asarray(b, dtype=F32).astype(np.float64)
            + np.asarray(c, dtype=F32).astype(np.float64)).astype(F32)


def norm3(u):
    """torch's CPU vector_norm over three entries: sqrt(fma(z, z, fma(y, y, x x)))."""
    return np.sqrt(fma(u[..., 2], u[..., 2], fma(u[..., 1], u[..., 1], u[..., 0] * u[..., 0])))


def normalize(u):
    """F.normalize: x / max(|x|, 1e-12)."""
    return u / np.maximum(norm3(u), F32(1e-12))[..., None]


def sign(x):
    """torch.sign: 0 for NaN."""
    return ((0 < x).astype(F32) - (x < 0).astype(F32)).astype(F32)


def cross(u, v):
    """torch's CPU cross: fma(a, b, -(c d)) per component."""
    return np.stack([fma(u[..., 1], v[..., 2], -(u[..., 2] * v[..., 1])), fma(u[..., 2], v[..., 0], -(u[..., 0] * v[..., 2])),
                     fma(u[..., 0], v[..., 1], -(u[..., 1] * v[..., 0]))], axis=-1)


def log32(x):
    return np.log(np.asarray(x, dtype=F32).astype(np.float64)).astype(F32)


def bary_sum(attr, faces, n):
    """[F * n, 3]: (b0 a0 + b1 a1) + b2 a2 per (face, k)."""
    a = np.asarray(attr, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    b = bary_table(n)[None, :, :, None]                      # [1, n, 3, 1]
    a0, a1, a2 = a[f[:, 0]][:, None], a[f[:, 1]][:, None], a[f[:, 2]][:, None]
    with np.errstate(all="ignore"):
        out = (b[:, :, 0] * a0 + b[:, :, 1] * a1) + b[:, :, 2] * a2
    return out.reshape(-1, 3).astype(F32)


def surface_normals(normals, faces, n):
    """_compute_surface_normals."""
    with np.errstate(all="ignore"):
        return normalize(bary_sum(normals, faces, n))


def normal2rotation_matrix(nrm):
    """The columns (R0, R1, n) of normal2rotation's matrix, each [N,3]."""
    with np.errstate(all="ignore"):
        n = normalize(np.asarray(nrm, dtype=F32).reshape(-1, 3))
        dot = (F32(1) * n[:, 0] + F32(0) * n[:, 1]) + F32(0) * n[:, 2]
        r0 = np.stack([F32(1) - dot * n[:, 0], F32(0) - dot * n[:, 1], F32(0) - dot * n[:, 2]], axis=-1)
        r0 = normalize(r0 * sign(r0[:, 0:1]))
        r1 = cross(n, r0)
        r1 = r1 * (sign(r1[:, 1:2]) * sign(n[:, 2:3]))
    return r0, r1, n


def quaternion(r0, r1, n):
    """rotmat2quaternion of R = [r0 | r1 | n], not normalised: (w, x, y, z)."""
    with np.errstate(all="ignore"):
        tr = ((r0[:, 0] + r1[:, 1]) + n[:, 2]) + F32(1e-6)
        q0 = np.sqrt(F32(1) + tr) / F32(2)
        q4 = F32(4) * q0
        return np.stack([q0, (r1[:, 2] - n[:, 1]) / q4, (n[:, 0] - r0[:, 2]) / q4, (r0[:, 1] - r1[:, 0]) / q4], axis=-1).astype(F32)


def normal2rotation(nrm):
    return quaternion(*normal2rotation_matrix(nrm))


def min_nan(a, b):
    return np.where(a != a, a, np.where(b != b, b, np.where(b < a, b, a)))


def scales(verts, faces, n):
    """_compute_scales: [F * n, 3] raw."""
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(all="ignore"):
        e = min_nan(min_nan(norm3(p0 - p1), norm3(p1 - p2)), norm3(p2 - p0))
        s = e * F32(RADIUS[n])
        s = np.where(s != s, s, np.maximum(s, F32(0)))
        ls = log32(s * F32(2) + F32(1e-7))
    out = np.stack([ls, ls, np.full_like(ls, log32(F32(0) * F32(2) + F32(1e-7)))], axis=-1)
    return np.repeat(out, n, axis=0).astype(F32)


def rgb2sh(rgb):
    with np.errstate(all="ignore"):
        return ((np.asarray(rgb, dtype=F32) - F32(0.5)) / F32(C0)).astype(F32)


def seeds(verts, faces, normals, colors=None, n=1, sh_degree=3):
    """dict(xyz, f_dc [P,1,3], f_rest, opacity, scale, rot) of the P = F * n Gaussians."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    P = f.shape[0] * n
    xyz = bary_sum(verts, f, n)
    rgb = np.ones((P, 3), dtype=F32) if colors is None else bary_sum(colors, f, n)
    return dict(xyz=xyz, f_dc=rgb2sh(rgb).reshape(P, 1, 3), f_rest=np.zeros((P, (sh_degree + 1) ** 2 - 1, 3), dtype=F32),
                opacity=np.full((P, 1), np.inf, dtype=F32), scale=scales(verts, f, n),
                rot=normal2rotation(surface_normals(normals, f, n)))


def random_mesh(num_faces=40, num_verts=30, seed=5):
    """A seeded triangle soup over shared vertices with unit vertex normals and colours: (v, f, normals, colors)."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (num_verts, 3)).astype(F32)
    f = np.stack([rng.permutation(num_verts)[:3] for _ in range(num_faces)]).astype(np.int32)
    nr = rng.normal(size=(num_verts, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(F32)
    return v, f, nr, rng.uniform(0, 1, (num_verts, 3)).astype(F32)
