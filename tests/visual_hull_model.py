"""TEST INFRASTRUCTURE: numpy models of csrc/gsr_hull.hip (gaustudio_amd/visual_hull.py).

  * pack_bits / unpack_bits  the packed mask layout: bit x & 31 of word y * stride + (x >> 5), stride = ceil(W / 32)
  * carve                    float32, every operation of the kernel in its order (one rounding per operation, correctly
                             rounded divide): the GPU tests compare with it exactly
  * replay64                 the same decisions in float64 and, per voxel and camera, the distance to the nearest decision
                             boundary -- clip.z = 0, |ndc| = 1, or an integer pixel edge across which the mask changes --
                             in clip / ndc / pixel units: a voxel on which two float32 evaluations with different summation
                             orders disagree must sit that close to one
  * mesh helpers             edge manifoldness and signed volume of an indexed triangle mesh

A camera is (M float32 [4,4] = full_proj_transform of the reference, row-vector convention, W, H); voxel (i, j, k) of the grid
[R0, R1, R2] sits at (ax_x[j], ax_y[i], ax_z[k]) (np.meshgrid's default 'xy' indexing, mask.py:43-48)."""
import numpy as np

F = np.float32


def pack_bits(mask):
    """(words uint32 [H * stride], stride): a pixel is set iff its value is nonzero (NaN is nonzero)."""
    m = np.asarray(mask)
    H, W = m.shape
    stride = (W + 31) // 32
    bits = np.zeros((H, stride * 32), dtype=np.uint64)
    bits[:, :W] = (m != 0)
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    words = (bits.reshape(H, stride, 32) * weights).sum(axis=2).astype(np.uint32)
    return words.reshape(-1), stride


def unpack_bits(words, stride, W, H):
    w = np.asarray(words, dtype=np.uint32).reshape(H, stride)
    x = np.arange(W)
    return ((w[:, x >> 5] >> (x & 31).astype(np.uint32)) & 1).astype(bool)


def grid_points(axes):
    """Flat (x, y, z) float32 vectors of the grid, index (i R1 + j) R2 + k."""
    ax_x, ax_y, ax_z = (np.asarray(a, dtype=F) for a in axes)
    R1, R0, R2 = len(ax_x), len(ax_y), len(ax_z)
    i, j, k = np.meshgrid(np.arange(R0), np.arange(R1), np.arange(R2), indexing="ij")
    return ax_x[j.ravel()], ax_y[i.ravel()], ax_z[k.ravel()], (R0, R1, R2)


def _clip32(M, x, y, z):
    M = np.asarray(M, dtype=F)
    return [((x * M[0, c] + y * M[1, c]) + z * M[2, c]) + M[3, c] for c in range(4)]


def inside_view32(cam, mask, x, y, z):
    """Camera.insideView (datasets/__init__.py:268-305) in float32 with the kernel's summation order; the mask is read
    through its packed bits.  mask None: every point inside the view is kept."""
    M, W, H = cam
    with np.errstate(all="ignore"):
        cx, cy, cz, cw = _clip32(M, x, y, z)
        nx, ny = cx / cw, cy / cw
        keep = (cz > 0) & (nx >= -1) & (nx <= 1) & (ny >= -1) & (ny <= 1)
        if mask is None:
            return keep
        fx = ((nx + F(1)) * F(0.5)) * F(W)
        fy = ((F(1) + ny) * F(0.5)) * F(H)
        px = np.clip(np.where(keep, fx, 0).astype(np.int64), 0, W - 1)
        py = np.clip(np.where(keep, fy, 0).astype(np.int64), 0, H - 1)
    words, stride = pack_bits(mask)
    bit = (words[py * stride + (px >> 5)] >> (px & 31).astype(np.uint32)) & 1
    return keep & (bit != 0)


def carve(axes, cameras, masks, per_camera=False):
    """(filled bool [R0,R1,R2], count, carved_by int32 [R0,R1,R2]): carved_by = the first camera in list order that does not
    keep the voxel, -1 for a filled one.  per_camera: a fourth value, keep [ncam, R0 R1 R2] without the early exit."""
    x, y, z, res = grid_points(axes)
    alive = np.ones(x.shape[0], dtype=bool)
    who = np.full(x.shape[0], -1, dtype=np.int32)
    keeps = []
    for c, (cam, mask) in enumerate(zip(cameras, masks)):
        keep = inside_view32(cam, mask, x, y, z)
        keeps.append(keep)
        first = alive & ~keep
        who[first] = c
        alive &= keep
    out = (alive.reshape(res), int(alive.sum()), who.reshape(res))
    return out + (np.stack(keeps),) if per_camera else out


def replay64(axes, cameras, masks):
    """(keep [ncam, n] bool, margin [ncam, n] float64): the float64 decisions on the float32 inputs and the distance of each
    to its nearest boundary.  Boundaries whose crossing cannot change the decision are still counted (the margin is a lower
    bound of the true one), except pixel edges: only edges to a neighbouring pixel with another mask value count."""
    x, y, z, _ = grid_points(axes)
    x, y, z = x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)
    keeps, margins = [], []
    for (M, W, H), mask in zip(cameras, masks):
        M = np.asarray(M, dtype=np.float64)
        with np.errstate(all="ignore"):
            cx, cy, cz, cw = [x * M[0, c] + y * M[1, c] + z * M[2, c] + M[3, c] for c in range(4)]
            nx, ny = cx / cw, cy / cw
            keep = (cz > 0) & (nx >= -1) & (nx <= 1) & (ny >= -1) & (ny <= 1)
            margin = np.minimum.reduce([np.abs(cz), np.abs(np.abs(nx) - 1), np.abs(np.abs(ny) - 1)])
            margin = np.where(np.isfinite(margin), margin, np.inf)
            if mask is not None:
                m = np.asarray(mask) != 0
                fx, fy = (nx + 1) * 0.5 * W, (1 + ny) * 0.5 * H
                ok = keep & np.isfinite(fx) & np.isfinite(fy)
                px = np.clip(np.where(ok, fx, 0).astype(np.int64), 0, W - 1)
                py = np.clip(np.where(ok, fy, 0).astype(np.int64), 0, H - 1)
                here = m[py, px]
                # distance to the four edges of the pixel (a coordinate clamped into the last pixel has no edge beyond it)
                dl, dr = fx - px, np.where(px == W - 1, np.inf, px + 1 - fx)
                dt, db = fy - py, np.where(py == H - 1, np.inf, py + 1 - fy)
                edge = np.full(x.shape[0], np.inf)
                for sx, ddx in ((-1, dl), (0, None), (1, dr)):
                    for sy, ddy in ((-1, dt), (0, None), (1, db)):
                        if sx == 0 and sy == 0:
                            continue
                        qx, qy = np.clip(px + sx, 0, W - 1), np.clip(py + sy, 0, H - 1)
                        d = ddx if ddy is None else ddy if ddx is None else np.maximum(ddx, ddy)
                        edge = np.where(m[qy, qx] != here, np.minimum(edge, d), edge)
                margin = np.where(ok, np.minimum(margin, edge), margin)
                keep = keep & here
        keeps.append(keep)
        margins.append(margin)
    return np.stack(keeps), np.stack(margins)


def unattributed(model_keep, ref_keep, margin, tol=1e-4):
    """Indices (camera, voxel) where the two per-camera decisions differ although the float64 replay sees no boundary within
    tol, and the number of differing decisions."""
    diff = np.asarray(model_keep) != np.asarray(ref_keep)
    bad = diff & ~(margin < tol)
    return np.argwhere(bad), int(diff.sum())


# ---------------------------------------------------------------------------------------------- cameras and masks of the tests
def look_at_matrix(eye, target, fov_deg, W, H, znear=0.1, zfar=100.0):
    """A full_proj_transform (float32 [4,4], row-vector convention) built the way Camera._setup builds it: float32
    world-to-view transposed, times the transposed projection matrix, multiplied in float32."""
    eye = np.asarray(eye, dtype=np.float64)
    fwd = np.asarray(target, dtype=np.float64) - eye
    fwd /= np.linalg.norm(fwd)
    up = np.array([0.0, -1.0, 0.0]) if abs(fwd[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    Rc2w = np.stack([right, down, fwd], axis=1)
    Rt = np.eye(4)
    Rt[:3, :3] = Rc2w.T
    Rt[:3, 3] = -Rc2w.T @ eye
    view = np.float32(Rt).T
    tx = np.tan(np.radians(fov_deg) / 2)
    ty = tx * H / W
    P = np.zeros((4, 4), dtype=F)
    P[0, 0], P[1, 1], P[3, 2] = 1 / tx, 1 / ty, 1.0
    P[2, 2], P[2, 3] = zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)
    return (view @ P.T).astype(F)


def disc_mask(W, H, cx, cy, r, dtype=np.uint8):
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (((u + 0.5 - cx) ** 2 + (v + 0.5 - cy) ** 2) <= r * r).astype(dtype)


def ring_scene(n, W, H, distance=3.0, fov_deg=40.0, disc=0.3, elevation=0.3, seed=0):
    """n cameras on a ring looking at the origin and disc masks of the projected sphere of radius `disc` (jittered azimuths, seeded; the
    elevation alternates in sign): ([(M, W, H)], [mask uint8])."""
    rng = np.random.default_rng(seed)
    cams, masks = [], []
    f = (W / 2) / np.tan(np.radians(fov_deg) / 2)
    for a in range(n):
        t = 2 * np.pi * a / n + rng.uniform(-0.1, 0.1)
        eye = distance * np.array([np.cos(t), elevation * (1 if a % 2 == 0 else -1), np.sin(t)])
        cams.append((look_at_matrix(eye, (0, 0, 0), fov_deg, W, H), W, H))
        masks.append(disc_mask(W, H, W / 2, H / 2, f * disc / np.sqrt(np.linalg.norm(eye) ** 2 - disc ** 2)))
    return cams, masks


# ---------------------------------------------------------------------------------------------- mesh helpers
def edge_counts(faces):
    """Number of faces on every undirected edge."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e.sort(axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return counts


def signed_volume(vertices, faces):
    """Sum of the signed tetrahedra (origin, a, b, c): positive for a closed mesh whose normals point outwards."""
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = (v[np.asarray(faces)[:, n]] for n in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
