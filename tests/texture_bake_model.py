"""The float32 numpy model of the vertex-colour bake (csrc/gsr_mesh_bake.hip bake_select / bake_sample),
operation for operation: every intermediate is float32, every sum is written in the kernel's order, nothing is fused.  The GPU
tests compare with it exactly; tests/test_texture_bake_model.py checks it against torch's grid_sample, a float64 restatement of
the script's camera and closed forms.  Visibility comes from tests/mesh_raster_model.py (the model of s15)."""
import numpy as np

import mesh_raster_model as rm

F32 = np.float32
COS_LIMIT = F32(-0.05)


def _m(a, shape):
    return np.asarray(a, dtype=np.float64).reshape(shape).astype(F32)


def norm3(u):
    return np.sqrt((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2])


def view_axis(extrinsics):
    """The third row of the world-to-camera rotation, normalised in float32."""
    E = _m(extrinsics, (4, 4))
    d = E[2, :3]
    return d / norm3(d)


def select(verts, faces, visible, extrinsics):
    """(cos [F] float32, NaN where not visible; selected [F] bool)."""
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vis = np.asarray(visible).astype(bool)
    d = view_axis(extrinsics)
    cos = np.full(f.shape[0], np.nan, dtype=F32)
    with np.errstate(all="ignore"):
        p0, p1, p2 = v[f[vis, 0]], v[f[vis, 1]], v[f[vis, 2]]
        n = rm.cross(p1 - p0, p2 - p0)
        ln = norm3(n)
        cos[vis] = ((n[:, 0] / ln) * d[0] + (n[:, 1] / ln) * d[1]) + (n[:, 2] / ln) * d[2]
        sel = cos < COS_LIMIT
    return cos, sel


def stamped(faces, selected, num_verts):
    """bool [V]: the vertices of the selected faces (torch.unique(faces.flatten()) as a mask)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    m = np.zeros(num_verts, dtype=bool)
    m[f[np.asarray(selected, dtype=bool)].reshape(-1)] = True
    return m


def screen_points(verts, intrinsics, extrinsics):
    """(x, y) of the reference's flipped screen camera and (u, v) of the OpenCV pixel, float32 [N] each."""
    K = _m(intrinsics, (3, 3))
    pc = rm.camera_space(verts, extrinsics, F32)
    with np.errstate(all="ignore"):
        x = (K[0, 0] * (-pc[:, 0])) / pc[:, 2] + K[0, 2]
        y = (K[1, 1] * (-pc[:, 1])) / pc[:, 2] + K[1, 2]
        u = (K[0, 0] * pc[:, 0]) / pc[:, 2] + K[0, 2]
        w = (K[1, 1] * pc[:, 1]) / pc[:, 2] + K[1, 2]
    return x, y, u, w


def coords_reference(x, y, W, H):
    """texture_mesh.py:134-137 and grid_sample's unnormalisation: (ix, iy, valid)."""
    x, y = np.asarray(x, dtype=F32), np.asarray(y, dtype=F32)
    Wf, Hf = F32(W), F32(H)
    with np.errstate(all="ignore"):
        gx = F32(2) * (x / (Wf - F32(1))) - F32(1)
        gy = F32(2) * (y / (Hf - F32(1))) - F32(1)
        valid = (gx >= -1) & (gx <= 1) & (gy >= -1) & (gy <= 1)
        ix = ((gx + F32(1)) * Wf - F32(1)) / F32(2)
        iy = ((gy + F32(1)) * Hf - F32(1)) / F32(2)
    return ix, iy, valid


def coords_exact(u, w, W, H):
    u, w = np.asarray(u, dtype=F32), np.asarray(w, dtype=F32)
    with np.errstate(all="ignore"):
        valid = (u >= 0) & (u <= F32(W)) & (w >= 0) & (w <= F32(H))
    return u - F32(0.5), w - F32(0.5), valid


def bilinear(image, ix, iy, flip):
    """grid_sample's four taps (nw, ne, sw, se) at coordinates clipped to the image; flip reads I[H - 1 - r, W - 1 - c]."""
    img = np.asarray(image, dtype=F32)
    H, W = img.shape[:2]
    ix = np.minimum(np.maximum(np.asarray(ix, dtype=F32), F32(0)), F32(W - 1))
    iy = np.minimum(np.maximum(np.asarray(iy, dtype=F32), F32(0)), F32(H - 1))
    fx0, fy0 = np.floor(ix), np.floor(iy)
    fx1, fy1 = fx0 + F32(1), fy0 + F32(1)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    taps = ((x0, y0, (fx1 - ix) * (fy1 - iy)), (x0 + 1, y0, (ix - fx0) * (fy1 - iy)),
            (x0, y0 + 1, (fx1 - ix) * (iy - fy0)), (x0 + 1, y0 + 1, (ix - fx0) * (iy - fy0)))
    acc = np.zeros(ix.shape + (3,), dtype=F32)
    for tx, ty, wt in taps:
        ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        r = np.clip(H - 1 - ty if flip else ty, 0, H - 1)
        c = np.clip(W - 1 - tx if flip else tx, 0, W - 1)
        with np.errstate(all="ignore"):
            term = img[r, c] * wt[..., None]
            acc = np.where(ok[..., None], acc + term, acc)
    return acc


def clamp01(c):
    return np.where(c < 0, F32(0), np.where(c > 1, F32(1), c)).astype(F32)      # NaN stays NaN


def sample_points(image, x, y, u, w, sampling):
    """(colour [N,3] float32, valid [N]) for screen positions (x, y) / pixels (u, w)."""
    H, W = np.asarray(image).shape[:2]
    if sampling == "exact":
        ix, iy, valid = coords_exact(u, w, W, H)
    else:
        ix, iy, valid = coords_reference(x, y, W, H)
    ix, iy = np.where(valid, ix, F32(0)), np.where(valid, iy, F32(0))
    return clamp01(bilinear(image, ix, iy, flip=sampling != "exact")), valid


def add_view(colors, baked_by, seq, verts, faces, visible, image, intrinsics, extrinsics, sampling="reference"):
    """One view, in place.  Returns (cos, selected, baked mask)."""
    cos, sel = select(verts, faces, visible, extrinsics)
    st = stamped(faces, sel, colors.shape[0])
    x, y, u, w = screen_points(verts, intrinsics, extrinsics)
    col, valid = sample_points(image, x, y, u, w, sampling)
    m = st & valid
    colors[m] = col[m]
    baked_by[m] = seq
    return cos, sel, m


def visible_faces(verts, faces, intrinsics, extrinsics, H, W):
    p2f, _, _ = rm.rasterize(verts, faces, intrinsics, extrinsics, H, W)
    return rm.visible_faces(p2f, np.asarray(faces).reshape(-1, 3).shape[0])


def bake(verts, faces, views, sampling="reference", visibles=None):
    """views: [(image [H,W,3] float32, K, E)].  (colors [V,3] float32, baked_by [V] int32, [cos per view])."""
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    colors = np.zeros((v.shape[0], 3), dtype=F32)
    baked_by = np.full(v.shape[0], -1, dtype=np.int32)
    coss = []
    for seq, (image, K, E) in enumerate(views):
        H, W = np.asarray(image).shape[:2]
        vis = visibles[seq] if visibles is not None else visible_faces(v, faces, K, E, H, W)
        cos, _, _ = add_view(colors, baked_by, seq, v, faces, vis, image, K, E, sampling)
        coss.append(cos)
    return colors, baked_by, coss


# ------------------------------------------------------------------------------------------------ cameras and images
def intrinsics(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float64)


def gradient_image(H, W, a=0.1, b=0.05, c=0.03, channels=(1.0, 0.5, 0.25)):
    """I[i, j, ch] = (a + b j + c i) * channels[ch], float32."""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = a + b * j + c * i
    return np.stack([base * s for s in channels], axis=-1).astype(F32)


def random_image(H, W, seed):
    return np.random.default_rng(seed).uniform(0, 1, (H, W, 3)).astype(F32)
