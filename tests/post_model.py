"""The float32 numpy model of gaustudio_amd.postprocess (csrc/gsr_post.hip): depth -> points, depth -> normals, the fused
epilogue and the masked bilateral filter, every operation in the kernels' order and every intermediate float32.  It is the
DEFINITION of what those calls return: tests/test_gpu_post_edges.py compares points, normals and the epilogue with it bit
for bit, tests/test_post_model.py compares it with the reference's own Camera class (tests/golden/py_post.npz) and with the
independent float64 restatement oracle/post_oracle.py.

  * host setup (setup / invert3 / invert_affine of the source): Python floats are doubles, the operations are written in the
    source's order and the results rounded to float32 -- kinv[9] and c2w[12]; det == 0.0 raises;
  * unproject: xs = ((x / (W-1)) * (W-1)) * z, likewise ys, then p = fma(kinv[2], z, fma(kinv[1], ys, kinv[0] xs)) per row
    (W == 1 or H == 1: 0 / 0 = NaN, in the reference too);
  * normals: zero padding outside the image, validity (z > f32(d_min)) & (z < f32(d_max)) on the five camera-space z (NOT on
    the raw depth: they differ as soon as the last row of K is not (0, 0, 1)), -cross(top - bottom, left - right), the
    norm sqrt(fma(z, z, fma(y, y, x x))) clamped at 1e-12 with fmaxf (a NaN norm becomes 1e-12), correctly rounded divisions,
    world normals = A^-1 n WITHOUT renormalising (the reference does the same), invalid -> (-1, -1, -1);
  * the library is built without contraction: only the fma() written here fuses (scaffold_model.fma, with its caveat: keep
    results out of the float32 subnormal range);
  * bilateral32: the kernel's operations with np.exp (float32) where the kernel has __expf -- the only two operations that
    differ, hence a tolerance and not bit equality for the filtered values; bilateral64 is the same formula in float64 and
    serves the tolerance only.

A NaN produced on the device and one produced by numpy may differ in sign and payload; same_bits() compares NaN positions
and the bytes of everything else.
"""
import numpy as np

from scaffold_model import fma

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- host setup
def invert3(m):
    """gsr_post.hip invert3: 9 float32 (row-major) -> 9 float32, computed in double in the source's order."""
    a, b, c, d, e, f, g, h, i = (float(F32(v)) for v in np.asarray(m).reshape(-1))
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    if det == 0.0:
        raise ValueError("singular matrix")
    r = [(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det,
         (f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det,
         (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det]
    return np.array(r, dtype=np.float64).astype(F32)


def invert_affine(w2c):
    """Rows 0..2 of the inverse of [A t; 0 1] (row-major 4x4, float32): 12 float32."""
    w = np.asarray(w2c, dtype=np.float64).astype(F32).reshape(-1)
    ai = invert3([w[0], w[1], w[2], w[4], w[5], w[6], w[8], w[9], w[10]])
    out = np.zeros(12, F32)
    for r in range(3):
        out[4 * r:4 * r + 3] = ai[3 * r:3 * r + 3]
        t = float(ai[3 * r]) * float(w[3]) + float(ai[3 * r + 1]) * float(w[7]) + float(ai[3 * r + 2]) * float(w[11])
        out[4 * r + 3] = -F32(t)
    return out


def setup(K, E=None):
    """(kinv[9], c2w[12] or None)."""
    return invert3(K), (None if E is None else invert_affine(E))


# -------------------------------------------------------------------------------------------------------- points and normals
def unproject(x, y, z, W, H, kinv):
    """x, y integer arrays, z float32 array (broadcastable) -> (px, py, pz) float32."""
    z = np.asarray(z, dtype=F32)
    with np.errstate(all="ignore"):
        wx, hy = F32(W - 1), F32(H - 1)
        xs = ((np.asarray(x).astype(F32) / wx) * wx) * z
        ys = ((np.asarray(y).astype(F32) / hy) * hy) * z
        return tuple(fma(kinv[3 * r + 2], z, fma(kinv[3 * r + 1], ys, kinv[3 * r] * xs)) for r in range(3))


def _camera_points(depth, kinv):
    depth = np.ascontiguousarray(depth, dtype=F32)
    H, W = depth.shape
    return unproject(np.arange(W)[None, :], np.arange(H)[:, None], depth, W, H, kinv)


def _rotate(c2w, qx, qy, qz):
    with np.errstate(all="ignore"):
        return tuple(fma(c2w[4 * r + 2], qz, fma(c2w[4 * r + 1], qy, c2w[4 * r] * qx)) for r in range(3))


def _points_from(P, c2w):
    if c2w is not None:
        with np.errstate(all="ignore"):
            P = tuple(v + c2w[4 * r + 3] for r, v in enumerate(_rotate(c2w, *P)))
    return np.stack(P, -1).astype(F32)


def points(depth, K, E=None):
    """gsr_depth_to_points: [H,W] -> [H,W,3], world coordinates when E (world-to-camera 4x4) is given."""
    kinv, c2w = setup(K, E)
    return _points_from(_camera_points(depth, kinv), c2w)


def _normals_from(P, c2w, k, d_min, d_max):
    if k < 1:
        raise ValueError("k must be at least 1")
    kd = (k - 1) // 2
    H, W = P[0].shape
    pad = [np.zeros((H + 2 * kd, W + 2 * kd), F32) for _ in range(3)]        # F.pad(..., value=0)
    for c in range(3):
        pad[c][kd:kd + H, kd:kd + W] = P[c]
    lo, hi = F32(d_min), F32(d_max)
    at = lambda dy, dx: [p[kd + dy:kd + dy + H, kd + dx:kd + dx + W] for p in pad]
    pc, pt, pb, pl, pr = at(0, 0), at(-kd, 0), at(kd, 0), at(0, -kd), at(0, kd)
    with np.errstate(all="ignore"):
        valid = np.ones((H, W), bool)
        for p in (pc, pt, pb, pl, pr):
            valid &= (p[2] > lo) & (p[2] < hi)
        v = [pt[c] - pb[c] for c in range(3)]
        h = [pl[c] - pr[c] for c in range(3)]
        n = [-(v[1] * h[2] - v[2] * h[1]), -(v[2] * h[0] - v[0] * h[2]), -(v[0] * h[1] - v[1] * h[0])]
        ln = np.fmax(np.sqrt(fma(n[2], n[2], fma(n[1], n[1], n[0] * n[0]))), F32(1e-12))      # fmaxf: a NaN gives 1e-12
        n = [c / ln for c in n]
        if c2w is not None:
            n = _rotate(c2w, *n)
    out = np.stack(n, -1).astype(F32)
    out[~valid] = F32(-1)
    return out


def normals(depth, K, E=None, k=3, d_min=1e-3, d_max=100000.0):
    """gsr_depth_to_normals: [H,W] -> [H,W,3], (-1, -1, -1) where invalid."""
    kinv, c2w = setup(K, E)
    return _normals_from(_camera_points(depth, kinv), c2w, k, d_min, d_max)


def epilogue(depth, opacity, min_opacity, K, E=None, k=3, d_min=1e-3, d_max=100000.0):
    """gsr_depth_epilogue: (points, normals) of the depth with z = 0 where opacity < min_opacity (a NaN opacity does not mask)."""
    if (k - 1) // 2 > 2:
        raise ValueError("tap distance > 2: the separate entry points")
    depth = np.ascontiguousarray(depth, dtype=F32)
    if opacity is not None:
        with np.errstate(invalid="ignore"):
            depth = np.where(np.asarray(opacity, dtype=F32) < F32(min_opacity), F32(0), depth).astype(F32)
    kinv, c2w = setup(K, E)
    P = _camera_points(depth, kinv)
    return _points_from(P, c2w), _normals_from(P, c2w, k, d_min, d_max)


def same_bits(a, b):
    """Same shape, dtype, NaN positions and -- NaNs aside, whose sign and payload are the producer's -- same bytes."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and np.where(na, F32(0), a).tobytes() == np.where(nb, F32(0), b).tobytes()


# ----------------------------------------------------------------------------------------------------------- bilateral filter
def reflect101(p, n):
    """cv2's BORDER_REFLECT_101 (borderInterpolate), by its own rule: reflect about the first / last sample and repeat until the
    index is inside; a single sample gives 0."""
    p = np.array(p, dtype=np.int64)
    if n == 1:
        return np.zeros_like(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * n - 2 - p, p)
    return p


def _f2ord(f):
    u = np.ascontiguousarray(f, dtype=F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _ord2f(o):
    o = np.uint32(o)
    u = (o & np.uint32(0x7FFFFFFF)) if (o & np.uint32(0x80000000)) else np.uint32(~o)
    return np.array([u], np.uint32).view(F32)[0]


def bilateral_setup(depth, mask, d, sigma_color, sigma_space):
    """What both forms share: (new_mask bool, region bool or None, vmin, vmax, radius, sigma_color, sigma_space).  region =
    new_mask without the NaN depths; None when the input comes back unchanged (no valid pixel)."""
    depth = np.ascontiguousarray(depth, dtype=F32)
    H, W = depth.shape
    if d != 0 and (d < 1 or d % 2 == 0):
        raise ValueError("d must be odd (or 0)")
    sc, ss = F32(sigma_color), F32(sigma_space)
    sc = F32(1) if sc <= 0 else sc
    ss = F32(1) if ss <= 0 else ss
    radius = int(np.rint(ss * F32(1.5))) if d <= 0 else d // 2               # lrintf: to nearest, ties to even
    radius = max(radius, 1)
    r = (2 * radius + 1 if d <= 0 else d) // 2
    valid = np.asarray(mask) != 0
    new_mask = np.ones((H, W), bool)
    for j in range(max(-r, 1 - H), min(r, H - 1) + 1):                       # the in-image part of the window
        for i in range(max(-r, 1 - W), min(r, W - 1) + 1):
            ys, xs = slice(max(0, -j), min(H, H - j)), slice(max(0, -i), min(W, W - i))
            yd, xd = slice(max(0, j), min(H, H + j)), slice(max(0, i), min(W, W + i))
            new_mask[ys, xs] &= valid[yd, xd]
    region = new_mask & ~np.isnan(depth)
    if not region.any():
        return new_mask, None, None, None, radius, sc, ss
    o = _f2ord(depth)[region]                                                # atomicMin / atomicMax on the ordered words
    return new_mask, region, _ord2f(o.min()), _ord2f(o.max()), radius, sc, ss


def _bilateral(depth, mask, d, sigma_color, sigma_space, T):
    depth = np.ascontiguousarray(depth, dtype=F32)
    H, W = depth.shape
    new_mask, region, vmin, vmax, radius, sc, ss = bilateral_setup(depth, mask, d, sigma_color, sigma_space)
    info = dict(taps=0, max_arg=0.0, range=0.0, radius=radius)
    out = depth.astype(T)
    if region is None:
        return out, new_mask, info
    rng = F32(vmax - vmin)                                                   # the kernel's float32 range, in both forms
    if not rng > 0:
        return out, new_mask, info
    info["range"] = float(rng)
    if T is F32:
        space_coeff, color_coeff = F32(-0.5) / (ss * ss), F32(-0.5) / (sc * sc)
    else:
        space_coeff, color_coeff = -0.5 / (float(ss) * float(ss)), -0.5 / (float(sc) * float(sc))
    vmin_t, rng_t = T(vmin), T(rng)
    with np.errstate(all="ignore"):
        norm = np.where(region, (depth.astype(T) - vmin_t) / rng_t, T(0)).astype(T)
    pad = norm[np.ix_(reflect101(np.arange(-radius, H + radius), H), reflect101(np.arange(-radius, W + radius), W))]
    num, den = np.zeros((H, W), T), np.zeros((H, W), T)
    floor = 2.0 ** -24
    for j in range(-radius, radius + 1):                                     # the kernel's order: j outer, i inner
        for i in range(-radius, radius + 1):
            if i * i + j * j > radius * radius:                              # circular window
                continue
            info["taps"] += 1
            v = pad[radius + j:radius + j + H, radius + i:radius + i + W]
            dv = v - norm
            a_s = np.full((1,), T(i * i + j * j) * space_coeff, T)
            a_c = dv * dv * color_coeff
            w = np.exp(a_s) * np.exp(a_c)
            num = num + v * w
            den = den + w
            if T is not F32:
                big = region & (w >= floor)
                if big.any():
                    info["max_arg"] = max(info["max_arg"], float(-a_s[0]), float((-a_c[big]).max()))
    with np.errstate(all="ignore"):
        filt = (num / den) * rng_t + vmin_t
    out[region] = filt[region]
    return out, new_mask, info


def bilateral32(depth, mask, d=3, sigma_color=75.0, sigma_space=75.0):
    """gsr_masked_bilateral in float32 with np.exp for __expf: (filtered float32 [H,W], new_mask bool [H,W])."""
    out, new_mask, _ = _bilateral(depth, mask, d, sigma_color, sigma_space, F32)
    return out, new_mask


def bilateral64(depth, mask, d=3, sigma_color=75.0, sigma_space=75.0):
    """The same formula in float64 (same erosion, same float32 min / max / range): (filtered float64, new_mask, info) with
    info = dict(taps, max_arg, range, radius): the taps of the circular window, and the largest |argument| of either exp
    over the taps whose weight is at least 2^-24 of the centre's (which is 1)."""
    return _bilateral(depth, mask, d, sigma_color, sigma_space, np.float64)


def bilateral_bound(depth, mask, d, sigma_color, sigma_space):
    """(ref64, new_mask, E, bound, info): the tolerance of tests/test_gpu_post_edges.py for |hip - ref64|, see there."""
    ref64, new_mask, info = bilateral64(depth, mask, d, sigma_color, sigma_space)
    out32, _ = bilateral32(depth, mask, d, sigma_color, sigma_space)
    with np.errstate(invalid="ignore"):
        diff = np.abs(out32.astype(np.float64) - ref64)
    E = float(np.nanmax(diff)) if diff.size else 0.0
    delta = 2.0 ** -22 + 2.0 ** -24 * np.log2(np.e) * info["max_arg"]
    bound = 4 * E + info["range"] * (2 * delta + info["taps"] * 2.0 ** -23)
    return ref64, new_mask, E, bound, info
