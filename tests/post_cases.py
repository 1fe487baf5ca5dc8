"""Inputs shared by tests/test_post_model.py (CPU: the float32 model against the float64 restatement) and
tests/test_gpu_post_edges.py (GPU: the kernels against the model): image sizes around the 64x8 / 64x4 blocks, cameras whose
last intrinsic row is not (0, 0, 1) or whose extrinsic is not rigid, depth maps with zeros, negatives, non-finite values and
values exactly on the validity bounds, and the masked-bilateral cases.  numpy only."""
import numpy as np

F32 = np.float32

# [H, W]: tile and halo tails of the 64x8 (normals) and 64x4 (points) blocks, and images smaller than one halo
SIZES = [(1, 5), (5, 1), (2, 2), (7, 63), (8, 64), (9, 65), (17, 129), (37, 200)]
KS = [1, 2, 3, 4, 5, 7, 11]            # tap distances 0, 0, 1, 1, 2 (tiled kernel) and 3, 5 (per-pixel kernel)
BOUNDS = [(1e-3, 100000.0), (0.5, 2.5)]
CAMERAS = ("pinhole", "skew", "rigid", "shear")


def far_k(H, W):
    """Every tap outside the image: everything is invalid."""
    return 2 * max(H, W) + 1


def camera(name, H, W):
    """(K [3,3] float32, E [4,4] float32 or None)."""
    f = 0.9 * max(W, 2)
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], F32)
    E = None
    a = 0.4
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    if name == "skew":       # skew, K[2][2] = 2, K[2][0] != 0: camera z is about depth / 2, and depends on the column
        K = np.array([[f, 0.3, W / 2], [0, 0.8 * f, H / 2], [0.002, 0, 2]], F32)
    elif name in ("rigid", "shear"):
        E = np.eye(4)
        E[:3, :3] = R if name == "rigid" else 2.0 * R @ np.array([[1, 0.3, 0], [0, 1, 0], [0, 0.2, 1.0]])
        E[:3, 3] = [0.3, -0.2, 1.0]
        E = E.astype(F32)
    return K, E


def bound_values():
    """The eight depths on and next to the bounds of BOUNDS: d_min, the float32 above it, d_max, the float32 below it."""
    out = []
    for lo, hi in BOUNDS:
        out += [F32(lo), np.nextafter(F32(lo), F32(np.inf)), F32(hi), np.nextafter(F32(hi), F32(-np.inf))]
    return np.array(out, F32)


def depth_map(H, W, name, boundary=True):
    """Depths in [2, 3] -- on both sides of d_max = 2.5 -- with 10 % zeros, a few negatives, NaN, +-inf and one 1e30 pixel; for
    the skew camera a third of the pixels in [0.6, 0.9] and in [2.6, 4.0], where raw depth and camera z (about depth / 2) lie on
    opposite sides of d_min = 0.5 and d_max = 2.5; with `boundary`, row H // 2 starts with bound_values() (cameras with the
    last intrinsic row (0, 0, 1) have camera z == depth exactly)."""
    rng = np.random.default_rng(1000 * H + W)
    d = (2.0 + rng.random((H, W))).astype(F32)
    if name == "skew":
        u = rng.random((H, W))
        d = np.where(u < 1 / 6, 0.6 + 0.3 * rng.random((H, W)), np.where(u < 1 / 3, 2.6 + 1.4 * rng.random((H, W)), d)).astype(F32)
    flat = d.reshape(-1)
    order = rng.permutation(H * W)
    n = H * W
    special = [np.nan, np.inf, -np.inf, 1e30, -1.5, -0.0, -2.25] if n >= 16 else [np.nan, -1.5][:n // 3]
    flat[order[:len(special)]] = np.array(special, F32)
    nz = n // 10
    flat[order[len(special):len(special) + nz]] = 0.0
    if boundary:
        bv = bound_values()[:W]
        d[H // 2, :len(bv)] = bv
    return d


def opacity_map(H, W, min_opacity=0.5):
    """Uniform opacities with pixels at exactly min_opacity (not masked), its float32 neighbours and NaN (not masked)."""
    rng = np.random.default_rng(77 * H + W)
    o = rng.random((H, W)).astype(F32)
    m = F32(min_opacity)
    special = np.array([m, np.nextafter(m, F32(0)), np.nextafter(m, F32(1)), np.nan], F32)
    flat = o.reshape(-1)
    idx = rng.permutation(H * W)[:min(4, H * W)]
    flat[idx] = special[:len(idx)]
    return o


# ---------------------------------------------------------------------------------------------------------- bilateral filter
def _depth(H, W, seed):
    rng = np.random.default_rng(seed)
    return (2.0 + 3.0 * rng.random((H, W)) + 0.3 * np.sin(np.arange(W) / 5.0)[None, :]).astype(F32)


def bilateral_cases():
    """[(id, depth, mask bool, d, sigma_color, sigma_space)]."""
    cases = []
    # the radius reaches past the image: BORDER_REFLECT_101 crosses it more than once
    for H, W, d in [(9, 2, 5), (3, 3, 7), (6, 1, 3), (1, 6, 3), (2, 2, 7), (70, 4, 9), (5, 20, 11)]:
        m = np.ones((H, W), bool)
        if H * W > 36:
            m[0, 0] = False               # erodes one corner band; the smaller images would lose every pixel
        cases.append((f"narrow-{H}x{W}-d{d}", _depth(H, W, 31 * H + W), m, d, 0.2, 3.0))
    # d = 0: the radius comes from sigma_space (1, 2 -- lrint(1.5) ties to even --, 3), the erosion window is 2 radius + 1
    for ss in (0.5, 1.0, 2.1):
        m = np.ones((33, 17), bool); m[4, 5] = m[30, 16] = False
        cases.append((f"d0-ss{ss}", _depth(33, 17, 5), m, 0, 0.2, ss))
    cases.append(("d0-default-sigma", _depth(40, 30, 6), np.ones((40, 30), bool), 0, 75.0, 75.0))      # radius lrint(112.5) = 112
    # the extremes in the first lane of the first wave, in the last lane of the tail wave, both in a row's 2-pixel tail
    for sign in ("pos", "neg", "mixed"):
        for place, (pmin, pmax) in dict(last_first=((12, 129), (0, 0)), first_last=((0, 0), (12, 129)),
                                        row_tail=((5, 128), (5, 129))).items():
            d = _depth(13, 130, 9)
            d[pmin], d[pmax] = 1.0, 6.0
            if sign == "neg":
                d = -d; d[pmin], d[pmax] = -1.0, -6.0        # pmin now holds the maximum
            elif sign == "mixed":
                d = d - F32(3.5); d[3, 7] = -0.0; d[3, 8] = 0.0
            cases.append((f"extremes-{sign}-{place}", d.astype(F32), np.ones((13, 130), bool), 3, 0.3, 1.0))
    # a NaN inside the eroded mask
    d = _depth(20, 30, 11); d[10, 12] = np.nan
    m = np.ones((20, 30), bool); m[2, 3] = False
    cases.append(("nan-inside", d, m, 3, 0.2, 1.0))
    # degenerate masks: one survivor; two survivors of equal depth; all valid; all invalid
    m = np.zeros((7, 8), bool); m[2:5, 2:5] = True
    cases.append(("one-survivor", _depth(7, 8, 12), m, 3, 0.2, 1.0))
    m = np.zeros((7, 8), bool); m[2:5, 2:6] = True
    d = _depth(7, 8, 12); d[3, 3] = d[3, 4] = 2.75
    cases.append(("two-equal-survivors", d, m, 3, 0.2, 1.0))
    cases.append(("all-valid", _depth(17, 33, 13), np.ones((17, 33), bool), 3, 0.2, 1.0))
    cases.append(("all-invalid", _depth(17, 33, 13), np.zeros((17, 33), bool), 3, 0.2, 1.0))
    # colour sigma 0.05: weights spanning many decades
    rng = np.random.default_rng(14)
    cases.append(("sigma-color-0.05", _depth(61, 97, 14), rng.random((61, 97)) > 0.03, 5, 0.05, 1.5))
    return cases
