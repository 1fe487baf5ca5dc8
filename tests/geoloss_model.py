"""The definition of gaustudio_amd.surfel_losses (csrc/gsr_geoloss.hip): a float32 numpy model that
reproduces the kernels TO THE BIT -- the blended depth, the rays, the stencil, the ten maps, the float64 partial tree of each
workgroup, the final sum, loss / normal_loss / dist_loss and all seven gradient planes.

No expression is fused: every product, sum, divide and square root below rounds once, in the order written, which is the
order of the kernels (the library is built without contraction and with correctly rounded divide and sqrt, as numpy's are).
The partial sums are those of loss_model (one 16 x 64 tile per workgroup, the fixed 256-leaf float64 tree).

Which branch at |c| < eps: F.normalize's.  n = c / max(|c|, eps); where |c| >= eps (`through`) the gradient passes through the
norm, dL/dc = (g - n <n, g>) / |c|; where |c| < eps the divisor is the constant eps and dL/dc = g / eps.  A depth gradient of
0 there needs c = 0 through a = b = 0 (all four neighbours at one depth 0), not |c| < eps alone.
"""
import numpy as np

from loss_model import F32, F64, TH, TW, final_sum, same_bits, tile_partials  # noqa: F401  (same_bits: for the tests)

EPS = F32(1e-12)
MAP_PLANES = dict(rendered_depth=slice(0, 1), rendered_median_depth=slice(1, 2), surf_depth=slice(2, 3), surf_normal=slice(3, 6),
                  rendered_normal=slice(6, 9), normal_error=9)


def _cam(intrinsics):
    return tuple(F32(v) for v in intrinsics)


def _finite_or_zero(v):
    return np.where(np.isfinite(v), v, F32(0)).astype(F32)


def blended_depth(a, depth_ratio):
    """(d_exp, d_med, d) [H,W]: nan_to_num(a0 / a1), nan_to_num(a5), (1 - rho) d_exp + rho d_med."""
    rho = F32(depth_ratio)
    wexp = F32(1) - rho
    with np.errstate(all="ignore"):
        de, dm = _finite_or_zero(a[0] / a[1]), _finite_or_zero(a[5])
        return de, dm, wexp * de + rho * dm


def rays(H, W, intrinsics):
    fx, fy, cx, cy = _cam(intrinsics)
    return (np.arange(W, dtype=F32) - cx) / fx, (np.arange(H, dtype=F32) - cy) / fy


def stencil(d, rxs, rys):
    """The stencils of the interior pixels, [H-2, W-2] each: a = p(x, y+1) - p(x, y-1), b = p(x+1, y) - p(x-1, y),
    n = a x b / max(|a x b|, eps), den = that maximum, through = the norm is not clamped."""
    dU, dD, dL, dR = d[:-2, 1:-1], d[2:, 1:-1], d[1:-1, :-2], d[1:-1, 2:]
    rx, rxl, rxr = rxs[None, 1:-1], rxs[None, :-2], rxs[None, 2:]
    ry, ryu, ryd = rys[1:-1, None], rys[:-2, None], rys[2:, None]
    with np.errstate(all="ignore"):
        ax, ay, az = dD * rx - dU * rx, dD * ryd - dU * ryu, dD - dU
        bx, by, bz = dR * rxr - dL * rxl, dR * ry - dL * ry, dR - dL
        cx, cy, cz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
        nrm = np.sqrt((cx * cx + cy * cy) + cz * cz)
        small = nrm < EPS
        den = np.where(small, EPS, nrm).astype(F32)
        n = (cx / den, cy / den, cz / den)
    return dict(a=(ax, ay, az), b=(bx, by, bz), c=(cx, cy, cz), nrm=nrm, den=den, n=n, through=~small)


def _full(v, H, W):
    """An interior quantity on the whole image, +0 on the border."""
    out = np.zeros((H, W), dtype=F32)
    if H >= 3 and W >= 3:
        out[1:-1, 1:-1] = v
    return out


def _interior(H, W):
    return H >= 3 and W >= 3


def surface_normal(a, d, intrinsics):
    """n a1 [3,H,W]: 0 on the border."""
    H, W = d.shape
    if not _interior(H, W):
        return np.zeros((3, H, W), dtype=F32), None
    st = stencil(d, *rays(H, W, intrinsics))
    with np.errstate(all="ignore"):
        return np.stack([_full(st["n"][j] * a[1][1:-1, 1:-1], H, W) for j in range(3)]), st


def forward(allmap, intrinsics, lambda_normal=0.05, lambda_dist=0.0, depth_ratio=0.0, viewmatrix=None):
    """allmap [7,H,W] float32.  Returns a dict: loss, normal_loss, dist_loss (float32 scalars), the maps of surfel_maps by name
    and `maps` [10,H,W] as the kernel writes them (both normals turned by viewmatrix when it is given)."""
    a = np.ascontiguousarray(allmap, dtype=F32)
    H, W = a.shape[1:]
    de, dm, d = blended_depth(a, depth_ratio)
    sn, _ = surface_normal(a, d, intrinsics)
    with np.errstate(all="ignore"):
        e = F32(1) - ((a[2] * sn[0] + a[3] * sn[1]) + a[4] * sn[2])
        n = F64(H) * F64(W)
        nl = F64(F32(lambda_normal)) * (final_sum(tile_partials(e[None])) / n)
        dl = F64(F32(lambda_dist)) * (final_sum(tile_partials(a[6][None])) / n)
        rn = a[2:5]
        if viewmatrix is not None:
            V = np.asarray(viewmatrix, dtype=F32).reshape(4, 4)
            turn = lambda v: np.stack([(v[0] * V[j, 0] + v[1] * V[j, 1]) + v[2] * V[j, 2] for j in range(3)])
            sn_out, rn_out = turn(sn), turn(rn)
        else:
            sn_out, rn_out = sn, rn
        maps = np.concatenate([de[None], dm[None], d[None], sn_out, rn_out, e[None]]).astype(F32)
        out = dict(loss=F32(nl + dl), normal_loss=F32(nl), dist_loss=F32(dl), maps=maps)
    out.update({k: maps[s] for k, s in MAP_PLANES.items()})
    return out


def backward(allmap, intrinsics, lambda_normal=0.05, lambda_dist=0.0, depth_ratio=0.0, grad_loss=1.0):
    """d(grad_loss * loss) / d allmap [7,H,W]."""
    a = np.ascontiguousarray(allmap, dtype=F32)
    H, W = a.shape[1:]
    rho = F32(depth_ratio)
    wexp = F32(1) - rho
    n = F64(H) * F64(W)
    wn, wd = F32(F64(F32(lambda_normal)) / n), F32(F64(F32(lambda_dist)) / n)
    gup = F32(grad_loss)
    g = np.zeros((7, H, W), dtype=F32)
    with np.errstate(all="ignore"):
        wng = gup * wn
        de, dm, d = blended_depth(a, depth_ratio)
        sn, st = surface_normal(a, d, intrinsics)
        for j in range(3):
            g[2 + j] = -(wng * sn[j])
        g[6] = gup * wd
        v = [np.zeros((H, W), dtype=F32)] * 3
        if st is not None:
            al, N = a[1][1:-1, 1:-1], [a[2 + j][1:-1, 1:-1] for j in range(3)]
            nx, ny, nz = st["n"]
            w = wng * al
            g0, g1, g2 = -(w * N[0]), -(w * N[1]), -(w * N[2])
            pr = np.where(st["through"], (nx * g0 + ny * g1) + nz * g2, F32(0)).astype(F32)
            den = st["den"]
            q0, q1, q2 = (g0 - nx * pr) / den, (g1 - ny * pr) / den, (g2 - nz * pr) / den
            (ax, ay, az), (bx, by, bz) = st["a"], st["b"]
            ga = (by * q2 - bz * q1, bz * q0 - bx * q2, bx * q1 - by * q0)
            gb = (q1 * az - q2 * ay, q2 * ax - q0 * az, q0 * ay - q1 * ax)
            # the gather: pixel q is the lower point of the centre above it, the upper point of the centre below, the right
            # point of the centre to its left, the left point of the centre to its right; no centre outside the interior
            v = []
            for j in range(3):
                A, B = np.pad(_full(ga[j], H, W), 1), np.pad(_full(gb[j], H, W), 1)
                v.append((A[:-2, 1:-1] - A[2:, 1:-1]) + (B[1:-1, :-2] - B[1:-1, 2:]))
        rxs, rys = rays(H, W, intrinsics)
        gd = (v[0] * rxs[None, :] + v[1] * rys[:, None]) + v[2]
        ge = wexp * gd
        q = a[0] / a[1]
        fin = np.isfinite(q)
        g[0] = np.where(fin, ge / a[1], F32(0))
        g[1] = np.where(fin, -(ge * q) / a[1], F32(0))
        g[5] = np.where(np.isfinite(a[5]), rho * gd, F32(0))
    return g


def loss_and_grad(allmap, intrinsics, lambda_normal=0.05, lambda_dist=0.0, depth_ratio=0.0, grad_loss=1.0, viewmatrix=None):
    f = forward(allmap, intrinsics, lambda_normal, lambda_dist, depth_ratio, viewmatrix)
    f["grad"] = backward(allmap, intrinsics, lambda_normal, lambda_dist, depth_ratio, grad_loss)
    return f
