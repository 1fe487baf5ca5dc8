"""The definition of gaustudio_amd.losses (csrc/gsr_loss.hip), twice.

1. A float32 numpy model that reproduces the two kernels TO THE BIT: every intermediate, the three saved maps, ssim_map, the
   float64 partial tree of each workgroup, the final sum, loss / l1 / ssim and the gradient.  Same tap order and fma placement
   (scaffold_model.fma is the tie-safe fmaf), same tile-partial order, numpy's correctly rounded float32 divide.  No
   transcendental function: the window is the table below.
2. `reference(...)`: the published formula restated with F.conv2d and autograd on the CPU, in float64 (the truth) or in float32
   (what everyone trains with today: the yardstick of the model's error in tests/test_loss_model.py).
"""
import numpy as np

from scaffold_model import fma

F32 = np.float32
F64 = np.float64
TH, TW = 16, 64          # the workgroup's tile: losses.TILE_H, losses.TILE_W
RAD = 5
# float32(exp(-(i - 5)^2 / (2 1.5^2)) / sum), evaluated in float64 and rounded once
WINDOW = np.array([float.fromhex(h) for h in (
    "0x1.0d956cp-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c4p-3", "0x1.10656p-2",
    "0x1.b43c4p-3", "0x1.bff0fep-4", "0x1.26eb18p-5", "0x1.f1fe02p-8", "0x1.0d956cp-10")], dtype=F32)
C1 = F32(0.01) * F32(0.01)
C2 = F32(0.03) * F32(0.03)


def conv_axis(v, axis):
    """11 taps along `axis` under zero padding: g[0] v[0] first, then one fma per tap in ascending tap order."""
    v = np.asarray(v, dtype=F32)
    pad = [(0, 0)] * v.ndim
    pad[axis] = (RAD, RAD)
    p = np.pad(v, pad)
    n = v.shape[axis]
    tap = lambda k: np.take(p, np.arange(k, k + n), axis=axis)
    with np.errstate(all="ignore"):
        acc = WINDOW[0] * tap(0)
        for k in range(1, 11):
            acc = fma(WINDOW[k], tap(k), acc)
    return acc


def conv(v):
    """The separable window: rows first (along W), then columns (along H)."""
    return conv_axis(conv_axis(v, -1), -2)


def _tree(a):
    """The fixed tree over the last axis of 256 float64 leaves: leaf t adds leaf t + s for s = 128, 64, ..., 1."""
    a = a.copy()
    s = 128
    while s > 0:
        a[..., :s] = a[..., :s] + a[..., s:2 * s]
        s >>= 1
    return a[..., 0]


def tile_partials(v):
    """[P,H,W] float32 -> float64 partials, one per workgroup in launch order (plane, tile row, tile column).  A lane owns
    column cx and rows 4 rg .. 4 rg + 3 of the tile, adds its four values in row order (pixels outside the image count 0.0)
    and is leaf cx + 64 rg of the tree."""
    P, H, W = v.shape
    ty, tx = -(-H // TH), -(-W // TW)
    full = np.zeros((P, ty * TH, tx * TW), dtype=F64)
    full[:, :H, :W] = v
    t = full.reshape(P, ty, 4, 4, tx, TW).transpose(0, 1, 4, 2, 3, 5)      # [P, ty, tx, rg, i, cx]
    with np.errstate(all="ignore"):
        lane = np.zeros(t.shape[:4] + (TW,), dtype=F64)
        for i in range(4):
            lane = lane + t[:, :, :, :, i, :]
        return _tree(lane.reshape(P, ty, tx, 256)).reshape(-1)


def final_sum(partials):
    """The one-workgroup kernel: lane t adds partials t, t + 256, ... in ascending order, then the tree."""
    n = len(partials)
    rows = -(-n // 256)
    p = np.zeros(rows * 256, dtype=F64)
    p[:n] = partials
    with np.errstate(all="ignore"):
        acc = np.zeros(256, dtype=F64)
        for r in p.reshape(rows, 256):
            acc = acc + r
        return _tree(acc)


def sign(d):
    """torch.sign: 0 at 0 (and for a NaN)."""
    return (0 < d).astype(F32) - (d < 0).astype(F32)


def forward(image, target, lambda_dssim=0.2):
    """image / target [..., H, W] float32.  Returns a dict: loss, l1, ssim (float32 scalars), ssim_map and maps [3, ...]
    (what the kernel saves for the backward) in the input's shape."""
    x = np.ascontiguousarray(image, dtype=F32)
    y = np.ascontiguousarray(target, dtype=F32)
    shape = x.shape
    H, W = shape[-2:]
    x = x.reshape(-1, H, W)
    y = y.reshape(-1, H, W)
    with np.errstate(all="ignore"):
        mu1, mu2 = conv(x), conv(y)
        e11, e22, e12 = conv(x * x), conv(y * y), conv(x * y)
        mu1sq, mu2sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
        s1, s2, s12 = e11 - mu1sq, e22 - mu2sq, e12 - mu12
        a1, a2 = F32(2) * mu12 + C1, F32(2) * s12 + C2
        b1, b2 = (mu1sq + mu2sq) + C1, (s1 + s2) + C2
        den = b1 * b2
        S = (a1 * a2) / den
        dD = (F32(2) * a1) / den
        dB = -(S / b2)
        dA = ((F32(2) * a2) / den) * (mu2 - mu1 * (a1 / b1))
        m0 = fma(-mu2, dD, fma(-(F32(2) * mu1), dB, dA))
        n = F64(x.size)
        ssim = final_sum(tile_partials(S)) / n
        l1 = final_sum(tile_partials(np.abs(x - y))) / n
        ld = F64(F32(lambda_dssim))
        loss = (F64(1) - ld) * l1 + ld * (F64(1) - ssim)
    return dict(loss=F32(loss), l1=F32(l1), ssim=F32(ssim), ssim_map=S.reshape(shape),
                maps=np.stack([m0, dB, dD]).reshape((3,) + shape))


def backward(image, target, maps, lambda_dssim=0.2, grad_loss=1.0):
    """d(grad_loss * loss) / d image from the forward's maps."""
    x = np.ascontiguousarray(image, dtype=F32)
    y = np.ascontiguousarray(target, dtype=F32)
    shape = x.shape
    H, W = shape[-2:]
    x = x.reshape(-1, H, W)
    y = y.reshape(-1, H, W)
    m = np.asarray(maps, dtype=F32).reshape(3, -1, H, W)
    ld, n = F64(F32(lambda_dssim)), F64(x.size)
    w_l1, w_ssim = F32((F64(1) - ld) / n), F32(ld / n)
    with np.errstate(all="ignore"):
        c0, c1, c2 = conv(m[0]), conv(m[1]), conv(m[2])
        dssim = fma(y, c2, fma(F32(2) * x, c1, c0))
        g = F32(grad_loss) * fma(w_l1, sign(x - y), -(w_ssim * dssim))
    return g.reshape(shape)


def loss_and_grad(image, target, lambda_dssim=0.2, grad_loss=1.0):
    f = forward(image, target, lambda_dssim)
    f["grad"] = backward(image, target, f["maps"], lambda_dssim, grad_loss)
    return f


def same_bits(a, b):
    """NaN in the same places, the same bytes everywhere else."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(np.where(na, F32(0), a).view(np.uint32), np.where(nb, F32(0), b).view(np.uint32)))


def reference(image, target, lambda_dssim=0.2, dtype="float64"):
    """The published 3DGS loss with F.conv2d (zero padding 5, one group per plane) and autograd, on the CPU.  The window is
    the float32 table, its outer product formed in `dtype`."""
    import torch
    import torch.nn.functional as F
    dt = getattr(torch, dtype)
    x0 = np.ascontiguousarray(image, dtype=F32)
    shape = x0.shape
    H, W = shape[-2:]
    x = torch.from_numpy(x0.reshape(1, -1, H, W)).to(dt).requires_grad_(True)
    y = torch.from_numpy(np.ascontiguousarray(target, dtype=F32).reshape(1, -1, H, W)).to(dt)
    P = x.shape[1]
    g = torch.from_numpy(WINDOW).to(dt)
    w = (g[:, None] * g[None, :]).expand(P, 1, 11, 11).contiguous()
    cv = lambda v: F.conv2d(v, w, padding=RAD, groups=P)
    mu1, mu2 = cv(x), cv(y)
    mu1sq, mu2sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = cv(x * x) - mu1sq, cv(y * y) - mu2sq, cv(x * y) - mu12
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    smap = ((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu1sq + mu2sq + c1) * (s1 + s2 + c2))
    ssim = smap.mean()
    l1 = (x - y).abs().mean()
    loss = (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - ssim)
    loss.backward()
    return dict(loss=loss.item(), l1=l1.item(), ssim=ssim.item(), ssim_map=smap.detach().numpy().reshape(shape),
                grad=x.grad.numpy().reshape(shape))
