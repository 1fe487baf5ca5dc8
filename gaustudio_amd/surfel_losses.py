"""The two geometric regularisers 2D Gaussian surfels are trained with, on the GPU (csrc/gsr_geoloss.hip), on the `allmap`
[7,H,W] the surfel operator returns (a0 = sum w z, a1 = alpha, a2..a4 = view-space normal, a5 = median depth, a6 = distortion):

    depth        = (1 - depth_ratio) * nan_to_num(a0 / a1) + depth_ratio * nan_to_num(a5)
    surf_normal  = normalize(cross(p(x, y+1) - p(x, y-1), p(x+1, y) - p(x-1, y))) * a1.detach(),  0 on the one-pixel border,
                   p(x, y) = depth(x, y) * ((x - cx) / fx, (y - cy) / fy, 1)
    normal_loss  = lambda_normal * mean(1 - <(a2, a3, a4), surf_normal>)
    dist_loss    = lambda_dist * mean(a6)
    loss         = normal_loss + dist_loss

One fused forward kernel and one backward kernel replace about 25 torch ops with [H,W,3] intermediates and their autograd; the
gradient [7,H,W] is what the surfel operator's backward takes as grad_allmap.  Nothing here synchronises with the host when the
intrinsics are Python floats or a CPU tensor: the loss stays a 0-dim device tensor and the backward reads its upstream gradient
from device memory.  The backward recomputes the forward's quantities: the forward saves nothing but `allmap` itself.

Contract, float order included: INTEGRATION.md s26; to the bit: tests/geoloss_model.py.
"""
import ctypes
import math
from types import SimpleNamespace

import torch

from ._abi import call, on_rocm

TILE_H, TILE_W = 16, 64      # the tile of one workgroup (csrc/gsr_geoloss.hip TH, TW)
MAP_NAMES = ("rendered_depth", "rendered_median_depth", "surf_depth", "surf_normal", "rendered_normal", "normal_error")
_ERRORS = {-2: "{what}: height and width must be >= 1 with 7 * height * width < 2^31, depth_ratio in [0, 1], the lambdas finite "
               "and >= 0, the intrinsics finite with fx, fy != 0"}


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{name} must be a number")
    return float(v)


def _check(allmap, intrinsics, lambda_normal, lambda_dist, depth_ratio, viewmatrix=None):
    """Types, shape, dtype, size, the scalars, the intrinsics, then the device.  Returns (allmap contiguous, (fx, fy, cx, cy),
    lambda_normal, lambda_dist, depth_ratio, viewmatrix on allmap's device or None)."""
    if not torch.is_tensor(allmap):
        raise TypeError("allmap must be a torch tensor")
    if not torch.is_tensor(intrinsics) and not isinstance(intrinsics, (tuple, list)):
        raise TypeError("intrinsics must be (fx, fy, cx, cy): a tuple or list of numbers, or a tensor of four values")
    if not torch.is_tensor(intrinsics):
        for v in intrinsics:
            _number("every value of intrinsics", v)
    ln, ld, rho = _number("lambda_normal", lambda_normal), _number("lambda_dist", lambda_dist), _number("depth_ratio", depth_ratio)
    if viewmatrix is not None and not torch.is_tensor(viewmatrix):
        raise TypeError("viewmatrix must be a torch tensor or None")
    if allmap.dim() != 3 or allmap.shape[0] != 7:
        raise ValueError(f"allmap must have shape [7, H, W], got {list(allmap.shape)}")
    n_intr = intrinsics.numel() if torch.is_tensor(intrinsics) else len(intrinsics)
    if n_intr != 4:
        raise ValueError(f"intrinsics must hold four values (fx, fy, cx, cy), got {n_intr}")
    if viewmatrix is not None and tuple(viewmatrix.shape) != (4, 4):
        raise ValueError(f"viewmatrix must have shape [4, 4], got {list(viewmatrix.shape)}")
    if allmap.dtype != torch.float32:
        raise TypeError(f"allmap must be float32, got {allmap.dtype}")
    if viewmatrix is not None and viewmatrix.dtype != torch.float32:
        raise TypeError(f"viewmatrix must be float32, got {viewmatrix.dtype}")
    if allmap.numel() == 0:
        raise ValueError("allmap is empty")
    if allmap.numel() >= 2 ** 31:
        raise ValueError("allmap must have fewer than 2^31 elements")
    if not 0.0 <= rho <= 1.0:                       # (a NaN fails both comparisons)
        raise ValueError(f"depth_ratio must be in [0, 1], got {depth_ratio}")
    for name, v in (("lambda_normal", ln), ("lambda_dist", ld)):
        if not math.isfinite(v) or v < 0.0:
            raise ValueError(f"{name} must be finite and >= 0, got {v}")
    # a device tensor of intrinsics is read back here: the one synchronisation of this module, and the caller's choice
    cam = tuple(float(v) for v in (intrinsics.detach().reshape(4).tolist() if torch.is_tensor(intrinsics) else intrinsics))
    if not all(math.isfinite(v) for v in cam) or cam[0] == 0.0 or cam[1] == 0.0:
        raise ValueError(f"intrinsics (fx, fy, cx, cy) must be finite with fx, fy != 0, got {cam}")
    cam32 = tuple(ctypes.c_float(v).value for v in cam)
    if not all(math.isfinite(v) for v in cam32) or cam32[0] == 0.0 or cam32[1] == 0.0:
        raise ValueError(f"intrinsics (fx, fy, cx, cy) must be finite with fx, fy != 0 as float32, got {cam}")
    on_rocm(allmap=allmap)
    if viewmatrix is not None:
        viewmatrix = viewmatrix.detach().to(allmap.device).contiguous()
    return allmap.contiguous(), cam, ln, ld, rho, viewmatrix


def _scalars(cam, rho, ln, ld):
    return [ctypes.c_float(v) for v in cam + (rho, ln, ld)]


def _forward(allmap, cam, ln, ld, rho, viewmatrix=None, want_maps=False):
    """One launch of the forward on a checked, contiguous allmap.  Returns the state: out [3] = (loss, normal_loss, dist_loss),
    maps [10,H,W] or None."""
    H, W = allmap.shape[1:]
    out = torch.empty(3, dtype=torch.float32, device=allmap.device)
    maps = torch.empty((10, H, W), dtype=torch.float32, device=allmap.device) if want_maps else None
    call("gsr_surfel_geoloss_fwd", allmap.device, allmap, H, W, *_scalars(cam, rho, ln, ld), viewmatrix, maps, out, workspace=True,
         what="surfel_geometric_loss", errors=_ERRORS)
    return SimpleNamespace(out=out, maps=maps)


def _backward(allmap, cam, ln, ld, rho, grad_loss):
    """dL/dallmap [7,H,W] from allmap and the upstream gradient of the loss, a 0-dim float32 DEVICE tensor."""
    H, W = allmap.shape[1:]
    grad = torch.empty_like(allmap)
    g = grad_loss.detach().to(device=allmap.device, dtype=torch.float32).reshape(1).contiguous()
    call("gsr_surfel_geoloss_bwd", allmap.device, allmap, H, W, *_scalars(cam, rho, ln, ld), g, grad,
         what="surfel_geometric_loss backward", errors=_ERRORS)
    return grad


class _SurfelGeometricLoss(torch.autograd.Function):
    """(loss, normal_loss, dist_loss) of one forward launch; the gradient flows through `loss` only."""

    @staticmethod
    def forward(ctx, allmap, cam, ln, ld, rho, box):
        st = _forward(allmap.detach(), cam, ln, ld, rho)
        box.append(st)
        ctx.args = (cam, ln, ld, rho)
        ctx.save_for_backward(allmap)
        loss, nl, dl = st.out.unbind(0)
        ctx.mark_non_differentiable(nl, dl)
        return loss, nl, dl

    @staticmethod
    def backward(ctx, g_loss, g_nl, g_dl):
        (allmap,) = ctx.saved_tensors
        cam, ln, ld, rho = ctx.args
        return _backward(allmap.detach(), cam, ln, ld, rho, g_loss), None, None, None, None, None


def surfel_geometric_loss_with_state(allmap, intrinsics, lambda_normal=0.05, lambda_dist=0.0, depth_ratio=0.0):
    """((loss, normal_loss, dist_loss), state): surfel_geometric_loss_with_parts and the state its forward left behind --
    `state.out` [3] and `state.maps`, which is always None here (the backward recomputes; only surfel_maps asks for maps)."""
    allmap, cam, ln, ld, rho, _ = _check(allmap, intrinsics, lambda_normal, lambda_dist, depth_ratio)
    box = []
    parts = _SurfelGeometricLoss.apply(allmap, cam, ln, ld, rho, box)
    return parts, box[0]


def surfel_geometric_loss_with_parts(allmap, intrinsics, lambda_normal=0.05, lambda_dist=0.0, depth_ratio=0.0):
    """(loss, normal_loss, dist_loss) from one launch: 0-dim float32 device tensors.  `loss` is differentiable in allmap."""
    return surfel_geometric_loss_with_state(allmap, intrinsics, lambda_normal, lambda_dist, depth_ratio)[0]


def surfel_geometric_loss(allmap, intrinsics, lambda_normal=0.05, lambda_dist=0.0, depth_ratio=0.0):
    """lambda_normal * mean(1 - <rendered normal, surface normal>) + lambda_dist * mean(distortion): a 0-dim float32 device
    tensor, differentiable in allmap.  intrinsics = (fx, fy, cx, cy) in the operator's pixel convention
    (intrinsics_from_settings): floats or a CPU tensor; a device tensor is accepted and read back (one synchronisation)."""
    return surfel_geometric_loss_with_parts(allmap, intrinsics, lambda_normal, lambda_dist, depth_ratio)[0]


def surfel_maps(allmap, intrinsics, viewmatrix=None, depth_ratio=0.0):
    """What SurfelRenderer.render derives from allmap after the operator, plus the surface normal (forward only): a dict of
    rendered_depth, rendered_median_depth, surf_depth [1,H,W]; surf_normal, rendered_normal [3,H,W]; normal_error [H,W].
    With `viewmatrix` ([4,4] as the operator takes it) both normals are turned to world space, v -> v @ viewmatrix[:3,:3].T."""
    allmap, cam, ln, ld, rho, view = _check(allmap, intrinsics, 0.05, 0.0, depth_ratio, viewmatrix)
    m = _forward(allmap.detach(), cam, ln, ld, rho, view, want_maps=True).maps
    return dict(rendered_depth=m[0:1], rendered_median_depth=m[1:2], surf_depth=m[2:3], surf_normal=m[3:6],
                rendered_normal=m[6:9], normal_error=m[9])


def intrinsics_from_settings(raster_settings):
    """(fx, fy, cx, cy) as Python floats from the operator's settings (projmatrix, viewmatrix, image size), in the operator's
    own pixel convention, pixel = ndc * size / 2 + (size - 1) / 2: the point depth * ((x - cx) / fx,
    (y - cy) / fy, 1) projects onto pixel (x, y).  Evaluated in float64 on the host; matrices on a device are read back."""
    rs = raster_settings
    view = rs.viewmatrix.detach().double().cpu()
    full = rs.projmatrix.detach().double().cpu()
    W, H = int(rs.image_width), int(rs.image_height)
    P = torch.linalg.solve(view, full)               # row vectors: clip = (x, y, z, 1) @ view @ P
    w = float(P[2, 3])
    if not math.isfinite(w) or w == 0.0:
        raise ValueError("projmatrix is no perspective projection of viewmatrix: the clip w does not depend on the view depth")
    fx, fy = float(P[0, 0]) / w * W / 2.0, float(P[1, 1]) / w * H / 2.0
    cx, cy = float(P[2, 0]) / w * W / 2.0 + (W - 1) / 2.0, float(P[2, 1]) / w * H / 2.0 + (H - 1) / 2.0
    return fx, fy, cx, cy
