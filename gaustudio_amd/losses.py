"""The photometric loss Gaussian splatting is trained with, on the GPU (csrc/gsr_loss.hip):

    loss = (1 - lambda_dssim) * L1(image, target) + lambda_dssim * (1 - SSIM(image, target))

with the published 3DGS `l1_loss` / `ssim` (11 x 11 Gaussian window, sigma 1.5, zero padding, mean over every element).
`image` and `target` are float32 tensors of one shape [..., H, W]; every leading dimension is a plane.  One fused forward
kernel and one backward kernel replace five depthwise conv2d calls, ~25 elementwise passes and their autograd; the gradient
[3,H,W] is what the rasterizer's backward takes as grad_out_color.  Nothing here synchronises with the host: the loss stays a
0-dim device tensor and the backward reads its upstream gradient from device memory.

Contract, float order included: INTEGRATION.md s24; to the bit: tests/loss_model.py.
"""
import ctypes
import math
from types import SimpleNamespace

import torch

from ._abi import call, on_rocm

TILE_H, TILE_W = 16, 64      # the tile of one workgroup (csrc/gsr_loss.hip TH, TW)
_ERRORS = {-2: "{what}: planes, height and width must be >= 1 and planes * height * width < 2^31"}


def _check(image, target, lambda_dssim):
    """Types, shapes and dtypes first, then the devices.  Returns (image, target, lambda) with contiguous tensors."""
    for name, t in (("image", image), ("target", target)):
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a torch tensor")
    if isinstance(lambda_dssim, bool) or not isinstance(lambda_dssim, (int, float)):
        raise TypeError("lambda_dssim must be a number")
    lam = float(lambda_dssim)
    if not math.isfinite(lam) or not 0.0 <= lam <= 1.0:
        raise ValueError(f"lambda_dssim must be in [0, 1], got {lambda_dssim}")
    if image.dim() < 2:
        raise ValueError(f"image must have shape [..., H, W], got {list(image.shape)}")
    if tuple(image.shape) != tuple(target.shape):
        raise ValueError(f"image {list(image.shape)} and target {list(target.shape)} must have one shape")
    for name, t in (("image", image), ("target", target)):
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
    if image.numel() == 0:
        raise ValueError("image is empty")
    if image.numel() >= 2 ** 31:
        raise ValueError("image must have fewer than 2^31 elements")
    if target.requires_grad:
        raise NotImplementedError("the gradient with respect to target is not implemented: pass target.detach()")
    on_rocm(image=image, target=target)
    if image.device != target.device:
        raise ValueError(f"image is on {image.device}, target on {target.device}")
    return image.contiguous(), target.contiguous(), lam


def _forward(image, target, lam, want_maps, want_ssim_map=False):
    """One launch of the forward on checked, contiguous tensors.  Returns the state: out [3] = (loss, l1, ssim), maps
    [3, ...] or None, ssim_map or None."""
    H, W = image.shape[-2:]
    planes = image.numel() // (H * W)
    out = torch.empty(3, dtype=torch.float32, device=image.device)
    maps = torch.empty((3,) + tuple(image.shape), dtype=torch.float32, device=image.device) if want_maps else None
    smap = torch.empty_like(image) if want_ssim_map else None
    call("gsr_photometric_fwd", image.device, image, target, ctypes.c_longlong(planes), H, W, ctypes.c_float(lam), smap, maps,
         out, workspace=True, what="photometric_loss", errors=_ERRORS)
    return SimpleNamespace(out=out, maps=maps, ssim_map=smap)


def _backward(image, target, maps, lam, grad_loss):
    """dL/dimage from the saved maps and the upstream gradient of the loss, a 0-dim float32 DEVICE tensor."""
    H, W = image.shape[-2:]
    grad = torch.empty_like(image)
    g = grad_loss.detach().to(device=image.device, dtype=torch.float32).reshape(1).contiguous()
    call("gsr_photometric_bwd", image.device, image, target, maps, ctypes.c_longlong(image.numel() // (H * W)), H, W,
         ctypes.c_float(lam), g, grad, what="photometric_loss backward", errors=_ERRORS)
    return grad


class _PhotometricLoss(torch.autograd.Function):
    """(loss, l1, ssim) of one forward launch; the gradient flows through `loss` only.  `box` receives the forward state."""

    @staticmethod
    def forward(ctx, image, target, lam, want_maps, box):
        st = _forward(image.detach(), target, lam, want_maps)
        box.append(st)
        ctx.lam = lam
        if want_maps:
            ctx.save_for_backward(image, target, st.maps)
        loss, l1, ssim_ = st.out.unbind(0)
        ctx.mark_non_differentiable(l1, ssim_)
        return loss, l1, ssim_

    @staticmethod
    def backward(ctx, g_loss, g_l1, g_ssim):
        image, target, maps = ctx.saved_tensors
        return _backward(image.detach(), target, maps, ctx.lam, g_loss), None, None, None, None


def photometric_loss_with_state(image, target, lambda_dssim=0.2):
    """((loss, l1, ssim), state): photometric_loss_with_parts and the state its forward left behind -- `state.maps` is None
    unless image.requires_grad and grad mode is enabled (what a forward under no_grad must not allocate)."""
    image, target, lam = _check(image, target, lambda_dssim)
    box = []
    parts = _PhotometricLoss.apply(image, target, lam, bool(image.requires_grad and torch.is_grad_enabled()), box)
    return parts, box[0]


def photometric_loss_with_parts(image, target, lambda_dssim=0.2):
    """(loss, l1, ssim) from one launch: 0-dim float32 device tensors.  `loss` is differentiable in image."""
    return photometric_loss_with_state(image, target, lambda_dssim)[0]


def photometric_loss(image, target, lambda_dssim=0.2):
    """(1 - lambda_dssim) * l1 + lambda_dssim * (1 - ssim): a 0-dim float32 device tensor, differentiable in image."""
    return photometric_loss_with_parts(image, target, lambda_dssim)[0]


def l1_loss(image, target):
    """mean |image - target|: the l1 part of photometric_loss, from the same kernels (forward only)."""
    image, target, lam = _check(image, target, 0.2)
    return _forward(image.detach(), target, lam, False).out[1]


def ssim(image, target):
    """Mean SSIM: the ssim part of photometric_loss, from the same kernels (forward only)."""
    image, target, lam = _check(image, target, 0.2)
    return _forward(image.detach(), target, lam, False).out[2]


def ssim_map(image, target):
    """The per-pixel SSIM, in image's shape (forward only)."""
    image, target, lam = _check(image, target, 0.2)
    return _forward(image.detach(), target, lam, False, want_ssim_map=True).ssim_map
