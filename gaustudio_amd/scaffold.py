"""Scaffold-GS inference in front of the operator: anchors + three small MLPs + camera -> Gaussians -> render, what the
reference's `scaffold_pcd` + `scaffold_renderer` do (gaustudio/models/scaffold_sg.py, gaustudio/renderers/scaffold_renderer.py
get_gaussians_properties and prefilter_voxel).

    model = ScaffoldModel.from_modules(mlp_opacity, mlp_cov, mlp_color, mlp_feature_bank, anchor=..., anchor_feat=...,
                                       offset=..., scaling=..., rot=...)          # or ScaffoldModel.from_raw(...)
    mask, radii = visible_anchors(model, view)                     # the filter alone (csrc/gsr_scaffold.hip, pass 1)
    g = decode(model, view)                                        # ScaffoldGaussians: two HIP passes over the anchors
    g = decode_torch(model, view, mask)                            # the same in plain torch ops: any device, differentiable
    out = render_scaffold(model, camera_settings)                  # decode + GaussianRasterizer(colors_precomp)
    g = decode(model, view, backward="hip")                        # training: the same forward, gradients by the HIP backward
    out = render_scaffold(model, camera_settings, backward="hip")

`view` / `camera_settings` is the operator's GaussianRasterizationSettings.  Contract, quirks and what is unsupported:
INTEGRATION.md s23 (the gradient: s23a); the definition of every bit `decode` returns is tests/scaffold_model.py, of every bit
of its HIP gradient tests/scaffold_grad_model.py.  `decode` takes ROCm tensors only and has no CPU fallback; every call runs
on the current stream of the tensors' device.
"""
import ctypes
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from ._abi import call, on_rocm, same_device

FEAT_DIM = 32          # the reference's `anchor_feat: 32`; the hidden width of every MLP equals it
MAX_OFFSETS = 16
MAX_ANCHORS = 2 ** 24

_ERRORS = {-2: "{what}: the library rejected the arguments (sizes, a missing tensor)",
           -4: (MemoryError, "{what}: the workspace allocation failed")}

Mlp = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]      # W1 [32,in], b1 [32], W2 [out,32], b2 [out]


class ScaffoldGaussians(NamedTuple):
    """What decode returns: M Gaussians in anchor-major, offset-minor order (the order of the reference's
    concatenated_all[mask]).  opacity is [M,1]; anchor_index / offset_index int32 [M]; visible bool [N]; radii int32 [N]
    (None when the caller gave the mask, and from decode_torch)."""
    xyz: torch.Tensor
    colors: torch.Tensor
    opacity: torch.Tensor
    scales: torch.Tensor
    rotations: torch.Tensor
    anchor_index: torch.Tensor
    offset_index: torch.Tensor
    visible: torch.Tensor
    radii: Optional[torch.Tensor]


def _linear_pair(name, seq, n_in, n_out, last):
    """(W1, b1, W2, b2) of an nn.Sequential(Linear(n_in, 32), ReLU, Linear(32, n_out)[, last])."""
    if not isinstance(seq, nn.Sequential):
        raise TypeError(f"{name} must be an nn.Sequential, got {type(seq).__name__}")
    layers = list(seq)
    want = [nn.Linear, nn.ReLU, nn.Linear] + ([last] if last is not None else [])
    if len(layers) != len(want) or any(not isinstance(l, w) for l, w in zip(layers, want)):
        raise TypeError(f"{name} must be Sequential({', '.join(w.__name__ for w in want)}), got "
                        f"({', '.join(type(l).__name__ for l in layers)})")
    l1, l2 = layers[0], layers[2]
    if l1.bias is None or l2.bias is None:
        raise ValueError(f"{name}: both Linear layers need a bias")
    if last is nn.Softmax and layers[3].dim not in (1, -1):
        raise ValueError(f"{name}: the Softmax must run over dim 1")
    if l1.out_features != FEAT_DIM or l2.in_features != FEAT_DIM:
        raise ValueError(f"{name}: hidden width {l1.out_features} (feat_dim): only feat_dim = {FEAT_DIM} is supported")
    if l1.in_features != n_in:
        raise ValueError(f"{name}: the first Linear takes {l1.in_features} inputs, expected {n_in}")
    if l2.out_features != n_out:
        raise ValueError(f"{name}: the last Linear has {l2.out_features} outputs, expected {n_out}")
    return (l1.weight, l1.bias, l2.weight, l2.bias)


def _check_k(k):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_OFFSETS:
        raise ValueError(f"n_offsets must be an int in [1, {MAX_OFFSETS}], got {k!r}")
    return k


class ScaffoldModel:
    """A plain container: anchor [N,3], anchor_feat [N,32], offset [N,k,3], scaling [N,6] (ACTIVATED, as
    get_attribute("scale") gives it: columns 0:3 scale the offsets, 3:6 the covariance), rot [N,4] (activated; the filter
    alone reads it), the three MLPs and optionally the feature bank as (W1, b1, W2, b2) in nn.Linear layout, and n_offsets = k.
    float32 throughout."""

    _ATTRS = ("anchor", "anchor_feat", "offset", "scaling", "rot")
    _MLPS = ("mlp_opacity", "mlp_cov", "mlp_color", "mlp_feature_bank")

    def __init__(self, anchor, anchor_feat, offset, scaling, rot, mlp_opacity, mlp_cov, mlp_color, mlp_feature_bank=None,
                 n_offsets=None):
        self.anchor, self.anchor_feat, self.offset, self.scaling, self.rot = anchor, anchor_feat, offset, scaling, rot
        self.mlp_opacity, self.mlp_cov, self.mlp_color = tuple(mlp_opacity), tuple(mlp_cov), tuple(mlp_color)
        self.mlp_feature_bank = None if mlp_feature_bank is None else tuple(mlp_feature_bank)
        if n_offsets is None and torch.is_tensor(offset) and offset.dim() == 3:
            n_offsets = int(offset.shape[1])
        self.n_offsets = n_offsets
        self.check()

    @classmethod
    def from_modules(cls, mlp_opacity, mlp_cov, mlp_color, mlp_feature_bank=None, *, anchor, anchor_feat, offset, scaling, rot,
                     n_offsets=None):
        """From nn.Sequentials of the reference's shape (scaffold_sg.py:49-76): Linear(36, 32), ReLU, Linear(32, k | 7k | 3k)
        followed by Tanh (opacity), nothing (cov) and Sigmoid (color); the bank Linear(4, 32), ReLU, Linear(32, 3),
        Softmax(dim=1).  Layer types and sizes are checked; the weights are shared with the modules, not copied."""
        k = _check_k(int(offset.shape[1]) if n_offsets is None and torch.is_tensor(offset) and offset.dim() == 3 else n_offsets)
        n_in = FEAT_DIM + 4
        return cls(anchor, anchor_feat, offset, scaling, rot,
                   _linear_pair("mlp_opacity", mlp_opacity, n_in, k, nn.Tanh),
                   _linear_pair("mlp_cov", mlp_cov, n_in, 7 * k, None),
                   _linear_pair("mlp_color", mlp_color, n_in, 3 * k, nn.Sigmoid),
                   None if mlp_feature_bank is None else _linear_pair("mlp_feature_bank", mlp_feature_bank, 4, 3, nn.Softmax),
                   n_offsets=k)

    @classmethod
    def from_raw(cls, anchor, anchor_feat, offset, scale_raw, rot_raw, mlp_opacity, mlp_cov, mlp_color, mlp_feature_bank=None,
                 n_offsets=None):
        """From the stored (pre-activation) attributes: scaling = exp(scale_raw), rot = rot_raw / max(|rot_raw|, 1e-12), the
        model's activations (scaffold_sg.py:23-27), evaluated by torch."""
        return cls(anchor, anchor_feat, offset, torch.exp(scale_raw), F.normalize(rot_raw), mlp_opacity, mlp_cov, mlp_color,
                   mlp_feature_bank, n_offsets=n_offsets)

    def tensors(self):
        """name -> tensor, every tensor of the model."""
        out = {k: getattr(self, k) for k in self._ATTRS}
        for m in self._MLPS:
            w = getattr(self, m)
            if w is not None:
                out.update({f"{m}.{n}": t for n, t in zip(("W1", "b1", "W2", "b2"), w)})
        return out

    def check(self):
        """Types, dtypes, shapes and sizes; no device is touched."""
        k = _check_k(self.n_offsets)
        ts = self.tensors()
        for name, t in ts.items():
            if not torch.is_tensor(t):
                raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
            if t.dtype != torch.float32:
                raise TypeError(f"{name} must be float32, got {t.dtype}")
        if self.anchor_feat.dim() != 2:
            raise ValueError(f"anchor_feat must have shape [N, {FEAT_DIM}], got {list(self.anchor_feat.shape)}")
        if self.anchor_feat.shape[1] != FEAT_DIM:
            raise ValueError(f"anchor_feat has feat_dim = {self.anchor_feat.shape[1]}: only feat_dim = {FEAT_DIM} is supported")
        n = self.anchor_feat.shape[0]
        for name, shape in (("anchor", (n, 3)), ("offset", (n, k, 3)), ("scaling", (n, 6)), ("rot", (n, 4))):
            if tuple(ts[name].shape) != shape:
                raise ValueError(f"{name} must have shape {list(shape)}, got {list(ts[name].shape)}")
        if n > MAX_ANCHORS or n * k >= 2 ** 31:
            raise ValueError(f"at most 2^24 anchors and fewer than 2^31 offsets, got {n} x {k}")
        for m, n_in, n_out in (("mlp_opacity", FEAT_DIM + 4, k), ("mlp_cov", FEAT_DIM + 4, 7 * k), ("mlp_color", FEAT_DIM + 4, 3 * k),
                               ("mlp_feature_bank", 4, 3)):
            w = getattr(self, m)
            if w is None:
                continue
            if len(w) != 4:
                raise ValueError(f"{m} must be (W1, b1, W2, b2)")
            if w[0].dim() == 2 and w[0].shape[0] != FEAT_DIM:
                raise ValueError(f"{m}: hidden width {w[0].shape[0]} (feat_dim): only feat_dim = {FEAT_DIM} is supported")
            for t, shape, nm in zip(w, ((FEAT_DIM, n_in), (FEAT_DIM,), (n_out, FEAT_DIM), (n_out,)), ("W1", "b1", "W2", "b2")):
                if tuple(t.shape) != shape:
                    raise ValueError(f"{m}.{nm} must have shape {list(shape)}, got {list(t.shape)}")
        return self

    @property
    def num_anchors(self):
        return int(self.anchor.shape[0])

    @property
    def use_feat_bank(self):
        return self.mlp_feature_bank is not None

    def requires_grad(self):
        return any(t.requires_grad for t in self.tensors().values())

    def _map(self, fn):
        mlps = [None if getattr(self, m) is None else tuple(fn(t) for t in getattr(self, m)) for m in self._MLPS]
        return ScaffoldModel(*(fn(getattr(self, a)) for a in self._ATTRS), *mlps, n_offsets=self.n_offsets)

    def to(self, device):
        return self._map(lambda t: t.to(device))


# ----------------------------------------------------------------------------------------------------------- the view
def _check_view(view, need_camera=True):
    for f in ("viewmatrix", "projmatrix", "campos", "tanfovx", "tanfovy", "image_width", "image_height", "scale_modifier"):
        if not hasattr(view, f):
            raise TypeError(f"view must be a GaussianRasterizationSettings (it has no {f})")
    for name, numel in (("campos", 3),) + ((("viewmatrix", 16), ("projmatrix", 16)) if need_camera else ()):
        t = getattr(view, name)
        if not torch.is_tensor(t):
            raise TypeError(f"view.{name} must be a torch tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"view.{name} must be float32, got {t.dtype}")
        if t.numel() != numel:
            raise ValueError(f"view.{name} must have {numel} elements, got {list(t.shape)}")
    if need_camera and not (0 < int(view.image_width) <= 65535 and 0 < int(view.image_height) <= 65535):
        raise ValueError(f"image size {view.image_width} x {view.image_height} out of range")


def _check_mask(model, visible_mask):
    if visible_mask is None:
        return None
    if not torch.is_tensor(visible_mask):
        raise TypeError("visible_mask must be a torch bool tensor or None")
    if visible_mask.dtype != torch.bool:
        raise TypeError(f"visible_mask must be bool, got {visible_mask.dtype}")
    if tuple(visible_mask.shape) != (model.num_anchors,):
        raise ValueError(f"visible_mask must have shape [{model.num_anchors}], got {list(visible_mask.shape)}")
    return visible_mask


def _ready(t):
    return None if t is None else t.detach().contiguous()


def _weights(model):
    """(the HOST array of 16 device pointers the C entries take, the tensors that keep them alive)."""
    keep = []
    arr = (ctypes.c_void_p * 16)()
    for i, m in enumerate(ScaffoldModel._MLPS):
        w = getattr(model, m)
        for j in range(4):
            if w is None:
                arr[4 * i + j] = None
            else:
                t = _ready(w[j])
                keep.append(t)
                arr[4 * i + j] = t.data_ptr()
    return arr, keep


def _count(model, view, visible_mask, what):
    """Pass 1 on the device: (visible u8 [N], radii or None, kept, start, M, the prepared inputs)."""
    model.check()
    _check_view(view, need_camera=visible_mask is None)
    mask = _check_mask(model, visible_mask)
    cam = dict(campos=view.campos) if mask is not None else dict(campos=view.campos, viewmatrix=view.viewmatrix,
                                                                   projmatrix=view.projmatrix)
    on_rocm(**model.tensors(), visible_mask=mask, **cam)
    dev = model.anchor.device
    same_device(dev, ref="anchor", **{k: v for k, v in model.tensors().items() if k != "anchor"}, visible_mask=mask, **cam)
    n, k = model.num_anchors, model.n_offsets
    a = {name: _ready(getattr(model, name)) for name in ScaffoldModel._ATTRS}
    warr, wkeep = _weights(model)
    cam = {name: _ready(t) for name, t in cam.items()}
    visible = torch.empty(n, dtype=torch.uint8, device=dev)
    radii = torch.empty(n, dtype=torch.int32, device=dev) if mask is None else None
    kept = torch.empty(n, dtype=torch.int16, device=dev)
    start = torch.empty(n + 1, dtype=torch.int32, device=dev)
    total = ctypes.c_int(0)
    if n > 0:
        mask_u8 = None if mask is None else mask.contiguous().view(torch.uint8)
        call("gsr_scaffold_count", dev, a["anchor"], a["anchor_feat"], a["scaling"], a["rot"], warr, n, k, cam.get("viewmatrix"),
             cam.get("projmatrix"), cam["campos"], ctypes.c_float(view.tanfovx), ctypes.c_float(view.tanfovy),
             int(view.image_width), int(view.image_height), ctypes.c_float(view.scale_modifier), mask_u8, visible, radii, kept, start,
             ctypes.byref(total), workspace=True, what=what, errors=_ERRORS)
    return visible.view(torch.bool), radii, kept, start, int(total.value), a, (warr, wkeep), cam


def visible_anchors(model, view):
    """The filter alone, what prefilter_voxel means by `radii_pure > 0`: (mask bool [N], radii int32 [N]), radii being what this
    project's operator returns for Gaussians with means3D = anchor, scales = scaling[:, :3], rotations = rot and the view's
    scale_modifier (near-plane cull, det == 0, the 0.3 low-pass, ceil(3 sqrt(lambda_max)), the zero-area tile rect; opacity does
    not enter).  Runs pass 1 of decode (the opacity MLP included) and drops the rest."""
    visible, radii, *_ = _count(model, view, None, "visible_anchors")
    return visible, radii


def decode(model, view, visible_mask=None, backward="torch"):
    """The Gaussians of one view (ScaffoldGaussians), by two HIP passes over the anchors (csrc/gsr_scaffold.hip): count (filter,
    view direction, feature bank, opacity MLP, scan) and emit (covariance and colour MLPs, activations, compaction), with one
    4-byte read-back in between.  visible_mask (bool [N]) replaces the camera test.  ROCm tensors only.

    Per kept (anchor a, offset j), kept meaning visible[a] and opacity logit > 0 (the reference's tanh(o) > 0, taken on the
    logit): opacity = tanh(logit), colors = sigmoid, scales = scaling[a,3:6] sigmoid(o[0:3]), rotations = o[3:7] / max(|.|, 1e-12),
    xyz = anchor + offset scaling[a,0:3].  Every dot product is bias first, then a fused multiply-add per input in ascending
    order; tanh, sigmoid and the bank's softmax come from the library's polynomial exp.  Two calls return the same bits, and
    tests/scaffold_model.py reproduces them on a CPU.

    TRAINING: when grad mode is on and any tensor of the model requires grad, `backward` chooses the differentiable path.
    "torch" (the default): decode dispatches to decode_torch -- the differentiable restatement in torch ops -- with the mask of
    visible_anchors (or the caller's).  Its logits differ from the HIP path's in the last bits (torch's GEMM sums in another
    order), so an offset whose logit is within rounding of 0 can be kept by one path and dropped by the other.
    "hip": the two HIP passes above stay the forward (the same bits as under no_grad) and the gradient is the HIP backward
    gsr_scaffold_backward (tests/scaffold_grad_model.py defines its bits): d anchor, anchor_feat, offset,
    scaling and the weights of every MLP; the visible mask, the kept mask, rot and the camera are constants.  Under no_grad, or
    with nothing requiring grad, `backward` changes nothing."""
    if backward not in ("torch", "hip"):
        raise ValueError(f"backward must be 'torch' or 'hip', got {backward!r}")
    if torch.is_grad_enabled() and model.check().requires_grad():
        if backward == "hip":
            return _decode_hip_grad(model, view, visible_mask)
        if visible_mask is None:
            with torch.no_grad():
                visible_mask, radii = visible_anchors(model, view)
        else:
            radii = None
        return decode_torch(model, view, visible_mask)._replace(radii=radii)
    return _emit(model, _count(model, view, visible_mask, "decode"))


def _emit(model, counted):
    """Pass 2 on what _count returned."""
    visible, radii, kept, start, m, a, (warr, wkeep), cam = counted
    dev = model.anchor.device
    n, k = model.num_anchors, model.n_offsets
    new = lambda c, dt=torch.float32: torch.empty((m, c) if c else (m,), dtype=dt, device=dev)
    xyz, colors, opacity, scales, rotations = new(3), new(3), new(1), new(3), new(4)
    aidx, oidx = new(0, torch.int32), new(0, torch.int32)
    if m > 0:
        call("gsr_scaffold_emit", dev, a["anchor"], a["anchor_feat"], a["offset"], a["scaling"], warr, n, k, cam["campos"], kept, start,
             m, xyz, colors, opacity, scales, rotations, aidx, oidx, what="decode", errors=_ERRORS)
    return ScaffoldGaussians(xyz, colors, opacity, scales, rotations, aidx, oidx, visible, radii)


_GRAD_ATTRS = ("anchor", "anchor_feat", "offset", "scaling")


def _pointer_table(tensors):
    arr = (ctypes.c_void_p * 16)()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


class _DecodeHip(torch.autograd.Function):
    """decode with the HIP backward.  Inputs: the model and the view (plain objects), then the differentiable tensors: anchor,
    anchor_feat, offset, scaling and the 12 or 16 MLP tensors.  Saved: those, campos, kept, start; M."""

    @staticmethod
    def forward(ctx, model, view, visible_mask, *tensors):
        counted = _count(model, view, visible_mask, "decode")
        g = _emit(model, counted)
        visible, radii, kept, start, m, a, (warr, wkeep), cam = counted
        ctx.save_for_backward(*(a[name] for name in _GRAD_ATTRS), *wkeep, cam["campos"], kept, start)
        ctx.num_gaussians, ctx.n_offsets, ctx.bank = m, model.n_offsets, model.use_feat_bank
        nondiff = (g.anchor_index, g.offset_index, g.visible) + (() if radii is None else (radii,))
        ctx.mark_non_differentiable(*nondiff)
        return (g.xyz, g.colors, g.opacity, g.scales, g.rotations) + nondiff

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_xyz, g_col, g_op, g_sc, g_rot, *_):
        saved = ctx.saved_tensors
        anchor, feat, offset, scaling = saved[:4]
        nw = 16 if ctx.bank else 12
        weights, (campos, kept, start) = saved[4:4 + nw], saved[4 + nw:]
        dev, m, k, n = anchor.device, ctx.num_gaussians, ctx.n_offsets, anchor.shape[0]
        cots = {}
        for name, t, cols in (("xyz", g_xyz, 3), ("colors", g_col, 3), ("opacity", g_op, 1), ("scales", g_sc, 3), ("rotations", g_rot, 4)):
            if t is not None:
                if t.dtype != torch.float32 or tuple(t.shape) != (m, cols):
                    raise ValueError(f"decode backward: the cotangent of {name} must be float32 [{m}, {cols}], got {t.dtype} "
                                     f"{list(t.shape)}")
                t = t.contiguous()
            cots[name] = t
        on_rocm(**{"grad_" + name: t for name, t in cots.items()})
        same_device(dev, ref="anchor", **{"grad_" + name: t for name, t in cots.items()})
        d_attr = [torch.empty_like(t) for t in (anchor, feat, offset, scaling)]
        d_w = [torch.empty_like(t) for t in weights]
        if n > 0:
            call("gsr_scaffold_backward", dev, anchor, feat, offset, scaling, _pointer_table(list(weights) + [None] * (16 - nw)), n, k,
                 campos, kept, start, m, cots["xyz"], cots["colors"], cots["opacity"], cots["scales"], cots["rotations"], *d_attr,
                 _pointer_table(d_w + [None] * (16 - nw)), workspace=True, what="decode backward", errors=_ERRORS)
        else:
            for t in d_w:
                t.zero_()
        grads = d_attr + d_w
        return (None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:]))


def _decode_hip_grad(model, view, visible_mask):
    ts = [getattr(model, name) for name in _GRAD_ATTRS]
    for m in ScaffoldModel._MLPS:
        if getattr(model, m) is not None:
            ts.extend(getattr(model, m))
    out = _DecodeHip.apply(model, view, visible_mask, *ts)
    return ScaffoldGaussians(*out[:8], out[8] if len(out) > 8 else None)


def _kept_bool(model, kept):
    """decode_torch's kept argument as bool [N, k]: a bool [N, k] tensor, or the bit mask [N] (uint16 / int16, bit j = offset j)
    that the HIP passes use."""
    n, k = model.num_anchors, model.n_offsets
    if not torch.is_tensor(kept):
        raise TypeError("kept must be a torch tensor or None")
    if kept.dtype == torch.bool:
        if tuple(kept.shape) != (n, k):
            raise ValueError(f"a bool kept must have shape [{n}, {k}], got {list(kept.shape)}")
        return kept
    if kept.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)):
        raise TypeError(f"kept must be bool [N, k] or a 16-bit mask [N] (uint16 / int16), got {kept.dtype}")
    if tuple(kept.shape) != (n,):
        raise ValueError(f"a bit-mask kept must have shape [{n}], got {list(kept.shape)}")
    bits = kept.view(torch.int16).to(torch.int32) & 0xFFFF
    return ((bits[:, None] >> torch.arange(k, device=kept.device, dtype=torch.int32)[None, :]) & 1).bool()


def _mlp(w, x):
    return F.linear(torch.relu(F.linear(x, w[0], w[1])), w[2], w[3])


def decode_torch(model, view, visible_mask=None, kept=None):
    """get_gaussians_properties restated in plain torch ops: runs on any device, is differentiable, and is the default training
    path (decode dispatches here under grad).  visible_mask bool [N]; None = every anchor.  Returns ScaffoldGaussians with
    radii = None.  The logits differ from decode's in the last bits, because torch's GEMM sums in a different order: compare
    the two within a bound, never for equality.  kept (bool [N, k], or the bit mask [N] of the HIP passes) replaces the
    `logit > 0` rule for the visible anchors, so that both paths can work on the same set of Gaussians."""
    model.check()
    kept = None if kept is None else _kept_bool(model, kept)
    _check_view(view, need_camera=False)
    mask = _check_mask(model, visible_mask)
    n, k = model.num_anchors, model.n_offsets
    dev = model.anchor.device
    same_device(dev, ref="anchor", **{name: t for name, t in model.tensors().items() if name != "anchor"}, visible_mask=mask,
                kept=kept)
    if mask is None:
        mask = torch.ones(n, dtype=torch.bool, device=dev)
    feat, anchor = model.anchor_feat[mask], model.anchor[mask]
    offsets, scaling = model.offset[mask], model.scaling[mask]
    ob_view = anchor - view.campos.to(dev).reshape(1, 3)
    ob_dist = ob_view.norm(dim=1, keepdim=True)
    ob_view = ob_view / ob_dist
    if model.use_feat_bank:
        w = torch.softmax(_mlp(model.mlp_feature_bank, torch.cat([ob_view, ob_dist], dim=1)), dim=1)
        feat = feat[:, ::4].repeat(1, 4) * w[:, 0:1] + feat[:, ::2].repeat(1, 2) * w[:, 1:2] + feat * w[:, 2:3]
    x = torch.cat([feat, ob_view, ob_dist], dim=1)
    logit = _mlp(model.mlp_opacity, x).reshape(-1)
    keep = logit > 0.0 if kept is None else kept[mask].reshape(-1)
    color = torch.sigmoid(_mlp(model.mlp_color, x)).reshape(-1, 3)[keep]
    cov = _mlp(model.mlp_cov, x).reshape(-1, 7)[keep]
    rep = lambda t: t.repeat_interleave(k, dim=0)[keep]
    scaling_r, anchor_r = rep(scaling), rep(anchor)
    vis_idx = torch.nonzero(mask).reshape(-1)
    flat = torch.nonzero(keep).reshape(-1)
    return ScaffoldGaussians(
        xyz=anchor_r + offsets.reshape(-1, 3)[keep] * scaling_r[:, :3], colors=color,
        opacity=torch.tanh(logit[keep]).reshape(-1, 1), scales=scaling_r[:, 3:] * torch.sigmoid(cov[:, :3]),
        rotations=F.normalize(cov[:, 3:7]), anchor_index=vis_idx[flat // k].to(torch.int32),
        offset_index=(flat % k).to(torch.int32), visible=mask, radii=None)


def render_scaffold(model, camera_settings, bg=None, visible_mask=None, kernel_size=0.0, subpixel_offset=None, backward="torch"):
    """ScaffoldRenderer.render: decode, then the operator with colors_precomp.  Returns the reference's dict -- `render`,
    `viewspace_points`, `visibility_filter`, `radii` -- plus `depth`, `median_depth`, `opacity` (this operator's other outputs)
    and `gaussians` (the ScaffoldGaussians).  bg replaces camera_settings.bg.  kernel_size and subpixel_offset are the
    arguments of a rasterizer fork the vendored operator is not: anything but 0 / None raises.  backward: decode's ("torch" or
    "hip": which decoder gradient trains the model)."""
    if kernel_size not in (0, 0.0) or isinstance(kernel_size, bool):
        raise NotImplementedError("render_scaffold: kernel_size is not supported (the operator has no 3D filter); pass 0")
    if subpixel_offset is not None:
        raise NotImplementedError("render_scaffold: subpixel_offset is not supported")
    from .rasterizer import GaussianRasterizer
    g = decode(model, camera_settings, visible_mask, backward=backward)
    rs = camera_settings if bg is None else camera_settings._replace(bg=bg)
    screenspace = torch.zeros_like(g.xyz, requires_grad=True) + 0
    try:
        screenspace.retain_grad()
    except RuntimeError:
        pass
    color, radii, depth, median, opac = GaussianRasterizer(rs)(means3D=g.xyz, means2D=screenspace, opacities=g.opacity,
                                                              colors_precomp=g.colors, scales=g.scales, rotations=g.rotations)
    return dict(render=color, viewspace_points=screenspace, visibility_filter=radii > 0, radii=radii, depth=depth,
                median_depth=median, opacity=opac, gaussians=g)
