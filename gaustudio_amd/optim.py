"""The optimiser half of 3DGS training on the GPU (csrc/gsr_optim.hip): GaussianAdam, one launch per step over the six
parameter groups of a Gaussian model, dense or sparse in the rows a view saw (`step(visible=radii)`), and DensityControl, the
adaptive density control of the published method -- clone, split, prune and opacity reset -- as one classify -> scan -> emit
compaction that carries the Adam moments.

    params = dict(xyz=[N,3], f_dc=[N,1,3], f_rest=[N,K,3], opacity=[N,1], scaling=[N,3], rotation=[N,4])   # float32 leaves
    opt = GaussianAdam(params, lr=dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=1.25e-4, opacity=5e-2, scaling=5e-3, rotation=1e-3))
    dc = DensityControl(opt)
    ...  loss.backward();  dc.accumulate(means2D.grad, radii);  opt.step(visible=radii);  opt.zero_grad()
    report = dc.densify_and_prune(max_grad=2e-4, min_opacity=0.005, extent=extent)    # params[...] are new leaves now

Contract, float order included: INTEGRATION.md s25; to the bit: tests/optim_model.py.  There is no CPU fallback.
"""
import ctypes
import math
from collections import namedtuple

import torch

from ._abi import call, on_rocm

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
SH_REST = (0, 3, 8, 15)                 # K of f_rest [N,K,3]: SH degrees 0 .. 3
MAX_WIDTH = 45                          # floats of the widest row
ROW_LIMIT = 2 ** 31                     # rows * MAX_WIDTH stays below it
MAX_SPLIT = 8
_KIND = dict(xyz=1, scaling=2)          # GSR_COMPACT_XYZ / _SCALING; every other group is GSR_COMPACT_COPY
_STATS = 3                              # GSR_COMPACT_STATS

DensifyReport = namedtuple("DensifyReport", "n_cloned n_split n_pruned n_before n_after")


class _AdamGroup(ctypes.Structure):     # include/gsrast.h gsr_adam_group
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("lr", ctypes.c_double), ("width", ctypes.c_int), ("reserved", ctypes.c_int)]


class _CompactGroup(ctypes.Structure):  # include/gsrast.h gsr_compact_group
    _fields_ = [("src", ctypes.c_void_p * 3), ("dst", ctypes.c_void_p * 3), ("width", ctypes.c_int), ("kind", ctypes.c_int)]


def _addr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _tail_shape(name, k):
    return dict(xyz=(3,), f_dc=(1, 3), f_rest=(k, 3), opacity=(1,), scaling=(3,), rotation=(4,))[name]


def check_rows(n, what="the model"):
    """N * 45 < 2^31: the limit of every kernel here, checked before anything is written."""
    if n * MAX_WIDTH >= ROW_LIMIT:
        raise ValueError(f"{what} has {n} rows: rows * {MAX_WIDTH} must stay below 2^31")


def check_params(params):
    """Types, shapes and dtypes first, then the row limit, then the devices.  Returns (N, K)."""
    if not isinstance(params, dict):
        raise TypeError("params must be a dict of the six parameter tensors")
    for name in GROUPS:
        if name not in params:
            raise KeyError(f"params has no '{name}' (it needs {', '.join(GROUPS)})")
    extra = [k for k in params if k not in GROUPS]
    if extra:
        raise KeyError(f"params has unknown groups {extra}")
    for name in GROUPS:
        if not torch.is_tensor(params[name]):
            raise TypeError(f"params['{name}'] must be a torch tensor")
    xyz, rest = params["xyz"], params["f_rest"]
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"xyz must have shape [N, 3], got {list(xyz.shape)}")
    n = int(xyz.shape[0])
    if rest.dim() != 3 or rest.shape[2] != 3 or int(rest.shape[1]) not in SH_REST:
        raise ValueError(f"f_rest must have shape [N, K, 3] with K in {SH_REST}, got {list(rest.shape)}")
    k = int(rest.shape[1])
    for name in GROUPS:
        want = (n,) + _tail_shape(name, k)
        if tuple(params[name].shape) != want:
            raise ValueError(f"{name} must have shape {list(want)} (N = {n} rows like xyz), got {list(params[name].shape)}")
    for name in GROUPS:
        if params[name].dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {params[name].dtype}")
    check_rows(n)
    for name in GROUPS:
        t = params[name]
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if not t.is_leaf:
            raise ValueError(f"{name} must be a leaf tensor")
    on_rocm(**{name: params[name] for name in GROUPS})
    for name in GROUPS:
        if params[name].device != xyz.device:
            raise ValueError(f"{name} is on {params[name].device}, xyz on {xyz.device}")
    return n, k


def check_rows_tensor(name, t, n, dtype, tail=()):
    """A [n, *tail] tensor of one dtype: type, shape and dtype, no device."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch tensor")
    want = (n,) + tuple(tail)
    if tuple(t.shape) != want:
        raise ValueError(f"{name} must have shape {list(want)}, got {list(t.shape)}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")


def check_visible(visible, n):
    check_rows_tensor("visible", visible, n, torch.int32)


def check_noise(noise, n, n_split):
    check_rows_tensor("noise", noise, n, torch.float32, (n_split, 3))


def check_mask(mask, n):
    check_rows_tensor("mask", mask, n, torch.bool)


def _zeros_like_phase(p, fill=True):
    """A float32 tensor of p's shape whose storage sits at p's offset within 16 bytes, so that the step can take a
    parameter and its moments 16 bytes at a time wherever the parameter itself starts."""
    n = p.numel()
    buf = (torch.zeros if fill else torch.empty)(n + 4, dtype=torch.float32, device=p.device)
    off = ((p.data_ptr() - buf.data_ptr()) % 16) // 4 if n else 0
    return buf[off:off + n].view(p.shape)


class GaussianAdam:
    """torch.optim.Adam without weight decay or amsgrad over the six groups, with one step count for all of them.  The
    optimizer owns `exp_avg` and `exp_avg_sq`; `params` is the caller's dict, and DensityControl replaces its tensors."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-15):
        self.num_rows, self.sh_rest = check_params(params)
        if not isinstance(lr, dict):
            raise TypeError("lr must be a dict with a learning rate per group")
        for name in GROUPS:
            if name not in lr:
                raise KeyError(f"lr has no '{name}'")
        b1, b2 = (float(b) for b in betas)
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must be in [0, 1), got {betas}")
        if not (float(eps) >= 0.0):
            raise ValueError(f"eps must be >= 0, got {eps}")
        self.params = params
        self.lr = {}
        for name in GROUPS:
            self.set_lr(name, lr[name])
        self.betas, self.eps = (b1, b2), float(eps)
        self.step_count = 0
        self.exp_avg = {name: _zeros_like_phase(params[name]) for name in GROUPS}
        self.exp_avg_sq = {name: _zeros_like_phase(params[name]) for name in GROUPS}

    @property
    def device(self):
        return self.params["xyz"].device

    def set_lr(self, name, lr):
        if name not in GROUPS:
            raise KeyError(f"no group '{name}'")
        if isinstance(lr, bool) or not isinstance(lr, (int, float)):
            raise TypeError("a learning rate must be a number")
        if not (math.isfinite(lr) and lr >= 0.0):
            raise ValueError(f"a learning rate must be finite and >= 0, got {lr}")
        self.lr[name] = float(lr)

    def zero_grad(self):
        for name in GROUPS:
            self.params[name].grad = None

    @staticmethod
    def expon_lr(lr_init, lr_final, delay_steps=0, delay_mult=1.0, max_steps=1000000):
        """step -> learning rate: the log-linear schedule of the published training (get_expon_lr_func), host Python."""
        def at(step):
            if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
                return 0.0
            if delay_steps > 0:
                delay = delay_mult + (1.0 - delay_mult) * math.sin(0.5 * math.pi * min(max(step / delay_steps, 0.0), 1.0))
            else:
                delay = 1.0
            t = min(max(step / max_steps, 0.0), 1.0)
            return delay * math.exp(math.log(lr_init) * (1.0 - t) + math.log(lr_final) * t)
        return at

    def _check_visible(self, visible):
        check_visible(visible, self.num_rows)
        on_rocm(visible=visible)
        if visible.device != self.device:
            raise ValueError(f"visible is on {visible.device}, the parameters on {self.device}")
        return visible.contiguous()

    def step(self, visible=None):
        """One launch for every group that has a .grad.  visible: int32 [N]; rows with visible <= 0 keep parameter and moments."""
        if visible is not None:
            visible = self._check_visible(visible)
        arr = (_AdamGroup * len(GROUPS))()
        keep = []
        for i, name in enumerate(GROUPS):
            p = self.params[name]
            g = p.grad
            if g is not None:
                if g.dtype != torch.float32 or tuple(g.shape) != tuple(p.shape):
                    raise TypeError(f"the gradient of {name} must be float32 {list(p.shape)}")
                if g.device != p.device:
                    raise ValueError(f"the gradient of {name} is on {g.device}")
                g = g.contiguous()
                keep.append(g)
            arr[i].param, arr[i].grad = _addr(p), _addr(g)
            arr[i].exp_avg, arr[i].exp_avg_sq = _addr(self.exp_avg[name]), _addr(self.exp_avg_sq[name])
            arr[i].lr, arr[i].width = self.lr[name], p.numel() // max(self.num_rows, 1)
        self.step_count += 1
        call("gsr_adam_step", self.device, arr, len(GROUPS), self.num_rows, ctypes.c_double(self.betas[0]),
             ctypes.c_double(self.betas[1]), ctypes.c_double(self.eps), ctypes.c_longlong(self.step_count), visible,
             what="GaussianAdam.step")

    def state_dict(self):
        return dict(step=self.step_count, lr=dict(self.lr), betas=self.betas, eps=self.eps,
                    exp_avg={k: v.detach().clone() for k, v in self.exp_avg.items()},
                    exp_avg_sq={k: v.detach().clone() for k, v in self.exp_avg_sq.items()})

    def load_state_dict(self, state):
        for key in ("exp_avg", "exp_avg_sq"):
            for name in GROUPS:
                t = state[key][name]
                p = self.params[name]
                if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != tuple(p.shape):
                    raise ValueError(f"state {key}['{name}'] must be float32 {list(p.shape)}")
        for key, mine in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            for name in GROUPS:
                m = _zeros_like_phase(self.params[name], fill=False)
                m.copy_(state[key][name])
                mine[name] = m
        self.step_count = int(state["step"])
        for name in GROUPS:
            self.set_lr(name, state["lr"][name])
        self.betas, self.eps = tuple(float(b) for b in state["betas"]), float(state["eps"])


class DensityControl:
    """Clone, split, prune and opacity reset for the model a GaussianAdam steps.  Statistics per row: grad_accum (float32),
    denom and max_radii (int32)."""

    def __init__(self, optimizer, percent_dense=0.01):
        if not isinstance(optimizer, GaussianAdam):
            raise TypeError("optimizer must be a GaussianAdam")
        if not (isinstance(percent_dense, (int, float)) and math.isfinite(percent_dense) and percent_dense > 0):
            raise ValueError(f"percent_dense must be a positive number, got {percent_dense}")
        self.optimizer = optimizer
        self.percent_dense = float(percent_dense)
        self._zero_stats(optimizer.num_rows)

    def _zero_stats(self, n):
        dev = self.optimizer.device
        self.grad_accum = torch.zeros(n, dtype=torch.float32, device=dev)
        self.denom = torch.zeros(n, dtype=torch.int32, device=dev)
        self.max_radii = torch.zeros(n, dtype=torch.int32, device=dev)

    def accumulate(self, means2D_grad, radii):
        """Rows with radii > 0: grad_accum += |means2D_grad[:, :2]|, denom += 1, max_radii = max(max_radii, radii)."""
        n = self.optimizer.num_rows
        check_rows_tensor("means2D_grad", means2D_grad, n, torch.float32, (3,))
        check_rows_tensor("radii", radii, n, torch.int32)
        on_rocm(means2D_grad=means2D_grad, radii=radii)
        dev = self.optimizer.device
        if means2D_grad.device != dev or radii.device != dev:
            raise ValueError(f"means2D_grad and radii must be on {dev}")
        call("gsr_density_accumulate", dev, n, means2D_grad.contiguous(), radii.contiguous(), self.grad_accum, self.denom,
             self.max_radii, what="DensityControl.accumulate")

    # -------------------------------------------------------------------------------------------------- the compaction
    def _classify(self, mask, max_grad, min_opacity, extent, screen, n_split):
        opt = self.optimizer
        n, dev = opt.num_rows, opt.device
        pos = torch.empty(3 * n + 1, dtype=torch.int32, device=dev)
        totals = (ctypes.c_longlong * 4)()
        try:
            call("gsr_densify_classify", dev, n, opt.params["scaling"].detach(), opt.params["opacity"].detach(), self.grad_accum,
                 self.denom, self.max_radii, mask, ctypes.c_float(max_grad), ctypes.c_double(self.percent_dense),
                 ctypes.c_double(extent), ctypes.c_double(min_opacity), screen, n_split, pos, totals, workspace=True,
                 what="DensityControl")
        except RuntimeError:
            if totals[3] < 0:
                check_rows(totals[0] + totals[1] + n_split * totals[2], "the model after this pass")
            raise
        return pos, [int(v) for v in totals]

    def _emit(self, pos, n_after, n_split, noise, carry_stats):
        opt = self.optimizer
        n, dev = opt.num_rows, opt.device
        new_p, new_m, new_v = {}, {}, {}
        ngroups = len(GROUPS) + (1 if carry_stats else 0)
        arr = (_CompactGroup * ngroups)()
        for i, name in enumerate(GROUPS):
            p = opt.params[name].detach()
            new_p[name] = torch.empty((n_after,) + tuple(p.shape[1:]), dtype=torch.float32, device=dev)
            new_m[name] = _zeros_like_phase(new_p[name], fill=False)
            new_v[name] = _zeros_like_phase(new_p[name], fill=False)
            for j, (s, d) in enumerate(((p, new_p[name]), (opt.exp_avg[name], new_m[name]), (opt.exp_avg_sq[name], new_v[name]))):
                arr[i].src[j], arr[i].dst[j] = _addr(s), _addr(d)
            arr[i].width = p.numel() // max(n, 1)
            arr[i].kind = _KIND.get(name, 0) if noise is not None else 0
        old_stats = (self.grad_accum, self.denom, self.max_radii)
        self._zero_stats(n_after)
        if carry_stats:
            g = arr[len(GROUPS)]
            for j, (s, d) in enumerate(zip(old_stats, (self.grad_accum, self.denom, self.max_radii))):
                g.src[j], g.dst[j] = _addr(s), _addr(d)
            g.width, g.kind = 1, _STATS
        if n > 0:
            call("gsr_densify_emit", dev, n, n_split, arr, ngroups, pos, noise, opt.params["scaling"].detach(),
                 opt.params["rotation"].detach(), what="DensityControl")
        for name in GROUPS:
            opt.params[name] = new_p[name].requires_grad_(True)
            opt.exp_avg[name], opt.exp_avg_sq[name] = new_m[name], new_v[name]
        opt.num_rows = n_after

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size=None, n_split=2, noise=None, generator=None):
        """One pass of clone / split / prune.  Returns a DensifyReport; optimizer.params holds new leaf
        tensors afterwards (sources that survive first, then the clones, then child 0 of every split source, child 1, ...),
        the old tensors are left as they were, and the statistics are zero."""
        opt = self.optimizer
        n, dev = opt.num_rows, opt.device
        for name, v in (("max_grad", max_grad), ("min_opacity", min_opacity), ("extent", extent)):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise TypeError(f"{name} must be a number")
        if isinstance(n_split, bool) or not isinstance(n_split, int):
            raise TypeError("n_split must be an integer")
        if not 1 <= n_split <= MAX_SPLIT:
            raise ValueError(f"n_split must be in [1, {MAX_SPLIT}], got {n_split}")
        if math.isnan(max_grad):
            raise ValueError("max_grad is NaN")
        if not (math.isfinite(extent) and extent > 0):
            raise ValueError(f"extent must be positive, got {extent}")
        if not 0.0 <= min_opacity < 1.0:
            raise ValueError(f"min_opacity must be in [0, 1), got {min_opacity}")
        screen = -1
        if max_screen_size is not None:
            if isinstance(max_screen_size, bool) or not isinstance(max_screen_size, (int, float)):
                raise TypeError("max_screen_size must be a number or None")
            if not 0 <= max_screen_size < 2 ** 31:
                raise ValueError(f"max_screen_size must be in [0, 2^31), got {max_screen_size}")
            screen = int(math.floor(max_screen_size))      # radii are integers: r > s  <=>  r > floor(s)
        if noise is not None:
            check_noise(noise, n, n_split)
            on_rocm(noise=noise)
            if noise.device != dev:
                raise ValueError(f"noise is on {noise.device}, the parameters on {dev}")
            noise = noise.contiguous()
        else:
            noise = torch.randn((n, n_split, 3), dtype=torch.float32, device=dev, generator=generator)
        pos, (n_a, n_b, n_c, n_after) = self._classify(None, float(max_grad), float(min_opacity), float(extent), screen, n_split)
        self._emit(pos, n_after, n_split, noise, carry_stats=False)
        return DensifyReport(n_cloned=n_b, n_split=n_c, n_pruned=n - n_a - n_c, n_before=n, n_after=n_after)

    def prune(self, mask):
        """Removes the rows where mask (bool [N]) is True.  Survivors carry their moments and their statistics."""
        opt = self.optimizer
        n = opt.num_rows
        check_mask(mask, n)
        on_rocm(mask=mask)
        if mask.device != opt.device:
            raise ValueError(f"mask is on {mask.device}, the parameters on {opt.device}")
        pos, (n_a, _, _, n_after) = self._classify(mask.contiguous(), 0.0, 0.0, 1.0, -1, 1)
        self._emit(pos, n_after, 1, None, carry_stats=True)
        return DensifyReport(n_cloned=0, n_split=0, n_pruned=n - n_a, n_before=n, n_after=n_after)

    def reset_opacity(self, max_opacity=0.01):
        """opacity = min(opacity, float32(logit(max_opacity))), in place; the opacity group's moments become zero."""
        if isinstance(max_opacity, bool) or not isinstance(max_opacity, (int, float)):
            raise TypeError("max_opacity must be a number")
        if not 0.0 < max_opacity < 1.0:
            raise ValueError(f"max_opacity must be in (0, 1), got {max_opacity}")
        opt = self.optimizer
        p = opt.params["opacity"]
        cap = torch.tensor(math.log(max_opacity / (1.0 - max_opacity)), dtype=torch.float32, device=p.device)
        with torch.no_grad():
            torch.minimum(p, cap, out=p)
        opt.exp_avg["opacity"].zero_()
        opt.exp_avg_sq["opacity"].zero_()
