"""Scaffold-GS anchor control on the GPU (csrc/gsr_anchor.hip): the statistics of a training view, anchor growing by voxel
level and pruning, as one compaction that carries the moments of a torch.optim.Adam.

    params = dict(anchor=[N,3], anchor_feat=[N,32], offset=[N,k,3], scale_raw=[N,6], rot_raw=[N,4])   # float32 leaves
    ac = AnchorControl(params, voxel_size, optimizer=adam)
    out = render_scaffold(ScaffoldModel.from_raw(**params, ...), rs, backward="hip");  loss.backward()
    ac.accumulate(out["gaussians"], out["viewspace_points"].grad, out["radii"])
    report = ac.adjust(check_interval=100, success_threshold=0.8, grad_threshold=2e-4, min_opacity=0.005)

After adjust, params[...] are new leaf tensors (survivors in their order, then the new anchors of level 0, level 1, ...), the
optimiser's groups point at them, survivors keep exp_avg / exp_avg_sq and new rows start at zero; the old tensors are left as
they were.  Contract, float order included: INTEGRATION.md s23b; to the bit: tests/anchor_model.py.  There is no CPU fallback.
"""
import ctypes
import math
from collections import namedtuple

import torch

from ._abi import Workspace, call, on_rocm

NAMES = ("anchor", "anchor_feat", "offset", "scale_raw", "rot_raw")
FEAT_DIM = 32
MAX_OFFSETS = 16
MAX_ANCHORS = 2 ** 24
SLOT_LIMIT = 2 ** 31
MAX_LEVELS = 8                          # GSR_ANCHOR_MAX_LEVELS
_SLOT_STAT, _ANCHOR_STAT = 1, 2         # GSR_ANCHOR_SLOT_STAT / _ANCHOR_STAT

AnchorReport = namedtuple("AnchorReport", "n_grown n_pruned n_before n_after")

_ERRORS = {-2: "{what}: the library rejected the arguments (sizes, a missing tensor)",
           -4: (MemoryError, "{what}: the workspace allocation failed"),
           -7: "{what}: a growing candidate's position is not finite or its voxel cell is outside [-2^20, 2^20): nothing was changed"}


class _Cells(ctypes.Structure):         # include/gsrast.h gsr_anchor_cells
    _fields_ = [("cells", ctypes.c_void_p), ("count", ctypes.c_int), ("cur", ctypes.c_float)]


class _Tensor(ctypes.Structure):        # include/gsrast.h gsr_anchor_tensor
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("width", ctypes.c_int), ("kind", ctypes.c_int)]


def _f32(x):
    return ctypes.c_float(x).value


def _tail(name, k):
    return dict(anchor=(3,), anchor_feat=(FEAT_DIM,), offset=(k, 3), scale_raw=(6,), rot_raw=(4,))[name]


def check_limits(n, k, what="the model"):
    """N <= 2^24 and N k < 2^31: the limits of decode and of every kernel here."""
    if n > MAX_ANCHORS or n * k >= SLOT_LIMIT:
        raise ValueError(f"{what} has {n} anchors of {k} offsets: at most 2^24 anchors and fewer than 2^31 offsets")


def check_params_host(params):
    """Types and keys, shapes, dtypes, limits, contiguity and leafness: everything that needs no device.  Returns (N, k)."""
    if not isinstance(params, dict):
        raise TypeError("params must be a dict of the five anchor tensors")
    for name in NAMES:
        if name not in params:
            raise KeyError(f"params has no '{name}' (it needs {', '.join(NAMES)})")
    extra = [key for key in params if key not in NAMES]
    if extra:
        raise KeyError(f"params has unknown entries {extra}")
    for name in NAMES:
        if not torch.is_tensor(params[name]):
            raise TypeError(f"params['{name}'] must be a torch tensor")
    anchor, offset = params["anchor"], params["offset"]
    if anchor.dim() != 2 or anchor.shape[1] != 3:
        raise ValueError(f"anchor must have shape [N, 3], got {list(anchor.shape)}")
    n = int(anchor.shape[0])
    if offset.dim() != 3 or offset.shape[2] != 3 or not 1 <= int(offset.shape[1]) <= MAX_OFFSETS:
        raise ValueError(f"offset must have shape [N, k, 3] with 1 <= k <= {MAX_OFFSETS}, got {list(offset.shape)}")
    k = int(offset.shape[1])
    for name in NAMES:
        want = (n,) + _tail(name, k)
        if tuple(params[name].shape) != want:
            raise ValueError(f"{name} must have shape {list(want)} (N = {n} rows like anchor), got {list(params[name].shape)}")
    for name in NAMES:
        if params[name].dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {params[name].dtype}")
    check_limits(n, k)
    for name in NAMES:
        t = params[name]
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if not t.is_leaf:
            raise ValueError(f"{name} must be a leaf tensor")
    return n, k


def check_params_device(params):
    on_rocm(**{name: params[name] for name in NAMES})
    dev = params["anchor"].device
    for name in NAMES:
        if params[name].device != dev:
            raise ValueError(f"{name} is on {params[name].device}, anchor on {dev}")
    return dev


def check_optimizer(optimizer, params):
    """None, or a torch.optim.Adam whose groups hold the five leaves (each once).  Returns name -> (group, index)."""
    if optimizer is None:
        return {}
    if not isinstance(optimizer, torch.optim.Adam):
        raise TypeError(f"optimizer must be a torch.optim.Adam or None, got {type(optimizer).__name__}")
    where = {}
    for group in optimizer.param_groups:
        for idx, p in enumerate(group["params"]):
            for name in NAMES:
                if p is params[name]:
                    if name in where:
                        raise ValueError(f"the optimizer holds {name} twice")
                    where[name] = (group, idx)
                    if group.get("amsgrad", False):
                        raise ValueError(f"the optimizer's group of {name} uses amsgrad: its third moment is not carried")
    for name in NAMES:
        if name not in where:
            raise ValueError(f"the optimizer has no param group that holds params['{name}']")
    return where


def _number(name, v, integer=False):
    if isinstance(v, bool) or not isinstance(v, int if integer else (int, float)):
        raise TypeError(f"{name} must be {'an integer' if integer else 'a number'}")
    return v


def level_plan(voxel_size, grad_threshold, update_depth, update_init_factor, update_hierarchy_factor):
    """[(cur_i, t_i, rand_min_i)] of the levels, each float32 as the kernels take it."""
    plan = []
    for i in range(update_depth):
        size_factor = update_init_factor // (update_hierarchy_factor ** i)
        if size_factor < 1:
            raise ValueError(f"level {i}: update_init_factor // update_hierarchy_factor^{i} is 0: no voxel size")
        cur = _f32(voxel_size * size_factor)
        if not (math.isfinite(cur) and cur > 0.0):
            raise ValueError(f"level {i}: the voxel size {cur} is not a positive float32")
        plan.append((cur, _f32(grad_threshold * (update_hierarchy_factor // 2) ** i), 0.5 ** (i + 1)))
    return plan


class AnchorControl:
    """Statistics: offset_grad_accum float32 [N k], offset_denom int32 [N k], opacity_accum float32 [N], anchor_denom int32 [N]."""

    def __init__(self, params, voxel_size, optimizer=None, update_depth=3, update_init_factor=16, update_hierarchy_factor=4):
        _number("voxel_size", voxel_size)
        for name, v in (("update_depth", update_depth), ("update_init_factor", update_init_factor),
                        ("update_hierarchy_factor", update_hierarchy_factor)):
            _number(name, v, integer=True)
        if optimizer is not None and not isinstance(optimizer, torch.optim.Adam):
            raise TypeError(f"optimizer must be a torch.optim.Adam or None, got {type(optimizer).__name__}")
        n, k = check_params_host(params)
        if not (math.isfinite(voxel_size) and voxel_size > 0):
            raise ValueError(f"voxel_size must be positive, got {voxel_size}")
        if not 1 <= update_depth <= MAX_LEVELS:
            raise ValueError(f"update_depth must be in [1, {MAX_LEVELS}], got {update_depth}")
        if update_init_factor < 1 or update_hierarchy_factor < 1:
            raise ValueError("update_init_factor and update_hierarchy_factor must be >= 1")
        level_plan(voxel_size, 0.0, update_depth, update_init_factor, update_hierarchy_factor)
        check_optimizer(optimizer, params)
        dev = check_params_device(params)
        self.params, self.optimizer = params, optimizer
        self.voxel_size = float(voxel_size)
        self.update_depth, self.update_init_factor = update_depth, update_init_factor
        self.update_hierarchy_factor = update_hierarchy_factor
        self.num_anchors, self.n_offsets = n, k
        self._zero_stats(n, k, dev)

    @property
    def device(self):
        return self.params["anchor"].device

    def _zero_stats(self, n, k, dev):
        self.offset_grad_accum = torch.zeros(n * k, dtype=torch.float32, device=dev)
        self.offset_denom = torch.zeros(n * k, dtype=torch.int32, device=dev)
        self.opacity_accum = torch.zeros(n, dtype=torch.float32, device=dev)
        self.anchor_denom = torch.zeros(n, dtype=torch.int32, device=dev)

    def _stats(self):
        return (("offset_grad_accum", self.offset_grad_accum, self.n_offsets, _SLOT_STAT),
                ("offset_denom", self.offset_denom, self.n_offsets, _SLOT_STAT),
                ("opacity_accum", self.opacity_accum, 1, _ANCHOR_STAT), ("anchor_denom", self.anchor_denom, 1, _ANCHOR_STAT))

    # ------------------------------------------------------------------------------------------------------ statistics
    def accumulate(self, gaussians, viewspace_grad, radii):
        """One launch, no atomics.  gaussians: the ScaffoldGaussians of the view (either `backward` mode); viewspace_grad
        float32 [M,3] (the .grad of out["viewspace_points"]); radii int32 [M].  A Gaussian with radii > 0 adds
        sqrt(gx gx + gy gy) and 1 to its slot anchor_index k + offset_index; a visible anchor adds 1 to anchor_denom and the
        float32 sum of its kept Gaussians' opacities, in offset order, to opacity_accum."""
        n, k = self.num_anchors, self.n_offsets
        for f in ("anchor_index", "offset_index", "opacity", "visible"):
            if not torch.is_tensor(getattr(gaussians, f, None)):
                raise TypeError(f"gaussians must be the ScaffoldGaussians of a decode (it has no tensor {f})")
        for name, t in (("viewspace_grad", viewspace_grad), ("radii", radii)):
            if not torch.is_tensor(t):
                raise TypeError(f"{name} must be a torch tensor")
        aidx, oidx, opacity, visible = gaussians.anchor_index, gaussians.offset_index, gaussians.opacity, gaussians.visible
        m = int(aidx.shape[0]) if aidx.dim() == 1 else -1
        for name, t, shape, dt in (("anchor_index", aidx, (m,), torch.int32), ("offset_index", oidx, (m,), torch.int32),
                                   ("opacity", opacity, (m, 1), torch.float32), ("visible", visible, (n,), torch.bool),
                                   ("viewspace_grad", viewspace_grad, (m, 3), torch.float32), ("radii", radii, (m,), torch.int32)):
            if m < 0 or tuple(t.shape) != shape:
                raise ValueError(f"{name} must have shape {list(shape)}, got {list(t.shape)}")
            if t.dtype != dt:
                raise TypeError(f"{name} must be {dt}, got {t.dtype}")
        if m > n * k:
            raise ValueError(f"{m} Gaussians from {n} anchors of {k} offsets")
        ts = dict(anchor_index=aidx, offset_index=oidx, opacity=opacity, visible=visible, viewspace_grad=viewspace_grad, radii=radii)
        on_rocm(**ts)
        dev = self.device
        for name, t in ts.items():
            if t.device != dev:
                raise ValueError(f"{name} is on {t.device}, the anchors on {dev}")
        ready = {name: t.detach().contiguous() for name, t in ts.items()}
        call("gsr_anchor_accumulate", dev, n, k, m, ready["anchor_index"], ready["offset_index"], ready["opacity"],
             ready["viewspace_grad"], ready["radii"], ready["visible"].view(torch.uint8), self.offset_grad_accum, self.offset_denom,
             self.opacity_accum, self.anchor_denom, what="AnchorControl.accumulate", errors=_ERRORS)

    # ------------------------------------------------------------------------------------------------------ the pass
    def _moments(self, where):
        """name -> (exp_avg, exp_avg_sq) of the leaves the optimiser has already stepped."""
        out = {}
        for name in where:
            p = self.params[name]
            st = self.optimizer.state.get(p)
            if not st or "exp_avg" not in st:
                continue
            for key in ("exp_avg", "exp_avg_sq"):
                t = st[key]
                if t.dtype != torch.float32 or tuple(t.shape) != tuple(p.shape) or t.device != p.device or not t.is_contiguous():
                    raise ValueError(f"the optimizer's {key} of {name} must be a contiguous float32 {list(p.shape)} on {p.device}")
            out[name] = (st["exp_avg"], st["exp_avg_sq"])
        return out

    def adjust(self, check_interval=100, success_threshold=0.8, grad_threshold=2e-4, min_opacity=0.005, rand=None, generator=None):
        """One pass of growing and pruning.  Returns AnchorReport(n_grown per level, n_pruned, n_before,
        n_after).  rand: float32 [update_depth, N k] in [0, 1), the draw that thins the candidates of level i to those with
        rand[i] > 0.5^(i+1); None draws torch.rand with `generator`.  Level i > 0 runs only when an earlier level of this pass
        added an anchor (the published behaviour).  On an error nothing has been changed."""
        for name, v in (("check_interval", check_interval), ("success_threshold", success_threshold),
                        ("grad_threshold", grad_threshold), ("min_opacity", min_opacity)):
            _number(name, v)
        if rand is not None and not torch.is_tensor(rand):
            raise TypeError("rand must be a torch tensor or None")
        n, k = check_params_host(self.params)
        if (n, k) != (self.num_anchors, self.n_offsets):
            raise ValueError(f"params changed shape behind AnchorControl: {n} x {k}, the statistics are {self.num_anchors} x {self.n_offsets}")
        for name, v in (("check_interval", check_interval), ("success_threshold", success_threshold)):
            if not (math.isfinite(v) and v >= 0):
                raise ValueError(f"{name} must be finite and >= 0, got {v}")
        if math.isnan(grad_threshold) or math.isnan(min_opacity):
            raise ValueError("grad_threshold and min_opacity must not be NaN")
        mature_min = int(math.floor(check_interval * success_threshold * 0.5))
        settled_min = int(math.floor(check_interval * success_threshold))
        if settled_min >= 2 ** 31:
            raise ValueError("check_interval * success_threshold must stay below 2^31")
        plan = level_plan(self.voxel_size, grad_threshold, self.update_depth, self.update_init_factor, self.update_hierarchy_factor)
        if rand is not None:
            if tuple(rand.shape) != (self.update_depth, n * k):
                raise ValueError(f"rand must have shape [{self.update_depth}, {n * k}], got {list(rand.shape)}")
            if rand.dtype != torch.float32:
                raise TypeError(f"rand must be float32, got {rand.dtype}")
        where = check_optimizer(self.optimizer, self.params)
        dev = check_params_device(self.params)
        if rand is not None:
            on_rocm(rand=rand)
            if rand.device != dev:
                raise ValueError(f"rand is on {rand.device}, the anchors on {dev}")
            rand = rand.contiguous()
        else:
            rand = torch.rand((self.update_depth, n * k), dtype=torch.float32, device=dev, generator=generator)
        moments = self._moments(where)
        src = {name: self.params[name].detach() for name in NAMES}

        # the levels: cell lists and per-cell maximum features in workspace blocks, nothing of the model is written
        levels = (_Cells * MAX_LEVELS)()
        feats = (ctypes.c_void_p * MAX_LEVELS)()
        keep, grown = [], []
        for i, (cur, t_i, rand_min) in enumerate(plan):
            if n == 0 or (i > 0 and sum(grown) == 0):
                grown.append(0)
                continue
            ws = Workspace(dev)
            cells_p, feat_p, info = ctypes.c_void_p(), ctypes.c_void_p(), (ctypes.c_longlong * 2)()
            num_prior = len(keep)
            call("gsr_anchor_level", dev, n, k, src["anchor"], src["offset"], src["scale_raw"], src["anchor_feat"],
                 self.offset_grad_accum, self.offset_denom, rand[i], mature_min, ctypes.c_float(t_i), ctypes.c_float(rand_min),
                 ctypes.c_float(cur), levels, num_prior, ctypes.byref(cells_p), ctypes.byref(feat_p), info, workspace=ws,
                 what="AnchorControl.adjust", errors=_ERRORS)
            count = int(info[1])
            grown.append(count)
            if count > 0:
                keep.append(ws.bufs[-1])                     # the level's block: cells, then features
                levels[num_prior].cells, levels[num_prior].count, levels[num_prior].cur = cells_p.value, count, cur
                feats[num_prior] = feat_p.value
            check_limits(n + sum(grown), k, "the model with the anchors grown so far")

        # the prune decision on the anchors that existed before the pass
        pos = torch.empty(n + 1, dtype=torch.int32, device=dev)
        survivors = ctypes.c_int(0)
        call("gsr_anchor_prune", dev, n, self.opacity_accum, self.anchor_denom, settled_min, ctypes.c_float(min_opacity), pos,
             ctypes.byref(survivors), workspace=True, what="AnchorControl.adjust", errors=_ERRORS)
        n_after = int(survivors.value) + sum(grown)
        check_limits(n_after, k, "the model after this pass")

        # the one write of every output tensor
        new_p = {name: torch.empty((n_after,) + _tail(name, k), dtype=torch.float32, device=dev) for name in NAMES}
        new_m = {name: tuple(torch.empty_like(new_p[name]) for _ in range(2)) for name in moments}
        old_stats = self._stats()
        new_stats = [torch.empty(n_after * w, dtype=t.dtype, device=dev) for _, t, w, _ in old_stats]
        width = {name: math.prod(_tail(name, k)) for name in NAMES}
        pairs = [(src[name], new_p[name], width[name], 0) for name in NAMES]
        for name in moments:
            pairs += [(moments[name][j], new_m[name][j], width[name], 0) for j in range(2)]
        pairs += [(t, d, w, kind) for (_, t, w, kind), d in zip(old_stats, new_stats)]
        arr = (_Tensor * len(pairs))()
        for g, (s, d, w, kind) in zip(arr, pairs):
            g.src = s.data_ptr() if s.numel() else None
            g.dst = d.data_ptr() if d.numel() else None
            g.width, g.kind = w, kind
        if n_after > 0:
            call("gsr_anchor_emit", dev, n, k, arr, len(pairs), pos, self.offset_denom, self.anchor_denom, mature_min, settled_min,
                 levels, feats, len(keep), what="AnchorControl.adjust", errors=_ERRORS)

        for name in NAMES:
            old, new = self.params[name], new_p[name].requires_grad_(True)
            self.params[name] = new
            if name in where:
                group, idx = where[name]
                group["params"][idx] = new
                state = self.optimizer.state.pop(old, None)
                if state is not None:
                    state = dict(state)
                    if name in new_m:
                        state["exp_avg"], state["exp_avg_sq"] = new_m[name]
                    self.optimizer.state[new] = state
        self.offset_grad_accum, self.offset_denom, self.opacity_accum, self.anchor_denom = new_stats
        self.num_anchors = n_after
        return AnchorReport(n_grown=tuple(grown), n_pruned=n - int(survivors.value), n_before=n, n_after=n_after)
