"""The one call path from the Python wrappers into the C ABI of libgsrast.so (include/gsrast.h), and the argument checks the
wrappers share.  Host Python only.

    rc = call("gsr_knn", dev, pts, n, q, nq, k, dist2, idx, workspace=True, what="knn", errors=_ERRORS)

call() enters the device, passes the allocator callback first when asked to, marshals the arguments BY PYTHON TYPE, appends
the device's current stream, and turns a negative status into an exception.  No entry point declares argtypes; the marshaller
is the range check: a tensor or None becomes its address (NULL for None and for an empty tensor), a ctypes instance, array,
structure or byref() passes through, a bool or integer becomes c_int after a check against [-2^31, 2^31), anything else --
a Python float first of all, since the ABI mixes float and double -- is a TypeError.  The few 64-bit by-value arguments are
explicit c_uint64 / c_longlong at their call sites.
"""
import ctypes
import operator

import torch

from . import _C

_ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
_PASS = (ctypes._SimpleCData, ctypes.Array, ctypes.Structure, ctypes._Pointer, type(ctypes.byref(ctypes.c_int())))


class Workspace:
    """gsr_alloc_fn for the duration of one call: hands out torch uint8 tensors (stream-ordered through torch's caching
    allocator) and keeps them alive until the call has been enqueued."""

    def __init__(self, device):
        self.device = device
        self.bufs = []
        self.fn = _ALLOC_FN(self._alloc)

    def _alloc(self, ctx, nbytes):
        t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=self.device)
        self.bufs.append(t)
        return t.data_ptr()


def _marshal(name, pos, a):
    if a is None or isinstance(a, torch.Tensor):
        return _C._ptr(a)
    if isinstance(a, _PASS):
        return a
    try:
        v = operator.index(a)
    except TypeError:
        raise TypeError(f"{name}: argument {pos} is a {type(a).__name__}, not an integer (say c_float or c_double)") from None
    if not -2 ** 31 <= v < 2 ** 31:
        raise OverflowError(f"{name}: argument {pos} = {v} does not fit a 32-bit int")
    return ctypes.c_int(v)


def raise_status(rc, what, errors=None, hint=""):
    """The exception of a negative status: errors[rc] = (ExceptionType, message) or a message (ValueError), "{what}" in it
    replaced; RuntimeError otherwise."""
    e = (errors or {}).get(rc)
    if e is None:
        raise RuntimeError(f"{what} failed (rc={rc}){hint}")
    exc, msg = e if isinstance(e, tuple) else (ValueError, e)
    raise exc(msg.replace("{what}", what))


def call(name, device, *args, workspace=False, what=None, errors=None, hint="", fail=None):
    """lib().<name>([alloc, NULL,] *args, stream of `device`) on `device`; returns the status when it is >= 0.  workspace: True
    for a Workspace of this call's own, or one to share between the stages of a pipeline.  fail(lib, rc) -> exception replaces
    the errors / what / hint mapping (_C.py: the text of gsr_last_error)."""
    L = _C.lib()
    fn = getattr(L, name)
    ws = Workspace(device) if workspace is True else (workspace or None)      # alive until fn has returned
    argv = [_marshal(name, pos, a) for pos, a in enumerate(args)]
    with torch.cuda.device(device):
        rc = fn(*((ws.fn, None) if ws else ()), *argv, _C._stream(device))
    if rc >= 0:
        return rc
    if fail is not None:
        raise fail(L, rc)
    raise_status(rc, what or name, errors, hint)


# ------------------------------------------------------------------------------------------------------ argument checks
def on_rocm(exc=RuntimeError, **tensors):
    """Checked after shapes and dtypes, so that those errors need no device."""
    for name, t in tensors.items():
        if t is not None and t.device.type != "cuda":
            raise exc(f"{name} is on '{t.device}': gaustudio_amd runs on ROCm devices only (no CPU fallback)")


def same_device(dev, exc=ValueError, ref="the mesh", **tensors):
    for name, t in tensors.items():
        if t is not None and t.device != dev:
            raise exc(f"{name} is on {t.device}, {ref} on {dev}")


def check_mesh(vertices, faces, vertex_colors=None, *, vertex_dtypes, max_verts, max_faces, device_exc):
    """vertices [V,3] (None: faces alone), faces [F,3] int32 / int64, vertex_colors [V,3] float32 or None.  Types, shapes,
    dtypes and sizes first, then the devices, then -- the one check that reads the device -- the range of int64 indices.
    vertex_dtypes: the dtypes taken, or None for any; max_verts, max_faces: (exclusive limit, message)."""
    for name, t in (("vertices", vertices), ("faces", faces)):
        if not torch.is_tensor(t) and not (t is None and name == "vertices"):
            raise TypeError(f"{name} must be a torch tensor")
    if vertices is not None and (vertices.dim() != 2 or vertices.shape[1] != 3):
        raise ValueError(f"vertices must have shape [V, 3], got {list(vertices.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must have shape [F, 3], got {list(faces.shape)}")
    if vertices is not None and vertex_dtypes is not None and vertices.dtype not in vertex_dtypes:
        raise TypeError(f"vertices must be one of {[str(d) for d in vertex_dtypes]}, got {vertices.dtype}")
    if faces.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"faces must be int32 or int64, got {faces.dtype}")
    for t, (limit, msg) in ((vertices, max_verts), (faces, max_faces)):
        if t is not None and t.shape[0] >= limit:
            raise ValueError(msg)
    if vertex_colors is not None:
        if not torch.is_tensor(vertex_colors):
            raise TypeError("vertex_colors must be a torch tensor or None")
        if vertex_colors.dtype != torch.float32:
            raise TypeError(f"vertex_colors must be float32, got {vertex_colors.dtype}")
        if tuple(vertex_colors.shape) != tuple(vertices.shape):
            raise ValueError(f"vertex_colors must have shape {list(vertices.shape)} like vertices, got {list(vertex_colors.shape)}")
    on_rocm(device_exc, vertices=vertices, faces=faces, vertex_colors=vertex_colors)
    if faces.dtype == torch.int64 and faces.numel():
        lo, hi = int(faces.min()), int(faces.max())
        if lo < -2 ** 31 or hi >= 2 ** 31:
            raise ValueError("face indices out of range")
