"""CPU (-m "not gpu"): the one call path of the Python wrappers (gaustudio_amd/_abi.py) against a stand-in library whose
entry points record their arguments and return a canned status: argument order, marshalling by type, the 32-bit range
check and the status-to-exception mapping.  Needs neither the built library nor a device."""
import contextlib
import ctypes

import pytest
import torch

from gaustudio_amd import _C, _abi

STREAM = 0x5eed
DEV = torch.device("cpu")


class FakeLib:
    """lib().gsr_<anything>(*args): appends (name, args) to .calls and returns .status."""

    def __init__(self, status=0):
        self.status, self.calls = status, []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.status
        return entry


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_C, "lib", lambda: lib)
    monkeypatch.setattr(_C, "_stream", lambda device: ctypes.c_void_p(STREAM))
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    return lib


def sent(fake, *args, **kw):
    """The arguments the entry point received for call("gsr_x", DEV, *args, **kw), without the stream that ends them."""
    _abi.call("gsr_x", DEV, *args, **kw)
    name, got = fake.calls[-1]
    assert name == "gsr_x" and type(got[-1]) is ctypes.c_void_p and got[-1].value == STREAM
    return got[:-1]


def test_workspace_first_stream_last(fake):
    got = sent(fake, 7, workspace=True)
    assert len(got) == 3 and isinstance(got[0], ctypes._CFuncPtr) and got[1] is None
    assert type(got[2]) is ctypes.c_int and got[2].value == 7
    got = sent(fake, 7)
    assert len(got) == 1 and got[0].value == 7
    ws = _abi.Workspace(DEV)                                   # a workspace shared between the stages of a pipeline
    assert sent(fake, workspace=ws)[0] is ws.fn
    assert ws.fn(None, 0) == ws.bufs[0].data_ptr() and ws.bufs[0].numel() == 1 and ws.bufs[0].dtype == torch.uint8


def test_tensors_become_addresses(fake):
    t = torch.arange(4, dtype=torch.float32)
    none, empty, full = sent(fake, None, torch.zeros(0), t)
    for p in (none, empty, full):
        assert type(p) is ctypes.c_void_p
    assert not none.value and not empty.value                  # c_void_p(0).value is None
    assert full.value == t.data_ptr()


def test_integers_are_range_checked(fake):
    hi, lo, yes, no = sent(fake, 2 ** 31 - 1, -2 ** 31, True, False)
    for v, want in ((hi, 2 ** 31 - 1), (lo, -2 ** 31), (yes, 1), (no, 0)):
        assert type(v) is ctypes.c_int and v.value == want
    assert sent(fake, torch.Size([5, 3])[0])[0].value == 5     # what tensor.shape yields
    for pos, bad in enumerate((2 ** 31, -2 ** 31 - 1)):
        with pytest.raises(OverflowError, match=rf"gsr_x: argument {pos + 1} = {bad}\b") as e:
            _abi.call("gsr_x", DEV, *([0] * (pos + 1)), bad)
        assert "32-bit" in str(e.value)
    assert len(fake.calls) == 2                                 # nothing reached the library


def test_floats_must_be_explicit(fake):
    with pytest.raises(TypeError, match=r"gsr_x: argument 1 is a float.*c_float or c_double"):
        _abi.call("gsr_x", DEV, 3, 1.0)
    with pytest.raises(TypeError, match="argument 0 is a str"):
        _abi.call("gsr_x", DEV, "3")
    assert not fake.calls


def test_ctypes_pass_through(fake):
    big, f, d = ctypes.c_uint64(2 ** 40), ctypes.c_float(0.5), ctypes.c_double(0.25)
    arr, n = (ctypes.c_float * 3)(1, 2, 3), ctypes.c_int(0)
    ref = ctypes.byref(n)
    got = sent(fake, big, f, d, arr, ref, ctypes.c_longlong(-2 ** 40))
    assert got[0] is big and got[0].value == 2 ** 40 and type(got[0]) is ctypes.c_uint64
    assert got[1] is f and got[2] is d and got[3] is arr and got[4] is ref
    assert type(got[5]) is ctypes.c_longlong and got[5].value == -2 ** 40


def test_status_is_returned_or_raised(fake):
    assert _abi.call("gsr_x", DEV) == 0
    fake.status = 41
    assert _abi.call("gsr_x", DEV) == 41
    errors = {-2: "{what}: bad argument", -5: (KeyError, "no such {what}")}
    fake.status = -2
    with pytest.raises(ValueError, match=r"^gsr_x: bad argument$"):
        _abi.call("gsr_x", DEV, errors=errors)
    with pytest.raises(ValueError, match=r"^seeds: bad argument$"):
        _abi.call("gsr_x", DEV, errors=errors, what="seeds")
    fake.status = -5
    with pytest.raises(KeyError, match="no such gsr_x"):
        _abi.call("gsr_x", DEV, errors=errors)
    fake.status = -3
    with pytest.raises(RuntimeError, match=r"^seeds failed \(rc=-3\): d must be odd$"):
        _abi.call("gsr_x", DEV, errors=errors, what="seeds", hint=": d must be odd")
    with pytest.raises(RuntimeError, match=r"^gsr_x failed \(rc=-3\)$"):
        _abi.call("gsr_x", DEV)
    with pytest.raises(LookupError, match="rc -3 of FakeLib"):                     # _C.py: the library's own message
        _abi.call("gsr_x", DEV, errors=errors, fail=lambda lib, rc: LookupError(f"rc {rc} of {type(lib).__name__}"))


def test_device_checks():
    cpu = torch.zeros(2)
    for exc in (RuntimeError, ValueError):
        with pytest.raises(exc, match=r"^depth is on 'cpu': gaustudio_amd runs on ROCm devices only \(no CPU fallback\)$"):
            _abi.on_rocm(exc, mask=None, depth=cpu)
    with pytest.raises(RuntimeError, match="^pts is on 'cpu'"):
        _abi.on_rocm(pts=cpu)
    _abi.on_rocm(mask=None)
    _abi.on_rocm(ValueError)
    meta = torch.device("meta")
    _abi.same_device(cpu.device, a=cpu, b=None)
    with pytest.raises(ValueError, match=r"^normals is on cpu, the points on meta$"):
        _abi.same_device(meta, ref="the points", rgb=None, normals=cpu)
    with pytest.raises(RuntimeError, match=r"^image is on cpu, the mesh on meta$"):
        _abi.same_device(meta, RuntimeError, image=cpu)
