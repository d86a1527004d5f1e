"""ctypes binding of libgeoformer_hip.so (the C ABI declared in include/geoformer_hip.h).  Signatures, struct layouts
and constants are read from the headers (_abi.py), not restated here.

There is NO CPU fallback: if the library is missing or a call fails this module raises.
PyTorch is only used by callers for device memory and streams; pointers cross the boundary
as plain integers.
"""
from __future__ import annotations

import ctypes
import os

from . import _abi
from ._build import LIB_PATH

LIB_PATH = os.environ.get("GF_LIB_PATH", LIB_PATH)  # dev knob: load an experimental build of the library

_lib = None


class GeoFormerHipError(RuntimeError):
    pass


class _Handle(ctypes.CDLL):
    """The library's handle: an entry point gets its prototype from the headers (_abi.functions()) when it is first
    looked up, and is then an attribute of the handle like any ctypes function.  A process pays for the entry points
    it calls, not for every one the headers declare (about ten collector-tracked objects each).  The function object is
    put on the handle only AFTER its prototype is set: forwards run on several host threads, and a thread that finds the
    attribute another thread has just made must never call it without argtypes (ctypes would pass a pointer or a
    long long as a C int).  Two threads that look a name up at the same time each bind an object of their own; either
    may stay on the handle."""

    def __getattr__(self, name):
        if name.startswith("__") and name.endswith("__"):
            raise AttributeError(name)  # (as ctypes.CDLL.__getattr__ does)
        fn = self[name]  # a new function object, not yet visible to anyone; AttributeError for a missing export
        sig = _abi.functions().get(name)
        if sig is not None:
            fn.restype, fn.argtypes = sig
        setattr(self, name, fn)
        return fn


def _declare(lib):
    """Check that the library exports every prototype of the headers (_abi.functions()) -- AttributeError otherwise --
    without keeping a function object for any of them; returns that table.  _Handle binds them on first use."""
    sig = _abi.functions()
    for name in sig:
        lib[name]
    return sig


EXPORTS = None


def _check_hw_queues(torch):
    """The package asks the HIP runtime for HW_QUEUES_WANTED hardware queues (geoformer_amd/__init__.py).  The runtime
    reads GPU_MAX_HW_QUEUES once, at its first call: nothing can be fixed from here, so say so when the variable is unset."""
    import warnings

    from . import HW_QUEUES_MIN, HW_QUEUES_WANTED, hw_queues_setting

    have = hw_queues_setting()
    if have is not None and have >= HW_QUEUES_MIN:
        return
    up = torch.cuda.is_initialized()
    warnings.warn(
        f"geoformer_amd: GPU_MAX_HW_QUEUES is {'unset (runtime default 4)' if have is None else have}"
        + (" and the HIP runtime is already initialised" if up else "")
        + f": the runtime picks its own number of hardware queues.  Export GPU_MAX_HW_QUEUES="
        f"{HW_QUEUES_WANTED} or call geoformer_amd.configure_runtime() before the process's first HIP call"
        + (" (e.g. before torch.cuda.set_device in train.py / test.py)." if up else "."),
        RuntimeWarning, stacklevel=3)


def load():
    """Load the shared library (after ``import torch`` so both share one HIP runtime)."""
    global _lib, EXPORTS
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GeoFormerHipError(
            f"{LIB_PATH} is missing: build it with `python -m geoformer_amd._build` "
            "(or __graft_entry__.build()).  There is no CPU fallback for the HIP operators."
        )
    import torch  # noqa: F401  (loads libamdhip64 first; our library binds to the same SONAME)

    _check_hw_queues(torch)
    lib = _Handle(LIB_PATH)
    EXPORTS = _declare(lib)
    if lib.gf_abi_version() != _abi.const("GF_ABI_VERSION"):
        raise GeoFormerHipError("libgeoformer_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(status: int, what: str = ""):
    if status != 0:
        msg = load().gf_last_error()
        raise GeoFormerHipError(f"{what} failed ({status}): {msg.decode() if msg else ''}")


FEEDER_MAX_COPIES = _abi.const("GF_FEEDER_MAX_COPIES")
FeederJob = _abi.struct("GfFeederJob")
AugBatch = _abi.struct("GfAugBatch")  # device pointers of one training batch's augmentation


# seconds the host has spent blocked in the package's own Python-level waits (per process; bench.py's host_busy figure)
host_wait_s = [0.0]


def timed_wait(event):
    """event.synchronize() with its wall time added to host_wait_s."""
    import time

    t = time.perf_counter()
    event.synchronize()
    host_wait_s[0] += time.perf_counter() - t


def ptr(t):
    """Device (or host) address of a tensor as a plain int (ctypes converts it for a c_void_p argtype), None -> NULL."""
    return None if t is None else t.data_ptr()


_raw_stream = None


def stream_ptr():
    """hipStream_t of PyTorch's current stream on the current device (plain int)."""
    global _raw_stream
    import torch

    if _raw_stream is None:
        _raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", False)
    if _raw_stream:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream
