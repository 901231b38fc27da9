"""Helpers for the -m gpu parity tests: call the C ABI with torch device tensors."""
import contextlib
import os
import sys

import torch

from calipsync_amd import _lib


def kernel_table():
    """tools/kernel_resources.py's table of the built library's kernels, keyed by the short name a profiled row carries
    (tools/kernel_names.py); None where the LLVM binutils of the ROCm image are missing."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources
    return kernel_resources.table() if kernel_resources.tools_available() else None


def dev():
    return torch.device("cuda:0")


def ptr(t):
    return 0 if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(status, what="op"):
    _lib.check(status, what)
    torch.cuda.synchronize()


def nhwc(t):     # NCHW torch tensor -> contiguous NHWC on the GPU
    return t.permute(0, 2, 3, 1).contiguous().to(dev())


def nchw(t):     # NHWC device tensor -> NCHW on the CPU
    return t.permute(0, 3, 1, 2).contiguous().cpu()


@contextlib.contextmanager
def launched():
    """Record the kernels this thread launches inside the block (casync_debug_launch_log): yields a set that holds their
    short names (the keys of tools/kernel_resources.table()) once the block has ended."""
    import ctypes
    lib = _lib.load()
    names = set()
    _lib.check(lib.casync_debug_launch_log(1), "casync_debug_launch_log")
    try:
        yield names
        buf = ctypes.create_string_buffer(1 << 16)
        _lib.check(lib.casync_debug_launched(buf, len(buf)), "casync_debug_launched")
        names.update(n for n in buf.value.decode().split("\n") if n)
    finally:
        lib.casync_debug_launch_log(0)


@contextlib.contextmanager
def options(target=None, **kv):
    """Set engine switches (casync_set_option) for the duration of a block and restore them: on a
    calipsync_amd.unet.Model, or on the process defaults used by the casync_op_* calls (target None)."""
    if target is None:
        old = {k: _lib.get_option(k) for k in kv}
        for k, v in kv.items():
            _lib.set_option(k, v)
        try:
            yield
        finally:
            for k, v in old.items():
                _lib.set_option(k, v)
    else:
        old = {k: target.get_option(k) for k in kv}
        for k, v in kv.items():
            target.set_option(k, v)
        try:
            yield
        finally:
            for k, v in old.items():
                target.set_option(k, v)
