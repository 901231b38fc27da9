"""-m gpu: the weight ownership the HuBERT, PFLD and S3FD handles share (csrc/handle.h PackedWeights), on the smallest input
each network takes: a host load against an adopted device buffer, reloads (the bf16 image and the owned copy follow), an
adopted handle that turns to a copy of its own, and the three refusals in front of any launch.  Outputs are compared with
torch.equal: the same kernels on the same bits.  The refusal of a buffer on another device needs two GPUs in one process
and is not run here."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hubert_ref
from calipsync_amd import _lib, facedet, hubert, landmarks, recipe
from gpu_util import launched, stream

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SAMPLES = 400      # one HuBERT token
SIDE = 64          # the smallest S3FD frame the suite runs


class Hubert:
    prefix = "hubert"

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def state_dict():
        return hubert_ref.recipe_state_dict(2)

    @classmethod
    @functools.lru_cache(maxsize=None)
    def packed(cls):
        return hubert.pack(cls.state_dict(), 2)

    @classmethod
    def engine(cls, precision):
        return hubert.HubertEngine(cls.state_dict(), 2, DEV, precision)

    @staticmethod
    def create(lib, precision, h):
        return lib.casync_hubert_create_ex(0, 2, hubert.PRECISIONS[precision], C.byref(h))

    @staticmethod
    def input():
        return torch.from_numpy(recipe.normal01(7, 11, SAMPLES).astype(np.float32)).to(DEV)

    @staticmethod
    def forward(lib, precision, h, x):
        need = max(lib.casync_hubert_workspace_bytes(1, SAMPLES), lib.casync_hubert_workspace_bytes_h(h, 1, SAMPLES))
        ws = torch.empty(need // 4 + 1, dtype=torch.float32, device=DEV)
        out = torch.zeros(1, 1, 1024, dtype=torch.float32, device=DEV)
        return lib.casync_hubert_forward(h, x.data_ptr(), 1, SAMPLES, out.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream()), out


class Pfld:
    prefix = "pfld"

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def packed():
        return landmarks.pack(recipe.make_pfld_state_dict())

    @staticmethod
    def engine(precision):
        return landmarks.PFLDEngine(recipe.make_pfld_state_dict(), DEV)

    @staticmethod
    def create(lib, precision, h):
        return lib.casync_pfld_create(0, C.byref(h))

    @staticmethod
    def input():
        return torch.from_numpy(recipe.make_pfld_inputs(1)).to(DEV)

    @staticmethod
    def forward(lib, precision, h, x):
        ws = torch.empty(lib.casync_pfld_workspace_bytes(1) // 4 + 1, dtype=torch.float32, device=DEV)
        out = torch.zeros(1, 220, dtype=torch.float32, device=DEV)
        return lib.casync_pfld_forward_u8(h, x.data_ptr(), 1, out.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream()), out


class S3fd:
    prefix = "s3fd"

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def packed():
        return facedet.pack(recipe.make_s3fd_state_dict())

    @staticmethod
    def engine(precision):
        return facedet.S3FDEngine(recipe.make_s3fd_state_dict(), DEV, precision)

    @staticmethod
    def create(lib, precision, h):
        return lib.casync_s3fd_create_ex(0, facedet.PRECISIONS[precision], C.byref(h))

    @staticmethod
    def input():
        return torch.from_numpy(recipe.make_s3fd_inputs(1, SIDE, SIDE)).to(DEV)

    @staticmethod
    def forward(lib, precision, h, x):
        need = lib.casync_s3fd_workspace_bytes_ex(facedet.PRECISIONS[precision], 1, SIDE, SIDE)
        ws = torch.empty(need // 4 + 1, dtype=torch.float32, device=DEV)
        out = torch.zeros(1, lib.casync_s3fd_priors(SIDE, SIDE), 5, dtype=torch.float32, device=DEV)
        return lib.casync_s3fd_forward_u8(h, x.data_ptr(), 1, SIDE, SIDE, out.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream()), out


CASES = [(Hubert, "fp32"), (Hubert, "bf16"), (Pfld, "fp32"), (S3fd, "fp32"), (S3fd, "bf16")]
IDS = [f"{k.prefix}-{p}" for k, p in CASES]


def _run(lib, kind, precision, h, x):
    st, out = kind.forward(lib, precision, h, x)
    _lib.check(st, f"casync_{kind.prefix}_forward")
    torch.cuda.synchronize()
    return out


def _refused(lib, status, words):
    assert status < 0, status
    msg = lib.casync_last_error().decode()
    assert words in msg, msg


@pytest.mark.parametrize("kind,precision", CASES, ids=IDS)
def test_host_load_adopted_buffer_reloads_and_refusals(kind, precision):
    lib = _lib.load()
    load_host = getattr(lib, f"casync_{kind.prefix}_load_weights_host")
    load_device = getattr(lib, f"casync_{kind.prefix}_load_weights_device")
    destroy = getattr(lib, f"casync_{kind.prefix}_destroy")
    buf = kind.packed()
    half = buf * np.float32(0.5)
    x = kind.input()
    a = kind.engine(precision)                 # the normal way: a host load
    b, fresh = C.c_void_p(), C.c_void_p()
    try:
        first = _run(lib, kind, precision, a._h, x)
        assert first.abs().max() > 0 and torch.isfinite(first).all()

        # host load against device adopt
        _lib.check(kind.create(lib, precision, b), f"casync_{kind.prefix}_create")
        adopted = torch.from_numpy(buf).to(DEV)
        assert adopted.data_ptr() % 256 == 0
        _lib.check(load_device(b, adopted.data_ptr(), adopted.numel()), f"casync_{kind.prefix}_load_weights_device")
        assert torch.equal(_run(lib, kind, precision, b, x), first)

        # a reload refreshes everything the forward reads
        _lib.check(load_host(a._h, half.ctypes.data, half.size), f"casync_{kind.prefix}_load_weights_host")
        assert not torch.equal(_run(lib, kind, precision, a._h, x), first)
        _lib.check(load_host(a._h, buf.ctypes.data, buf.size), f"casync_{kind.prefix}_load_weights_host")
        assert torch.equal(_run(lib, kind, precision, a._h, x), first)

        # adopted to owned: the buffer the handle adopted goes away (its memory is handed out again and overwritten)
        _lib.check(load_host(b, buf.ctypes.data, buf.size), f"casync_{kind.prefix}_load_weights_host")
        n = adopted.numel()
        del adopted
        scribble = torch.full((n,), 3.0, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        assert torch.equal(_run(lib, kind, precision, b, x), first)
        del scribble

        # refusals, each in front of any launch
        _lib.check(kind.create(lib, precision, fresh), f"casync_{kind.prefix}_create")
        on_device = torch.from_numpy(buf).to(DEV)
        total = buf.size
        with launched() as kernels:
            _refused(lib, load_host(b, buf.ctypes.data, total - 1), "layout needs")
            _refused(lib, load_device(b, on_device.data_ptr(), total - 1), "layout needs")
            _refused(lib, load_device(b, on_device.data_ptr() + 4, total), "256-B aligned")
            st, _ = kind.forward(lib, precision, fresh, x)
            _refused(lib, st, "weights not loaded")
        assert kernels == set()
        torch.cuda.synchronize()
        assert torch.equal(_run(lib, kind, precision, b, x), first)      # a refused load leaves the handle as it was
    finally:
        torch.cuda.synchronize()
        a.close()
        for h in (b, fresh):
            if h.value:
                destroy(h)
