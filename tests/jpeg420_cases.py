"""The recorded cases of the 4:2:0 JPEG encoder (tests/golden/jpeg420_cases.npz, written by tests/golden/make_jpeg420_golden.py)
and a runner of casync_op_jpeg420_encode whose four device buffers sit between fences, after tests/jpeg_cases.py, whose helpers
it uses.  Every comparison is byte equality.  Nothing here touches a GPU at import."""
import functools
import importlib.util
import os

import numpy as np

import jpeg_cases as jc

HERE = os.path.dirname(os.path.abspath(__file__))
SUB = "4:2:0"


@functools.lru_cache(maxsize=None)
def generator():
    """tests/golden/make_jpeg420_golden.py as a module: its pillow() writes 4:2:0, its inputs are make_jpeg_golden.py's"""
    spec = importlib.util.spec_from_file_location("make_jpeg420_golden", os.path.join(HERE, "golden", "make_jpeg420_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _npz():
    with np.load(os.path.join(HERE, "golden", "jpeg420_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def names():
    return [str(n) for n in _npz()["names"]]


@functools.lru_cache(maxsize=None)
def case(name):
    """(input BGR uint8 [H,W,3], quality, the recorded bytes), read-only"""
    z = _npz()
    frame = z[name + ".input"]
    frame.setflags(write=False)
    return frame, int(z[name + ".quality"]), z[name + ".jpeg"].tobytes()


FULL = "full_1080x1920_q95"


@functools.lru_cache(maxsize=None)
def full_case():
    """(input, quality, sha256 hex, length) of the one full-size case: only its hash is recorded"""
    z = _npz()
    frame = generator().full_size(int(z[FULL + ".seed"]))
    frame.setflags(write=False)
    return frame, int(z[FULL + ".quality"]), z[FULL + ".sha256"].tobytes().hex(), int(z[FULL + ".length"])


@functools.lru_cache(maxsize=None)
def seeded(h, w, seed):
    """a frame without a fixture: a slow gradient with a patch of noise in the middle (read-only)"""
    gen = jc.generator()
    frame = gen.smooth(seed, h, w)
    ys, xs = slice(h // 3, max(2 * h // 3, h // 3 + 1)), slice(w // 4, max(3 * w // 4, w // 4 + 1))
    frame[ys, xs] = gen.noise(seed, h, w)[ys, xs]
    frame.setflags(write=False)
    return frame


@functools.lru_cache(maxsize=None)
def twin(h, w, seed, q):
    """the host twin's 4:2:0 file of seeded(h, w, seed), computed once"""
    from calipsync_amd import jpeg
    return jpeg.encode_jpeg_host(seeded(h, w, seed), q, SUB)


def run_op(frames: np.ndarray, quality: int, slot_bytes: int = 0, out_cap=None, spare: int = 64) -> jc.OpResult:
    """casync_op_jpeg420_encode on a batch [B,H,W,3]; out_cap None: room for every frame that passes its slots, plus `spare`."""
    import torch
    from calipsync_amd import _lib, jpeg
    lib = _lib.load()
    B, H, W = frames.shape[:3]
    rows = (H + 15) // 16
    slot = slot_bytes or jpeg.default_slot_bytes(W, SUB)
    need = int(lib.casync_op_jpeg420_workspace_bytes(B, H, W, slot_bytes))
    assert need >= B * rows * (4 + slot)
    cap = B * (jpeg.HEADER_BYTES + rows * slot) + spare if out_cap is None else int(out_cap)
    dev = torch.from_numpy(np.array(frames)).to("cuda:0")          # a copy: the cases are read-only
    bufs = {k: jc._fenced(n) for k, n in (("scratch", need), ("out", cap), ("offsets", 8 * (B + 1)), ("status", 4 * B))}
    _lib.check(lib.casync_op_jpeg420_encode(dev.data_ptr(), B, H, W, quality, slot_bytes, bufs["scratch"][1].data_ptr(), need,
                                            bufs["out"][1].data_ptr(), cap, bufs["offsets"][1].data_ptr(), bufs["status"][1].data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "casync_op_jpeg420_encode")
    torch.cuda.synchronize()
    r = jc.OpResult()
    r.fences_ok = all(jc._fence_ok(buf, mid.numel()) for buf, mid in bufs.values())
    r.offsets = bufs["offsets"][1].cpu().numpy().view(np.int64).copy()
    r.status = bufs["status"][1].cpu().numpy().view(np.int32).copy()
    r.out = bufs["out"][1].cpu().numpy().copy()
    end = int(r.offsets[B])
    r.tail_ok = 0 <= end <= cap and bool((r.out[end:] == jc.FILL).all())
    return r
