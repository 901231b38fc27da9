"""The recorded cases of the JPEG encoder (tests/golden/jpeg_cases.npz, written by tests/golden/make_jpeg_golden.py) and a runner
of casync_op_jpeg_encode whose four device buffers sit between fences.  Every comparison is byte equality.  Nothing here touches
a GPU at import."""
import functools
import hashlib
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FILL = 0x5A
FENCE = 256             # bytes before and after a buffer; a multiple of every alignment the operator asks for


@functools.lru_cache(maxsize=None)
def generator():
    """tests/golden/make_jpeg_golden.py as a module: the seeded inputs come from its functions"""
    spec = importlib.util.spec_from_file_location("make_jpeg_golden", os.path.join(HERE, "golden", "make_jpeg_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _npz():
    with np.load(os.path.join(HERE, "golden", "jpeg_cases.npz")) as z:
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


def sha256(data) -> str:
    return hashlib.sha256(data).hexdigest()


def pillow_restart_rows() -> bool:
    """does this Pillow write one restart interval per block row when asked to"""
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.new("RGB", (8, 16)).save(buf, format="JPEG", quality=95, subsampling=0, restart_marker_rows=1)
    return b"\xff\xdd" in buf.getvalue()


def decode(data: bytes) -> np.ndarray:
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        assert im.format == "JPEG"
        return np.asarray(im.convert("RGB"))


# ---------------------------------------------------------------------------------------------------------------- the operator
class OpResult:
    """status [B], offsets [B+1], out (the whole buffer, uint8), fences_ok, tail_ok (the bytes of out past offsets[B] unchanged)"""

    def file(self, i):
        return self.out[self.offsets[i]:self.offsets[i + 1]].tobytes()


def _fenced(nbytes):
    import torch
    buf = torch.full((nbytes + 2 * FENCE,), FILL, dtype=torch.uint8, device="cuda:0")
    return buf, buf[FENCE:FENCE + nbytes]


def _fence_ok(buf, nbytes):
    got = buf.cpu().numpy()
    return bool((got[:FENCE] == FILL).all() and (got[FENCE + nbytes:] == FILL).all())


def run_op(frames: np.ndarray, quality: int, slot_bytes: int = 0, out_cap=None, spare: int = 64) -> OpResult:
    """casync_op_jpeg_encode on a batch [B,H,W,3]; out_cap None: room for every frame that passes its slots, plus `spare`."""
    import torch
    from calipsync_amd import _lib, jpeg
    lib = _lib.load()
    B, H, W = frames.shape[:3]
    rows = (H + 7) // 8
    slot = slot_bytes or jpeg.default_slot_bytes(W)
    need = int(lib.casync_op_jpeg_workspace_bytes(B, H, W, slot_bytes))
    assert need >= B * rows * (4 + slot)
    cap = B * (jpeg.HEADER_BYTES + rows * slot) + spare if out_cap is None else int(out_cap)
    dev = torch.from_numpy(np.array(frames)).to("cuda:0")          # a copy: the cases are read-only
    bufs = {k: _fenced(n) for k, n in (("scratch", need), ("out", cap), ("offsets", 8 * (B + 1)), ("status", 4 * B))}
    _lib.check(lib.casync_op_jpeg_encode(dev.data_ptr(), B, H, W, quality, slot_bytes, bufs["scratch"][1].data_ptr(), need,
                                         bufs["out"][1].data_ptr(), cap, bufs["offsets"][1].data_ptr(), bufs["status"][1].data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "casync_op_jpeg_encode")
    torch.cuda.synchronize()
    r = OpResult()
    r.fences_ok = all(_fence_ok(buf, mid.numel()) for buf, mid in bufs.values())
    r.offsets = bufs["offsets"][1].cpu().numpy().view(np.int64).copy()
    r.status = bufs["status"][1].cpu().numpy().view(np.int32).copy()
    r.out = bufs["out"][1].cpu().numpy().copy()
    end = int(r.offsets[B])
    r.tail_ok = 0 <= end <= cap and bool((r.out[end:] == FILL).all())
    return r
