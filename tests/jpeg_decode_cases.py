"""The recorded cases of the JPEG decoder (tests/golden/jpeg_decode_cases.npz, written by tests/golden/make_jpeg_decode_golden.py),
the malformed scans of its tests, and a runner of casync_op_jpegdec_decode whose device buffers sit between fences, after
tests/jpeg_cases.py, whose helpers it uses.  Every comparison is byte equality.  Nothing here touches a GPU at import."""
import functools
import hashlib
import importlib.util
import os

import numpy as np

import jpeg_cases as jc

HERE = os.path.dirname(os.path.abspath(__file__))
BIG_CHUNK = 1 << 30          # above every scan: one subsequence per restart segment


@functools.lru_cache(maxsize=None)
def generator():
    spec = importlib.util.spec_from_file_location("make_jpeg_decode_golden", os.path.join(HERE, "golden", "make_jpeg_decode_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _npz():
    with np.load(os.path.join(HERE, "golden", "jpeg_decode_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def names():
    return [str(n) for n in _npz()["names"]]


@functools.lru_cache(maxsize=None)
def case(name):
    """(the file's bytes, Pillow's pixels BGR uint8 [H,W,3] or None, the SHA-256 of the pixels)"""
    z = _npz()
    data = z[name + ".jpeg"].tobytes()
    if name + ".pixels" in z:
        px = z[name + ".pixels"]
        px.setflags(write=False)
        return data, px, hashlib.sha256(px.tobytes()).hexdigest()
    return data, None, z[name + ".sha256"].tobytes().hex()


def differences(got: np.ndarray, name) -> float:
    """bytes of got [H,W,3] that differ from the recorded pixels of a case (inf: another shape, or another hash)"""
    _, px, sha = case(name)
    if px is None:
        return 0.0 if hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == sha else float("inf")
    return float((got != px).sum()) if got.shape == px.shape else float("inf")


def size_of(name):
    h, w = name.split("_")[1].split("x")
    return int(h), int(w)


@functools.lru_cache(maxsize=None)
def full_files():
    """(the host twin's 4:2:0 file of jpeg420_cases' seeded 1080 x 1920 frame, the recorded SHA-256 of Pillow's pixels)"""
    import jpeg420_cases as j4
    from calipsync_amd import jpeg
    frame, q, _, _ = j4.full_case()
    data = jpeg.encode_jpeg_host(frame, q, "4:2:0")
    z = _npz()
    assert hashlib.sha256(data).digest() == z[generator().FULL + ".file_sha256"].tobytes()
    return data, z[generator().FULL + ".sha256"].tobytes().hex()


@functools.lru_cache(maxsize=None)
def pixels_of(data: bytes) -> np.ndarray:
    """the host twin's pixels of a file without a fixture, computed once (read-only)"""
    from calipsync_amd import jpeg
    px = jpeg.decode_jpeg_host(data)
    px.setflags(write=False)
    return px


# ---------------------------------------------------------------------------------------------------------------- malformed scans
def _stuffed(bits: str) -> bytes:
    bits += "1" * (-len(bits) % 8)
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big")
    return raw.replace(b"\xff", b"\xff\x00")


@functools.lru_cache(maxsize=None)
def malformed():
    """{name: (good file, bad file, other good file)}: valid headers in front of a broken scan, between two valid files of its
    size.  Ordinary inputs that must come back with a status."""
    from calipsync_amd import jpeg
    gen = generator()
    a, b = case("noise_48x64_default")[0], case("smooth_48x64_default")[0]
    info = jpeg.parse_jpeg(a)
    head, scan = a[:info.scan_offset], a[info.scan_offset:info.scan_offset + info.scan_length]
    rng = np.random.default_rng(20250)
    noise = bytearray()                                          # random bytes of the scan's length, every 0xFF stuffed, so that no byte
    for v in rng.integers(0, 256, len(scan), dtype=np.uint8).tolist():      # reads as a marker and all of them reach the decoder
        noise += b"\xff\x00" if v == 0xFF else bytes([v])
    noise = bytes(noise[:len(scan)])
    if noise.endswith(b"\xff"):
        noise = noise[:-1] + b"\xfe"
    out = {"cut_in_half": (a, head + scan[:len(scan) // 2], b),
           "random_bytes": (a, head + noise + b"\xff\xd9", b),
           # Annex K luma: DC category 0 is 00, ZRL is 11111111001; the fourth ZRL passes coefficient 63
           "zrl_overrun": (a, head + _stuffed("00" + "11111111001" * 4) + b"\xff\xd9", b)}
    one, two = gen.pillow_write(gen.frame("noise", 8, 8), subsampling=0), gen.pillow_write(gen.frame("noise", 8, 16), subsampling=0)
    i1, i2 = jpeg.parse_jpeg(one), jpeg.parse_jpeg(two)
    out["too_many_blocks"] = (one, one[:i1.scan_offset] + two[i2.scan_offset:], gen.pillow_write(gen.frame("smooth", 8, 8), subsampling=0))
    return out


# ---------------------------------------------------------------------------------------------------------------- the operator
class OpResult:
    """status [B] int32, out [B,H,W,3] uint8, fences_ok"""


def run_op(files, chunk_bits: int = 0) -> OpResult:
    """casync_op_jpegdec_decode on a batch of files of one size; data, scratch, out and status each between 0x5A fences, out
    and scratch filled with 0x5A as well"""
    import torch
    from calipsync_amd import _lib, jpeg
    lib = _lib.load()
    plan = jpeg.plan_decode(list(files), chunk_bits)
    sizes = {(x.H, x.W) for x in plan.infos if isinstance(x, jpeg.JpegInfo)}
    assert len(sizes) == 1, sizes
    H, W = next(iter(sizes))
    B = len(files)
    need = int(lib.casync_op_jpegdec_workspace_bytes(B, H, W, plan.subsampling, plan.total_sub))
    assert need >= 64 * plan.total_sub
    bufs = {k: jc._fenced(n) for k, n in (("data", plan.blob.size), ("scratch", need), ("out", B * H * W * 3), ("status", 4 * B))}
    bufs["data"][1].copy_(torch.from_numpy(plan.blob.copy()))
    jpeg.decode_jpeg_op(plan, bufs["data"][1], bufs["scratch"][1], bufs["out"][1], bufs["status"][1].view(torch.int32), H, W)
    torch.cuda.synchronize()
    r = OpResult()
    r.fences_ok = all(jc._fence_ok(buf, mid.numel()) for buf, mid in bufs.values())
    r.data_ok = bool((bufs["data"][1].cpu().numpy() == plan.blob).all())
    r.status = bufs["status"][1].cpu().numpy().view(np.int32).copy()
    r.out = bufs["out"][1].cpu().numpy().reshape(B, H, W, 3).copy()
    return r
