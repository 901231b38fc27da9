"""The recorded cases of the wider JPEG decoder subset (tests/golden/mjpeg_decode_cases.npz, written by
tests/golden/make_mjpeg_decode_golden.py), the malformed 4:2:2 and grayscale scans of its tests, and a runner of
casync_op_mjpegdec_decode whose device buffers sit between fences, after tests/jpeg_decode_cases.py, whose helpers it uses.
Every comparison is byte equality.  Nothing here touches a GPU at import."""
import functools
import hashlib
import importlib.util
import os

import numpy as np

import jpeg_cases as jc
import jpeg_decode_cases as jd

HERE = os.path.dirname(os.path.abspath(__file__))
BIG_CHUNK = jd.BIG_CHUNK     # above every scan: one subsequence per restart segment
CHUNKS = (32, BIG_CHUNK)
SUBSET = "mjpeg"


@functools.lru_cache(maxsize=None)
def generator():
    spec = importlib.util.spec_from_file_location("make_mjpeg_decode_golden", os.path.join(HERE, "golden", "make_mjpeg_decode_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _npz():
    with np.load(os.path.join(HERE, "golden", "mjpeg_decode_cases.npz")) as z:
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


def by_size():
    """{(h, w): [names]}: the operator takes a batch of one size"""
    out = {}
    for n in names():
        out.setdefault(size_of(n), []).append(n)
    return out


# one 48 x 64 file of each sampling word 0, 1, 2, 3: (module, name)
MIXED = ((jd, "noise_48x64_sub0"), (None, "c422smooth_48x64_default"), (jd, "smooth_48x64_default"), (None, "graynoise_48x64_optimize"))


def mixed_batch():
    """[(file, name, differences function)] of MIXED"""
    return [((m or _self()).case(n)[0], n, (m or _self()).differences) for m, n in MIXED]


def _self():
    import mjpeg_decode_cases
    return mjpeg_decode_cases


@functools.lru_cache(maxsize=None)
def pixels_of(data: bytes) -> np.ndarray:
    """the host twin's pixels of a file without a fixture, computed once (read-only)"""
    from calipsync_amd import jpeg
    px = jpeg.decode_jpeg_host(data, subset=SUBSET)
    px.setflags(write=False)
    return px


# ---------------------------------------------------------------------------------------------------------------- malformed scans
MALFORMED = tuple(f"{s}_{k}" for s in ("422", "gray") for k in ("invalid_code", "zrl_overrun", "too_few_blocks", "too_many_blocks", "cut_in_half"))


@functools.lru_cache(maxsize=None)
def malformed():
    """{name: (good file, bad file, other good file)} for 4:2:2 and grayscale, built as jpeg_decode_cases.malformed() builds its
    own: valid headers (Annex K tables) in front of a broken scan, between two valid files of its size.  Ordinary inputs that must
    come back with a status."""
    from calipsync_amd import jpeg
    gen = generator()
    out = {}
    for s in ("422", "gray"):
        small, wide = ((8, 16), (8, 32)) if s == "422" else ((8, 8), (8, 16))          # one MCU, two MCUs
        write = lambda kind, hw: gen.pillow_write(gen.frame(kind, *hw), s)
        a, b = write("noise", small), write("smooth", small)
        a2, b2 = write("noise", wide), write("smooth", wide)
        i1, i2 = jpeg.parse_jpeg(a, SUBSET), jpeg.parse_jpeg(a2, SUBSET)
        head, scan = a[:i1.scan_offset], a[i1.scan_offset:i1.scan_offset + i1.scan_length]
        # Annex K luma: no DC code is sixteen 1-bits; DC category 0 is 00, ZRL is 11111111001 and the fourth passes coefficient 63
        out[f"{s}_invalid_code"] = (a, head + jd._stuffed("1" * 16) + b"\xff\xd9", b)
        out[f"{s}_zrl_overrun"] = (a, head + jd._stuffed("00" + "11111111001" * 4) + b"\xff\xd9", b)
        out[f"{s}_too_few_blocks"] = (a2, a2[:i2.scan_offset] + a[i1.scan_offset:], b2)
        out[f"{s}_too_many_blocks"] = (a, head + a2[i2.scan_offset:], b)
        out[f"{s}_cut_in_half"] = (a, head + scan[:len(scan) // 2], b)
    assert sorted(out) == sorted(MALFORMED)
    return out


# ---------------------------------------------------------------------------------------------------------------- the operator
def run_op(files, chunk_bits: int = 0, entry: str = SUBSET) -> jd.OpResult:
    """casync_op_mjpegdec_decode on a batch of files of one size; data, scratch, out and status each between 0x5A fences, out
    and scratch filled with 0x5A as well.  entry="baseline": the same batch through casync_op_jpegdec_decode (jd.run_op)."""
    if entry == "baseline":
        return jd.run_op(files, chunk_bits)
    import torch
    from calipsync_amd import jpeg
    plan = jpeg.plan_decode(list(files), chunk_bits, subset=SUBSET)
    sizes = {(x.H, x.W) for x in plan.infos if isinstance(x, jpeg.JpegInfo)}
    assert len(sizes) == 1, sizes
    H, W = next(iter(sizes))
    B = len(files)
    need = jpeg.workspace_bytes(plan, B, H, W)
    assert need >= 64 * plan.total_sub
    bufs = {k: jc._fenced(n) for k, n in (("data", plan.blob.size), ("scratch", need), ("out", B * H * W * 3), ("status", 4 * B))}
    bufs["data"][1].copy_(torch.from_numpy(plan.blob.copy()))
    jpeg.decode_jpeg_op(plan, bufs["data"][1], bufs["scratch"][1], bufs["out"][1], bufs["status"][1].view(torch.int32), H, W)
    torch.cuda.synchronize()
    r = jd.OpResult()
    r.fences_ok = all(jc._fence_ok(buf, mid.numel()) for buf, mid in bufs.values())
    r.data_ok = bool((bufs["data"][1].cpu().numpy() == plan.blob).all())
    r.status = bufs["status"][1].cpu().numpy().view(np.int32).copy()
    r.out = bufs["out"][1].cpu().numpy().reshape(B, H, W, 3).copy()
    return r
