"""The ledger of calipsync_amd/lib/obj_jpegdec/ (the baseline JPEG decoder, csrc/jpeg_dec.hip), under the rule of
tests/kernel_ledger.py: every compiled kernel instance has op-level cases that launch it through its casync_op_* entry with the
launch log on.  casync_op_jpegdec_decode launches its four kernels together, so they share their cases.  Every bar is exact
equality with the pixels Pillow (libjpeg-turbo) decodes (tests/golden/jpeg_decode_cases.npz): the error is the number of
differing bytes of the frames, inf where a status is wrong, a fence around data, scratch, out or status changed, or the data
buffer changed.  Nothing here touches a GPU at import."""
from __future__ import annotations

import hashlib

import numpy as np

import jpeg_decode_cases as jd
from kernel_ledger import C, _done, _Run

FIVE = ("noise_33x18_default", "smooth_33x18_sub0", "noise_33x18_optimize", "smooth_33x18_rstblocks", "noise_33x18_q100")


def _ok(res, statuses):
    return res.fences_ok and res.data_ok and list(res.status) == list(statuses)


def fixture(name, chunk_bits=0):
    """casync_op_jpegdec_decode on one recorded file, a batch of one"""
    with _Run(0) as r:
        res = jd.run_op([jd.case(name)[0]], chunk_bits)
    err = jd.differences(res.out[0], name) if _ok(res, [0]) else float("inf")
    return _done(r, err, 0.0, f"{name} at chunk_bits {chunk_bits}")


def five_settings():
    """five 33 x 18 files in one batch: tables, sampling and restart interval differ frame by frame"""
    with _Run(0) as r:
        res = jd.run_op([jd.case(n)[0] for n in FIVE])
    err = sum(jd.differences(res.out[i], n) for i, n in enumerate(FIVE)) if _ok(res, [0] * 5) else float("inf")
    return _done(r, err, 0.0, "five 33 x 18 files with five settings")


def many_small(n=80):
    """80 files of 7 x 5: the records travel 64 to a launch"""
    names = [k for k in jd.names() if k.split("_")[1] == "7x5"]
    names = [names[i % len(names)] for i in range(n)]
    with _Run(0) as r:
        res = jd.run_op([jd.case(k)[0] for k in names])
    err = sum(jd.differences(res.out[i], k) for i, k in enumerate(names)) if _ok(res, [0] * n) else float("inf")
    return _done(r, err, 0.0, f"{n} files of 7 x 5")


def full_size():
    """the 1080 x 1920 file twice in one batch (68 MCU rows, the bottom row of dummy Y blocks, the last chroma row from the real
    plane; no restart markers, so one segment of some 3000 subsequences): by hash"""
    data, sha = jd.full_files()
    with _Run(0) as r:
        res = jd.run_op([data, data])
    ok = _ok(res, [0, 0]) and all(hashlib.sha256(res.out[i].tobytes()).hexdigest() == sha for i in range(2))
    return _done(r, 0.0 if ok else float("inf"), 0.0, f"two full-size frames from files of {len(data)} bytes")


def broken(name):
    """a malformed scan between two valid files: its status is the host twin's, the neighbours are exact"""
    from calipsync_amd import jpeg
    a, bad, b = jd.malformed()[name]
    want = jpeg.scan_status(bad)
    with _Run(0) as r:
        res = jd.run_op([a, bad, b])
    ok = want != 0 and _ok(res, [0, want, 0])
    err = float((res.out[0] != jd.pixels_of(a)).sum() + (res.out[2] != jd.pixels_of(b)).sum()) if ok else float("inf")
    return _done(r, err, 0.0, f"{name}: status {list(res.status)}, the host twin says {want}")


_SHARED = [C(fixture, n) for n in jd.names()] + [C(five_settings), C(many_small), C(full_size)] + [
    C(broken, n) for n in ("cut_in_half", "random_bytes", "zrl_overrun", "too_many_blocks")]
LEDGER = {
    "jpegdec_sync_kernel": _SHARED,
    "jpegdec_write_kernel": _SHARED,
    "jpegdec_idct_kernel": _SHARED,
    "jpegdec_color_kernel": _SHARED,
}


def cases():
    """[(kernels, index, case)] in ledger order: one GPU test per case, which must launch exactly the kernels that list it"""
    return [(sorted(k for k, cs in LEDGER.items() if c in cs), i, c) for i, c in enumerate(_SHARED)]
