"""The ledger of calipsync_amd/lib/obj_jpeg420/ (the 4:2:0 JPEG encoder of finished frames, csrc/jpeg_enc420.hip), under the rule
of tests/kernel_ledger.py: every compiled kernel instance has op-level cases that launch it through its casync_op_* entry with
the launch log on.  casync_op_jpeg420_encode launches its three kernels together, so they share their cases.  Every bar is exact
equality with the recorded libjpeg-turbo bytes (tests/golden/jpeg420_cases.npz): the error is the number of differing bytes of
the files, inf where a length, a status or an offset is wrong, a fence around scratch, out, offsets or status changed, or a byte
of out past offsets[B] changed.  Nothing here touches a GPU at import."""
from __future__ import annotations

import numpy as np

import jpeg420_cases as j4
from kernel_ledger import C, _done, _Run
from kernel_ledger_jpeg import _differences


def fixture(name):
    """casync_op_jpeg420_encode on one recorded case, a batch of one"""
    frame, q, want = j4.case(name)
    with _Run(0) as r:
        res = j4.run_op(frame[None], q)
    return _done(r, _differences(res, [want]), 0.0, f"{name}: {len(want)} bytes")


def full_size():
    """the 1080 x 1920 case twice in one batch (68 MCU rows, the last with a bottom row of dummies; four chunks of 32 MCUs a row): by hash"""
    frame, q, sha, length = j4.full_case()
    with _Run(0) as r:
        res = j4.run_op(np.stack([frame, frame]), q)
    ok = res.fences_ok and res.tail_ok and list(res.status) == [0, 0] and list(res.offsets) == [0, length, 2 * length] and \
        j4.jc.sha256(res.file(0)) == sha and j4.jc.sha256(res.file(1)) == sha
    return _done(r, 0.0 if ok else float("inf"), 0.0, f"two full-size frames of {length} bytes")


def outgrown_slot():
    """noise | constant | noise at quality 100 with slots of an MCU row's raw size: the noise rows do not fit"""
    noise, q, _ = j4.case("noise_32x32_q100")
    flat = np.full((32, 32, 3), 99, dtype=np.uint8)
    from calipsync_amd import jpeg
    with _Run(0) as r:
        res = j4.run_op(np.stack([noise, flat, noise[::-1]]), q, slot_bytes=384 * 2)
    return _done(r, _differences(res, [None, jpeg.encode_jpeg_host(flat, q, j4.SUB), None]), 0.0,
                 "a batch whose first and last frame outgrow their slots")


def short_out(missing):
    """three different 19 x 37 frames with out_cap `missing` bytes short of the need: the last frame fails alone"""
    frame, q, want = j4.case("noise_19x37_q95")
    from calipsync_amd import jpeg
    batch = np.stack([frame, frame[::-1], frame[:, ::-1]])
    wants = [want, jpeg.encode_jpeg_host(batch[1], q, j4.SUB), jpeg.encode_jpeg_host(batch[2], q, j4.SUB)]
    need = sum(len(w) for w in wants)
    with _Run(0) as r:
        res = j4.run_op(batch, q, out_cap=need - missing)
    return _done(r, _differences(res, wants if missing <= 0 else wants[:2] + [None]), 0.0, f"out_cap {missing} bytes short of {need}")


_SHARED = [C(fixture, n) for n in j4.names()] + [C(full_size), C(outgrown_slot), C(short_out, 0), C(short_out, 1)]
LEDGER = {
    "jpeg420_encode_rows_kernel": _SHARED,
    "jpeg420_plan_kernel": _SHARED,
    "jpeg420_pack_kernel": _SHARED,
}


def cases():
    """[(kernels, index, case)] in ledger order: one GPU test per case, which must launch exactly the kernels that list it"""
    return [(sorted(k for k, cs in LEDGER.items() if c in cs), i, c) for i, c in enumerate(_SHARED)]
