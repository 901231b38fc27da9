"""The ledger of calipsync_amd/lib/obj_jpeg/ (the baseline JPEG encoder of finished frames, csrc/jpeg_enc.hip), under the rule of
tests/kernel_ledger.py: every compiled kernel instance has op-level cases that launch it through its casync_op_* entry with the
launch log on.  casync_op_jpeg_encode launches its three kernels together, so they share their cases.  Every bar is exact
equality with the recorded libjpeg-turbo bytes (tests/golden/jpeg_cases.npz): the error is the number of differing bytes of the
files, inf where a length, a status or an offset is wrong, a fence around scratch, out, offsets or status changed, or a byte of
out past offsets[B] changed.  Nothing here touches a GPU at import."""
from __future__ import annotations

import numpy as np

import jpeg_cases as jc
from kernel_ledger import C, _done, _Run


def _differences(r, wants):
    """wants: per frame its expected file, or None where the frame must have failed"""
    if not (r.fences_ok and r.tail_ok and r.offsets[0] == 0):
        return float("inf")
    err = 0.0
    for i, want in enumerate(wants):
        got = r.file(i)
        if want is None:
            if r.status[i] == 0 or got:
                return float("inf")
        elif r.status[i] != 0 or len(got) != len(want):
            return float("inf")
        else:
            err += np.count_nonzero(np.frombuffer(got, dtype=np.uint8) != np.frombuffer(want, dtype=np.uint8))
    return err


def fixture(name):
    """casync_op_jpeg_encode on one recorded case, a batch of one"""
    frame, q, want = jc.case(name)
    with _Run(0) as r:
        res = jc.run_op(frame[None], q)
    return _done(r, _differences(res, [want]), 0.0, f"{name}: {len(want)} bytes")


def full_size():
    """the 1080 x 1920 case twice in one batch (135 block rows, four lane chunks a row): by hash"""
    frame, q, sha, length = jc.full_case()
    with _Run(0) as r:
        res = jc.run_op(np.stack([frame, frame]), q)
    ok = res.fences_ok and res.tail_ok and list(res.status) == [0, 0] and list(res.offsets) == [0, length, 2 * length] and \
        jc.sha256(res.file(0)) == sha and jc.sha256(res.file(1)) == sha
    return _done(r, 0.0 if ok else float("inf"), 0.0, f"two full-size frames of {length} bytes")


def outgrown_slot():
    """noise | constant | noise at quality 100 with slots of a block row's raw size: the noise rows do not fit"""
    noise, q, _ = jc.case("noise_16x16_q100")
    flat = np.full((16, 16, 3), 99, dtype=np.uint8)
    from calipsync_amd import jpeg
    with _Run(0) as r:
        res = jc.run_op(np.stack([noise, flat, noise[::-1]]), q, slot_bytes=8 * 3 * 16)
    return _done(r, _differences(res, [None, jpeg.encode_jpeg_host(flat, q), None]), 0.0, "a batch whose first and last frame outgrow their slots")


def short_out(missing):
    """three different 19 x 37 frames with out_cap `missing` bytes short of the need: the last frame fails alone"""
    frame, q, want = jc.case("noise_19x37_q95")
    from calipsync_amd import jpeg
    batch = np.stack([frame, frame[::-1], frame[:, ::-1]])
    wants = [want, jpeg.encode_jpeg_host(batch[1], q), jpeg.encode_jpeg_host(batch[2], q)]
    need = sum(len(w) for w in wants)
    with _Run(0) as r:
        res = jc.run_op(batch, q, out_cap=need - missing)
    return _done(r, _differences(res, wants if missing <= 0 else wants[:2] + [None]), 0.0, f"out_cap {missing} bytes short of {need}")


_SHARED = [C(fixture, n) for n in jc.names()] + [C(full_size), C(outgrown_slot), C(short_out, 0), C(short_out, 1)]
LEDGER = {
    "jpeg_encode_rows_kernel": _SHARED,
    "jpeg_plan_kernel": _SHARED,
    "jpeg_pack_kernel": _SHARED,
}


def cases():
    """[(kernels, index, case)] in ledger order: one GPU test per case, which must launch exactly the kernels that list it"""
    return [(sorted(k for k, cs in LEDGER.items() if c in cs), i, c) for i, c in enumerate(_SHARED)]
