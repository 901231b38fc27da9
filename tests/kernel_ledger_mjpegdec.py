"""The ledger of calipsync_amd/lib/obj_mjpegdec/ (the Motion-JPEG decoder, csrc/jpeg_dec_mjpeg.hip), under the rule of
tests/kernel_ledger.py: every compiled kernel instance has op-level cases that launch it through its casync_op_* entry with the
launch log on.  casync_op_mjpegdec_decode launches its four kernels together, so they share their cases.  Every bar is exact
equality with the pixels Pillow (libjpeg-turbo) decodes (tests/golden/mjpeg_decode_cases.npz; for 4:4:4 and 4:2:0
tests/golden/jpeg_decode_cases.npz, and there also with the bytes of casync_op_jpegdec_decode): the error is the number of
differing bytes of the frames, inf where a status is wrong, a fence around data, scratch, out or status changed, or the data
buffer changed.  Nothing here touches a GPU at import."""
from __future__ import annotations

import jpeg_decode_cases as jd
import mjpeg_decode_cases as mj
from kernel_ledger import C, _done, _Run

SIZES = sorted(mj.by_size())
BASELINE_SIZES = sorted({jd.size_of(n) for n in jd.names()})


def _ok(res, statuses):
    return res.fences_ok and res.data_ok and list(res.status) == list(statuses)


def one_size(h, w, chunk_bits=0):
    """every recorded file of one size in one batch: 4:2:2 and gray, every setting, the files without tables"""
    group = mj.by_size()[(h, w)]
    with _Run(0) as r:
        res = mj.run_op([mj.case(n)[0] for n in group], chunk_bits)
    err = sum(mj.differences(res.out[i], n) for i, n in enumerate(group)) if _ok(res, [0] * len(group)) else float("inf")
    return _done(r, err, 0.0, f"{len(group)} files of {h} x {w} at chunk_bits {chunk_bits}")


def four_samplings(chunk_bits=0):
    """one 48 x 64 file of each sampling word in one batch"""
    batch = mj.mixed_batch()
    with _Run(0) as r:
        res = mj.run_op([f for f, _, _ in batch], chunk_bits)
    err = sum(diff(res.out[i], n) for i, (_, n, diff) in enumerate(batch)) if _ok(res, [0] * 4) else float("inf")
    return _done(r, err, 0.0, f"4:4:4, 4:2:2, 4:2:0 and gray in one batch at chunk_bits {chunk_bits}")


def baseline_files(h, w):
    """every 4:4:4 and 4:2:0 file of tests/jpeg_decode_cases.py of one size: the recorded pixels through this entry"""
    group = [n for n in jd.names() if jd.size_of(n) == (h, w)]
    with _Run(0) as r:
        res = mj.run_op([jd.case(n)[0] for n in group])
    err = sum(jd.differences(res.out[i], n) for i, n in enumerate(group)) if _ok(res, [0] * len(group)) else float("inf")
    return _done(r, err, 0.0, f"{len(group)} baseline files of {h} x {w}")


def broken_one(name):
    """(launched names, error, what) of one malformed scan between two valid files: its status is the host twin's, the
    neighbours are exact"""
    from calipsync_amd import jpeg
    a, bad, b = mj.malformed()[name]
    want = jpeg.scan_status(bad, subset="mjpeg")
    with _Run(0) as r:
        res = mj.run_op([a, bad, b])
    ok = want != 0 and _ok(res, [0, want, 0])
    err = float((res.out[0] != mj.pixels_of(a)).sum() + (res.out[2] != mj.pixels_of(b)).sum()) if ok else float("inf")
    return r.names, err, f"{name}: status {list(res.status)}, the host twin says {want}"


def broken(sampling):
    """the five malformed scans of a sampling ("422" / "gray"), one batch of three each"""
    runs = [broken_one(n) for n in mj.MALFORMED if n.startswith(sampling + "_")]
    r = type("Names", (), {"names": set().union(*(set(n) for n, _, _ in runs))})
    return _done(r, sum(e for _, e, _ in runs), 0.0, "; ".join(w for _, _, w in runs))


_SHARED = [C(one_size, h, w) for h, w in SIZES] + [C(four_samplings)] + [C(baseline_files, h, w) for h, w in BASELINE_SIZES] + [
    C(broken, s) for s in ("422", "gray")]
LEDGER = {
    "mjpegdec_sync_kernel": _SHARED,
    "mjpegdec_write_kernel": _SHARED,
    "mjpegdec_idct_kernel": _SHARED,
    "mjpegdec_color_kernel": _SHARED,
}


def cases():
    """[(kernels, index, case)] in ledger order: one GPU test per case, which must launch exactly the kernels that list it"""
    return [(sorted(k for k, cs in LEDGER.items() if c in cs), i, c) for i, c in enumerate(_SHARED)]
