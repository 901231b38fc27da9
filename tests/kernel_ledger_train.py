"""The ledger of calipsync_amd/lib/obj_train/ (the trainer's batch kernel, csrc/train_ops.hip), under the rule of
tests/kernel_ledger.py: every compiled kernel instance has op-level cases that launch it through casync_op_train_batch with the
launch log on.  The kernel is integer resize arithmetic and one IEEE division a value: every bar is exact equality with the numpy
restatement (tests/train_data_ref.py), the error is the number of differing floats of both outputs (inf where a sentinel around
an output changed).  The two instances differ in their stores alone (16-byte, or 4-byte where an output is not 16-byte aligned):
the cases of the second hand the entry outputs that start one float off.  tests/test_train_data_gpu.py names the shapes
these cases hold and runs the same helpers on a frame above byte 2^31, against the inference path and on the refusals.  Nothing here touches a GPU at import."""
from __future__ import annotations

import zlib

import numpy as np

import train_data_ref as ref
from calipsync_amd.train_data import REC_WORDS
from kernel_ledger import C, _done, _lib, _Run, _s, _t

PAD = 64                  # sentinel floats on either side of an output
SENTINEL = -777.0
RECORDS_PER_LAUNCH = 64   # csrc/train_ops.hip
WIDTHS = (1, 2, 3, 83, 84, 85, 167, 168, 169, 336, 337, 701)   # square regions: around 168 / 2, 168 (a copy), 336 (exact 2x: INTER_AREA)


def noise_frames(n, H, W, *key):
    """n seeded noise frames [n,H,W,3] uint8 (every seventh row darker: some structure)"""
    rng = np.random.default_rng(zlib.crc32(repr(("train frames", n, H, W) + key).encode()))
    f = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    f[:, ::7] //= 2
    return f


def boxes(H, W):
    """(y0, x0, h, w) inside an H x W frame: every square of WIDTHS that fits, regions cut at the bottom edge, at the right edge and
    at both (non-square), a square that ends on the last row and column, and (where it fits) a 336-wide region cut to 200 rows,
    which must NOT take the exact-2x branch"""
    out = [((H - s) // 3, (W - s) // 2, s, s) for s in WIDTHS if s <= min(H, W)]
    s = min(90, H, W)
    out += [(H - s // 2 - 5, (W - s) // 2, s // 2 + 5, s), ((H - s) // 2, W - s // 3 - 7, s, s // 3 + 7), (H - 41, W - 29, 41, 29),
            (H - s, W - s, s, s)]
    if W >= 336 and H >= 200:
        out.append((H - 200, (W - 336) // 2, 200, 336))
    assert all(y >= 0 and x >= 0 and h >= 1 and w >= 1 and y + h <= H and x + w <= W for y, x, h, w in out), out
    return out


def records(H, W, n_frames, batch=None):
    """[batch,12] int32: record i pairs box i (target) with box i + 1 (reference) on frames that differ where there are two; the last
    record's reference is its own target, frame and box"""
    bx = boxes(H, W)
    batch = len(bx) if batch is None else batch
    rec = np.zeros((batch, REC_WORDS), dtype=np.int32)
    for i in range(batch):
        rec[i, 0], rec[i, 1:5] = i % n_frames, bx[i % len(bx)]
        rec[i, 5], rec[i, 6:10] = (3 * i + 1) % n_frames, bx[(i + 1) % len(bx)]
    rec[-1, 5:10] = rec[-1, 0:5]
    return rec


def expected(frames, rec):
    """the restatement of every record -> (img_concat [B,6,160,160], img_real [B,3,160,160]); one resize per distinct (frame, box)"""
    reals = {}

    def real(side):
        key = tuple(int(v) for v in side)
        if key not in reals:
            f, y0, x0, h, w = key
            reals[key] = ref.real_of(frames[f][y0:y0 + h, x0:x0 + w])
        return reals[key]

    pairs = [ref.tensors(real(r[0:5]), real(r[5:10])) for r in rec]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def call(frames_dev, n_frames, H, W, rec, misalign=0):
    """casync_op_train_batch into sentinel-filled buffers that start `misalign` floats off a 16-byte boundary -> (status, img_concat,
    img_real, sentinels intact); the outputs as numpy arrays"""
    torch = _t()
    rec = np.ascontiguousarray(rec, dtype=np.int32)
    b = rec.shape[0]
    bufs = [torch.full((2 * PAD + misalign + max(b, 1) * c * 25600,), SENTINEL, dtype=torch.float32, device="cuda:0") for c in (6, 3)]
    ptrs = [buf.data_ptr() + 4 * (PAD + misalign) for buf in bufs]
    st = _lib().casync_op_train_batch(frames_dev.data_ptr(), n_frames, H, W, rec.ctypes.data, b, ptrs[0], ptrs[1], _s())
    torch.cuda.synchronize()
    host = [buf.cpu().numpy() for buf in bufs]
    lo = PAD + misalign
    outs = [h[lo:lo + b * c * 25600].reshape(b, c, 160, 160) for h, c in zip(host, (6, 3))]
    intact = all((h[:lo] == SENTINEL).all() and (h[lo + b * c * 25600:] == SENTINEL).all() for h, c in zip(host, (6, 3)))
    return st, outs[0], outs[1], intact


def differing(frames, rec, misalign=0, frames_dev=None, n_frames=None):
    """the entry against the restatement: floats that differ in both outputs, inf where a sentinel changed or the entry refused"""
    torch = _t()
    if frames_dev is None:
        frames_dev = torch.from_numpy(frames).to("cuda:0")
    H, W = int(frames_dev.shape[1]), int(frames_dev.shape[2])
    st, cat, real, intact = call(frames_dev, int(frames_dev.shape[0]) if n_frames is None else n_frames, H, W, rec, misalign)
    if st != 0 or not intact:
        return float("inf")
    want_cat, want_real = expected(frames, rec)
    return float((cat.view(np.uint32) != want_cat.view(np.uint32)).sum() + (real.view(np.uint32) != want_real.view(np.uint32)).sum())


def shapes(H, W, n_frames, misalign=0):
    """every box of boxes(H, W) as target and as reference, one launch"""
    frames = noise_frames(n_frames, H, W)
    rec = records(H, W, n_frames)
    with _Run(0) as r:
        err = differing(frames, rec, misalign)
    return _done(r, err, 0.0, f"{len(rec)} records on {n_frames} frame(s) of {H} x {W}, outputs {misalign} float(s) off")


def many(H, W, n_frames, batch, misalign=0):
    """more records than one launch carries"""
    frames = noise_frames(n_frames, H, W)
    rec = records(H, W, n_frames, batch)
    with _Run(0) as r:
        err = differing(frames, rec, misalign)
    return _done(r, err, 0.0, f"{batch} records ({-(-batch // RECORDS_PER_LAUNCH)} launches) on {n_frames} frames of {H} x {W}, outputs {misalign} off")


# 211 x 317: a row of 951 bytes, no multiple of 16; 720 x 720 holds every width; one frame (target and reference share it); one
# record; one more than a launch's block of records
LEDGER = {
    "train_batch_kernel<true>": [C(shapes, 211, 317, 3), C(shapes, 720, 720, 2), C(shapes, 211, 317, 1), C(many, 211, 317, 3, 1),
                                 C(many, 211, 317, 3, RECORDS_PER_LAUNCH + 1)],
    "train_batch_kernel<false>": [C(shapes, 211, 317, 3, 1), C(shapes, 720, 720, 2, 3), C(many, 211, 317, 2, RECORDS_PER_LAUNCH + 1, 2)],
}


def cases():
    """[(kernel, index, case)] in ledger order: one GPU test each"""
    return [(name, i, c) for name, cs in LEDGER.items() for i, c in enumerate(cs)]


def launched_by(case):
    """the kernels a case is listed under: what its entry launches"""
    return {name for name, cs in LEDGER.items() if case in cs}
