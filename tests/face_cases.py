"""Shared by the face-pipeline tests (test_face_ops*.py, kernel_ledger_face.py, test_face_pipeline_gpu.py): seeded inputs, the
expected values from the unchanged oracle (oracle/frame_ops_oracle.py::resize_linear_u8) and from numpy, and runners that put
every output of a device operator into a sentinel-padded buffer.  Nothing here touches a GPU at import."""
from __future__ import annotations

import zlib

import numpy as np

from oracle import frame_ops_oracle as fo

FENCE_U8 = 0xA5
FENCE_F32 = -7.0
FENCE_I32 = -123456789
PAD = 4096                     # sentinel elements on either side of an output


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def image(h, w, *key):
    """smooth ramps over noise: neighbouring pixels differ, and an interpolation error of one index shows"""
    r = rng("image", h, w, *key)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 128 + 90 * np.sin(yy[..., None] / 7.0 + r.random(3) * 6) * np.cos(xx[..., None] / 5.0 + r.random(3) * 6)
    return np.clip(base + r.integers(-30, 31, (h, w, 3)), 1, 255).astype(np.uint8)      # no zero: padding is told apart


def virtual_crop(img, x1, y1, w, h):
    """the h x w window at (x1, y1): img inside, zeros outside"""
    out = np.zeros((h, w) + img.shape[2:], dtype=img.dtype)
    ys, xs = np.arange(h) + y1, np.arange(w) + x1
    my, mx = (ys >= 0) & (ys < img.shape[0]), (xs >= 0) & (xs < img.shape[1])
    out[np.ix_(my, mx)] = img[np.ix_(ys[my], xs[mx])]
    return out


def quarter_size(h, w):
    """(dw, dh) of cv2.resize(fx=0.25, fy=0.25): cvRound"""
    return int(round(w * 0.25)), int(round(h * 0.25))


def quarter_canvas(img, mode="edge"):
    """img cropped or padded to (4 dh, 4 dw): the unchanged oracle's resize of it to (dw, dh) is the fx=0.25 form of img when the
    padding replicates the edge (tests/test_face_ops.py::test_oracle_on_an_edge_replicated_canvas_is_the_quarter_scale_form)"""
    dw, dh = quarter_size(img.shape[0], img.shape[1])
    c = img[:4 * dh, :4 * dw]
    return np.pad(c, ((0, 4 * dh - c.shape[0]), (0, 4 * dw - c.shape[1]), (0, 0)), mode=mode), (dw, dh)


def expected_resize(img, dsize=None, fx=None):
    if fx is None:
        return fo.resize_linear_u8(img, dsize)
    assert fx == 0.25
    canvas, dsize = quarter_canvas(img)
    return fo.resize_linear_u8(canvas, dsize)


# (source (h, w), dsize (dw, dh) or None, fx or None): tests/test_face_ops_gpu.py runs each in batches of 1 and 3
RESIZE_CASES = {
    "quarter-308x372": ((308, 372), (93, 77), None),
    "fx-41x50": ((41, 50), None, 0.25),
    "fx-42x54": ((42, 54), None, 0.25),
    "fx-43x51": ((43, 51), None, 0.25),
    "upscale-7x5": ((7, 5), (23, 19), None),
    "identity-12x17": ((12, 17), (17, 12), None),
    "area-20x14": ((20, 14), (7, 10), None),
    "one-column-9x1": ((9, 1), (4, 5), None),
    "to-one-pixel-6x9": ((6, 9), (1, 1), None),
}


def _fenced(torch, n, dtype, fence):
    buf = torch.full((n + 2 * PAD,), fence, dtype=dtype, device="cuda:0")
    return buf, buf[PAD:PAD + n]


def _fence_ok(buf, n, fence):
    return bool((buf[:PAD] == fence).all()) and bool((buf[PAD + n:] == fence).all())


def run_resize(name, batch):
    """-> (got [B,dh,dw,3], want, the sentinels are untouched)"""
    import torch
    from calipsync_amd import face_ops
    (h, w), dsize, fx = RESIZE_CASES[name]
    src = np.stack([image(h, w, name, b) for b in range(batch)])
    want = np.stack([expected_resize(s, dsize, fx) for s in src])
    n = want.size
    buf, mid = _fenced(torch, n, torch.uint8, FENCE_U8)
    got = face_ops.resize_frames_u8(torch.from_numpy(src).to("cuda:0"), dsize=dsize, fx=fx, out=mid.view(want.shape))
    torch.cuda.synchronize()
    assert got.data_ptr() == mid.data_ptr()
    return got.cpu().numpy(), want, _fence_ok(buf, n, FENCE_U8)


# ------------------------------------------------------------------------------------------------ crops
CROP_FRAMES = (3, 230, 310)          # three frames of 230 x 310


def crop_frames():
    b, h, w = CROP_FRAMES
    return np.stack([image(h, w, "crop frame", i) for i in range(b)])


def crop_table(which):
    """geometry records (frame, x1, y1, w, h) over CROP_FRAMES"""
    from calipsync_amd.landmarks import LandmarkDetector
    _, fh, fw = CROP_FRAMES
    g = LandmarkDetector._crop_geometry
    if which == "one":
        return np.asarray([(1, 20, 10, 141, 141)], dtype=np.int32)
    if which == "kinds":
        rows = [(0,) + g(fh, fw, (30, 20, 135, 120)),          # 141: upscale
                (1,) + g(fh, fw, (40, 25, 183, 170)),          # a 183-pixel box: 192, the identity
                (2,) + g(fh, fw, (-30, -70, 366, 300)),        # a 366-pixel box: 384, the 2x area mean, over all four borders
                (0, -150, -200, 600, 600), (1, -900, -1000, 2104, 2104),      # mostly outside
                (0, -50, 40, 141, 141), (0, 250, 40, 100, 100), (0, 50, -60, 120, 120), (0, 50, 180, 120, 120),   # one per border
                (2, 400, 50, 90, 90),                          # wholly outside
                (1, -30, 100, 200, 130),                       # not square
                (2, 5, 7, 1, 1), (1, 100, 100, 192, 384), (0, 10, 10, 384, 192)]   # one pixel; one axis alone at 192 / 384: bilinear
        assert [r[3] for r in rows[:3]] == [141, 192, 384] and all(r[3] == r[4] for r in rows[:3])
        return np.asarray(rows, dtype=np.int32)
    if which == "many":                                        # more records than one launch carries
        r = rng("crop table many")
        return np.asarray([(int(r.integers(0, 3)), int(r.integers(-60, 300)), int(r.integers(-60, 220)), int(r.integers(1, 90)),
                            int(r.integers(1, 90))) for _ in range(70)], dtype=np.int32)
    raise KeyError(which)


def expected_crops(frames, table):
    return np.stack([fo.resize_linear_u8(virtual_crop(frames[f], x1, y1, w, h), (192, 192)) for f, x1, y1, w, h in table])


def run_crops(which):
    import torch
    from calipsync_amd import face_ops
    frames, table = crop_frames(), crop_table(which)
    want = expected_crops(frames, table)
    buf, mid = _fenced(torch, want.size, torch.uint8, FENCE_U8)
    got = face_ops.face_crops192(torch.from_numpy(frames).to("cuda:0"), table, out=mid.view(want.shape))
    torch.cuda.synchronize()
    return got.cpu().numpy(), want, _fence_ok(buf, want.size, FENCE_U8)


# ------------------------------------------------------------------------------------------------ candidates
def expected_candidates(det, thresh, cap):
    """numpy's mask-select per frame -> (counts, [rows of frame b, at most cap])"""
    counts, rows = [], []
    for d in det:
        sel = d[d[:, 0] > np.float32(thresh)]
        counts.append(len(sel))
        rows.append(sel[:cap])
    return np.asarray(counts, dtype=np.int32), rows


def run_candidates(det, thresh, cap):
    """det [B,P,5] float32 numpy -> (counts, rows [B,cap,5] with the sentinel where nothing was written, sentinels untouched)"""
    import torch
    from calipsync_amd import face_ops
    b = det.shape[0]
    cbuf, cmid = _fenced(torch, b, torch.int32, FENCE_I32)
    rbuf, rmid = _fenced(torch, b * cap * 5, torch.float32, FENCE_F32)
    counts, rows = face_ops.s3fd_candidates(torch.from_numpy(det.copy()).to("cuda:0"), thresh, cap, counts=cmid, rows=rmid.view(b, cap, 5))
    torch.cuda.synchronize()
    return counts.cpu().numpy(), rows.cpu().numpy(), _fence_ok(cbuf, b, FENCE_I32) and _fence_ok(rbuf, b * cap * 5, FENCE_F32)


def candidates_match(det, thresh, cap):
    """True when counts, the compacted rows (bit for bit, NaN included) and everything past them are as numpy has them"""
    counts, rows, fence = run_candidates(det, thresh, cap)
    want_counts, want_rows = expected_candidates(det, thresh, cap)
    ok = fence and np.array_equal(counts, want_counts)
    for b, w in enumerate(want_rows):
        ok = ok and np.array_equal(rows[b, :len(w)].view(np.uint32), w.view(np.uint32)) and bool((rows[b, len(w):] == FENCE_F32).all())
    return ok, want_counts


def synthetic_det(batch, p, *key):
    """scores uniform in [0, 1), boxes seeded: a stand-in for the detector's dense output (kernel ledger)"""
    r = rng("det", batch, p, *key)
    det = r.random((batch, p, 5)).astype(np.float32)
    det[..., 1:] = (det[..., 1:] * 2 - 0.5)
    return det


# ------------------------------------------------------------------------------------------------ finalize
def finalize_inputs(n):
    r = rng("finalize", n)
    y = (r.standard_normal((n, 220)) * 0.3).astype(np.float32)
    mean = r.random(220).astype(np.float32)
    table = np.asarray([(int(r.integers(0, 3)), int(r.integers(-2000, 2000)), int(r.integers(-2000, 2000)), int(r.integers(1, 2200)),
                         int(r.integers(1, 2200))) for _ in range(n)], dtype=np.int32)
    table[0, 1:3] = (-1000, -900)            # negative offsets whatever the seed
    return y, mean, table


def expected_landmarks(y, mean, table):
    """LandmarkDetector.landmarks_from_crops itself (its numpy loop) on these rows"""
    from calipsync_amd.landmarks import LandmarkDetector

    class Rows:
        def forward_u8(self, _crops):
            return y

    lm = object.__new__(LandmarkDetector)
    lm.mean_face, lm.pfld_backbone = mean, Rows()
    return np.stack(lm.landmarks_from_crops(None, [(int(t[3]), int(t[4])) for t in table], [(int(t[1]), int(t[2])) for t in table]))


def run_finalize(n):
    import torch
    from calipsync_amd import face_ops
    y, mean, table = finalize_inputs(n)
    want = expected_landmarks(y, mean, table)
    buf, mid = _fenced(torch, want.size, torch.int32, FENCE_I32)
    got = face_ops.landmarks_finalize(torch.from_numpy(y).to("cuda:0"), torch.from_numpy(mean).to("cuda:0"), table, out=mid.view(want.shape))
    torch.cuda.synchronize()
    return got.cpu().numpy(), want, _fence_ok(buf, want.size, FENCE_I32)
