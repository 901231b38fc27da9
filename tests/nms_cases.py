"""Shared by the tests of S3FD's NMS on the device (test_face_nms*.py, kernel_ledger_nms.py, the end-to-end tests): a seeded
generator of candidate rows, the expected values from the host code itself (facedet.detect_output, facedet.detect_faces_rows;
where stage 2 meets tied scores, facedet.nms_ restated with a stable argsort and nothing else changed), and a runner that puts
every output of casync_op_s3fd_nms into a sentinel-filled buffer.  Nothing here touches a GPU at import."""
from __future__ import annotations

import contextlib
import functools

import numpy as np

from calipsync_amd import facedet
from face_cases import FENCE_F32, FENCE_I32, _fence_ok, _fenced

FENCE_F64 = -7.0
TOP_K = facedet.TOP_K
WIDTH, HEIGHT, CONF_TH = 372, 308, 0.1          # the frame of tests/test_face_pipeline_gpu.py, S3FDDetector's default threshold

# (n, clusters, ties, seed): n = 1, 2: one and two rows; 64 / 65: a wave and one row over; 257: one row over a round of 256 lanes;
# 777: odd, three rounds and a part; 1024: the kernel's cap, once with few clusters and tied scores, once crowded.  The seeds are the
# first at which BOTH passes suppress rows from 64 rows on (faces < kept < n: tests/test_face_nms.py holds them to it) and at which
# a ties case still has tied scores in stage 2.
TABLE = ((1, 1, False, 0), (2, 1, False, 0), (64, 3, False, 1), (65, 4, True, 1), (257, 6, False, 0), (777, 40, False, 0),
         (1024, 12, True, 0), (1024, 300, False, 0))


def candidate_rows(n, clusters, ties=False, seed=0):
    """[n,5] float32 (score, x1, y1, x2, y2) in prior order, as casync_op_s3fd_candidates hands them over: `clusters` faces
    with centres in (0.15, 0.85) and a size of their own, every row one of them with a jittered centre and size"""
    r = np.random.default_rng([0x4E4D53, n, clusters, int(ties), seed])
    centre = r.uniform(0.15, 0.85, (clusters, 2))
    size = r.uniform(0.05, 0.25, (clusters, 1)) * np.array([0.5, 0.6])
    which = r.integers(0, clusters, n)
    c = centre[which] + r.normal(0.0, 0.012, (n, 2))
    half = size[which] * r.uniform(0.8, 1.25, (n, 1))
    score = r.uniform(0.0501, 0.999, n)
    if ties:
        score = np.maximum(np.round(score * 16.0), 1.0) / 16.0
    return np.concatenate([score[:, None], c - half, c + half], axis=1).astype(np.float32)


def nms_stable(dets, thresh):
    """facedet.nms_ (box_utils.py:7-38) with argsort(kind="stable"): among equal scores the higher index is visited first,
    where the default argsort leaves the order open.  Nothing else differs."""
    x1, y1, x2, y2, scores = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3], dets[:, 4]
    areas = (x2 - x1) * (y2 - y1)
    order = scores.argsort(kind="stable")[::-1]
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(int(i))
        xx1, yy1 = np.maximum(x1[i], x1[order[1:]]), np.maximum(y1[i], y1[order[1:]])
        xx2, yy2 = np.minimum(x2[i], x2[order[1:]]), np.minimum(y2[i], y2[order[1:]])
        w, h = np.maximum(0.0, xx2 - xx1), np.maximum(0.0, yy2 - yy1)
        inter = w * h
        with np.errstate(divide="ignore", invalid="ignore"):
            ovr = inter / (areas[i] + areas[order[1:]] - inter)
        order = order[np.where(ovr <= thresh)[0] + 1]
    return np.array(keep).astype(int)


@contextlib.contextmanager
def _stable_final_nms():
    real = facedet.nms_
    facedet.nms_ = nms_stable
    try:
        yield
    finally:
        facedet.nms_ = real


class Expected:
    """what the host code makes of one frame's candidate rows"""

    def __init__(self, rows, width=WIDTH, height=HEIGHT, conf_th=CONF_TH):
        rows = np.asarray(rows, dtype=np.float32).reshape(-1, 5)
        self.n = len(rows)
        out = facedet.detect_output(rows[None])[0]                          # [2,750,5]; class 0 stays zero
        mask = rows[:, 0] > np.float32(facedet.CONF_THRESH)
        assert mask.all(), "candidate rows are above CONF_THRESH by construction: the kernel takes every row it is given"
        self.detect_n = min(facedet.nms_f32(rows[mask, 1:], rows[mask, 0])[1], TOP_K)
        self.detect_out = out[1, :self.detect_n].copy()
        passing = 0
        while passing < TOP_K and out[1, passing, 0] > np.float32(conf_th):
            passing += 1
        self.passing = passing
        self.tied = len(np.unique(out[1, :passing, 0])) < passing
        try:
            with _stable_final_nms():
                self.faces = facedet.detect_faces_rows(out, width, height, conf_th)
            self.status = len(self.faces)
            if not self.tied:                                               # no tie: the host code as it is says the same
                assert np.array_equal(facedet.detect_faces_rows(out, width, height, conf_th), self.faces)
        except IndexError:
            self.faces, self.status = np.empty((0, 5)), -2


@functools.lru_cache(maxsize=None)
def table_case(n, clusters, ties, seed=0):
    """(rows, Expected) of one row of TABLE: computed once, never changed"""
    rows = candidate_rows(n, clusters, ties, seed)
    rows.setflags(write=False)
    return rows, Expected(rows)


# ------------------------------------------------------------------------------------------------ special frames
ZERO_AREA = np.array([0.5, 0.4, 0.5, 0.6], dtype=np.float32)             # x2 == x1
FAR_ZERO_AREA = np.array([-0.5, -0.5, -0.5, -0.4], dtype=np.float32)     # ... and one that touches nothing


def degenerate_rows():
    """two frames of 24 normal rows.  Frame 0 has three identical zero-area rows among them (scores 0.9, 0.8, 0.7): a zero-area
    row against a normal one has IoU 0 / area = 0 and survives; against its identical twin it is 0 / 0 = NaN, which `iou <= thr`
    drops, so one of the three is kept.  Frame 1 has one zero-area row far from everything (0.6), which survives with IoU 0
    throughout (two zero-area rows in one frame would be 0 / 0 to each other wherever they lie)."""
    rows = candidate_rows(24, 3, seed=7)
    twins = np.array([[0.9, *ZERO_AREA], [0.8, *ZERO_AREA], [0.7, *ZERO_AREA]], dtype=np.float32)
    return np.insert(rows, [3, 11, 11], twins, axis=0), np.insert(rows, [20], np.array([[0.6, *FAR_ZERO_AREA]], dtype=np.float32), axis=0)


def tied_clusters():
    """40 rows with ONE score: 8 disjoint clusters of 5 near-identical boxes, the clusters interleaved (row i is of cluster
    i % 8).  Visiting order among equal scores is the higher row index first, so stage 1 keeps rows 39, 38, ... 32; stage 2
    then meets eight tied rows."""
    r = np.random.default_rng(0x71ED)
    rows = np.empty((40, 5), dtype=np.float32)
    for i in range(40):
        cx, cy = 0.15 + 0.2 * (i % 4), 0.3 + 0.4 * ((i % 8) // 4)
        jx, jy = r.uniform(-0.002, 0.002, 2)
        rows[i] = (0.5, cx - 0.05 + jx, cy - 0.08 + jy, cx + 0.05 + jx, cy + 0.08 + jy)
    return rows


def disjoint_grid():
    """28 x 28 = 784 disjoint boxes, scores in (0.2, 0.9): stage 1 keeps 750 and every one of them is above conf_th 0.1, which
    is where the reference's walk runs off Detect.forward's [750,5] array"""
    r = np.random.default_rng(0x28)
    gy, gx = np.mgrid[0:28, 0:28].reshape(2, -1) / 28.0
    return np.column_stack([r.uniform(0.2, 0.9, 784), gx + 0.1 / 28, gy + 0.1 / 28, gx + 0.9 / 28, gy + 0.9 / 28]).astype(np.float32)


def run_nms(frames, cap, width=WIDTH, height=HEIGHT, conf_th=CONF_TH, counts=None):
    """frames: per frame its [n,5] rows (n <= cap, or the first cap of more with counts[b] saying how many there were).  ->
    dict of numpy arrays status [B], faces [B,750,5], detect_out [B,750,5], detect_n [B], each still holding the sentinel where
    the kernel wrote nothing, and fence = the sentinels around all four are untouched.  Candidate rows behind a frame's count are
    NaN: reading one shows."""
    import torch
    from calipsync_amd import face_ops
    b = len(frames)
    rows = np.full((b, cap, 5), np.nan, dtype=np.float32)
    for i, f in enumerate(frames):
        rows[i, :len(f)] = f
    counts = np.asarray([len(f) for f in frames] if counts is None else counts, dtype=np.int32)
    sbuf, smid = _fenced(torch, b, torch.int32, FENCE_I32)
    nbuf, nmid = _fenced(torch, b, torch.int32, FENCE_I32)
    fbuf, fmid = _fenced(torch, b * TOP_K * 5, torch.float64, FENCE_F64)
    dbuf, dmid = _fenced(torch, b * TOP_K * 5, torch.float32, FENCE_F32)
    got = face_ops.s3fd_nms(torch.from_numpy(counts).to("cuda:0"), torch.from_numpy(rows).to("cuda:0"), width, height, conf_th, status=smid,
                            faces=fmid.view(b, TOP_K, 5), detect_out=dmid.view(b, TOP_K, 5), detect_n=nmid)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == smid.data_ptr() and got[1].data_ptr() == fmid.data_ptr()
    fence = _fence_ok(sbuf, b, FENCE_I32) and _fence_ok(nbuf, b, FENCE_I32) and _fence_ok(fbuf, b * TOP_K * 5, FENCE_F64) and \
        _fence_ok(dbuf, b * TOP_K * 5, FENCE_F32)
    return {"status": got[0].cpu().numpy(), "faces": got[1].cpu().numpy(), "detect_out": got[2].cpu().numpy(), "detect_n": got[3].cpu().numpy(),
            "fence": fence}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def frame_differences(got, b, want):
    """the number of elements of frame b that differ from the host's, bit for bit, counting every row behind status / detect_n
    that lost its sentinel; want None: a frame the kernel must not have touched at all (status -1 aside)"""
    if want is None:
        return int(got["status"][b] != -1) + int(got["detect_n"][b] != FENCE_I32) + int((got["faces"][b] != FENCE_F64).sum()) + \
            int((got["detect_out"][b] != FENCE_F32).sum())
    bad = int(got["status"][b] != want.status) + int(got["detect_n"][b] != want.detect_n)
    k, m = max(want.status, 0), want.detect_n
    bad += int((_bits(got["faces"][b, :k]) != _bits(want.faces)).sum()) + int((got["faces"][b, k:] != FENCE_F64).sum())
    bad += int((_bits(got["detect_out"][b, :m]) != _bits(want.detect_out)).sum()) + int((got["detect_out"][b, m:] != FENCE_F32).sum())
    return bad
