"""The bf16 precision of the S3FD handle without a GPU: the precision argument, the workspace of each precision, and the bar
file tests/golden/s3fd_bf16_bar.npz (the reference under autocast against its own float64 run; written by
tests/golden/make_s3fd_bf16_bar.py) -- tied to tests/golden/s3fd_b2.npz, its own conditions re-asserted from its contents, and
the host post-processing run on its stored float32 dense tensors bit for bit against the reference's faces."""
import ctypes
import os

import numpy as np
import pytest

from calipsync_amd import _lib, facedet, recipe
from conftest import GOLDEN

H, W, P = 77, 93, 596
STAT_KEYS = facedet.STAGES[:9] + ("loc", "conf", "dlogit", "score", "box")


@pytest.fixture(scope="module")
def lib():
    from calipsync_amd import build
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def bar():
    return np.load(os.path.join(GOLDEN, "s3fd_bf16_bar.npz"))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "s3fd_b2.npz"))


# ---- the precision argument ---------------------------------------------------------------------------------------------------
def test_create_ex_refuses_an_unknown_precision_before_any_device_call(lib):
    for precision in (2, -1):
        h = ctypes.c_void_p(1)
        assert lib.casync_s3fd_create_ex(0, precision, ctypes.byref(h)) == -1           # CASYNC_ERR_ARG, not _NO_DEVICE
        assert h.value is None
        assert f"precision {precision}".encode() in lib.casync_last_error()
    assert lib.casync_s3fd_precision(None) == -1
    assert _lib.ABI_VERSION == 13 == lib.casync_abi_version()


def test_engine_and_detector_refuse_an_unknown_precision_name():
    sd = {}                                                      # (the name is looked at before the checkpoint)
    for bad in ("fp16", "BF16", 1):
        with pytest.raises(ValueError, match="precision"):
            facedet.S3FDEngine(sd, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            facedet.S3FDDetector(state_dict=sd, precision=bad)
    assert facedet.PRECISIONS == {"fp32": 0, "bf16": 1}


# ---- the workspace ----------------------------------------------------------------------------------------------------------------
def test_bf16_workspace_is_about_half_and_zero_where_fp32_refuses(lib):
    ws = lib.casync_s3fd_workspace_bytes_ex
    for b, h, w in ((1, H, W), (3, H, W), (1, 64, 64), (8, 270, 480), (16, 270, 480)):
        f32, b16 = ws(0, b, h, w), ws(1, b, h, w)
        assert f32 == lib.casync_s3fd_workspace_bytes(b, h, w) > 0
        assert 0 < b16 < f32 and b16 % 256 == 0
        # activations and the im2col matrix halve, loc and conf stay fp32 (24 bytes a prior), every part on a 256-B boundary
        assert f32 / 2 <= b16 <= f32 / 2 + 12 * b * facedet.n_priors(h, w) + 5 * 256, (b, h, w, f32, b16)
    for b, h, w in ((1, 8, 8), (1, 15, 64), (0, H, W), (1, 9000, 64), (65537, H, W), (1, 0, 5)):
        assert ws(0, b, h, w) == 0 == ws(1, b, h, w) == lib.casync_s3fd_workspace_bytes(b, h, w), (b, h, w)
    assert ws(2, 1, H, W) == 0 == ws(-1, 1, H, W)
    # the 2 GiB rule on the bf16 byte sizes: conv1's output of 130 frames of 270 x 480 passes 2 GiB at two bytes a value
    assert 129 * 270 * 480 * 64 * 2 < 2 ** 31 <= 130 * 270 * 480 * 64 * 2
    assert ws(1, 130, 270, 480) == ws(1, 129, 270, 480) > ws(1, 128, 270, 480)
    assert ws(0, 65, 270, 480) == ws(0, 64, 270, 480)


# ---- the bar file ----------------------------------------------------------------------------------------------------------------
def test_bar_file_is_tied_to_the_fp32_fixture(bar, fx):
    tie = float(bar["c1.fp32_vs_fixture"])
    ref_err = max(float(fx[f"ref_err.{n}"]) for n in facedet.STAGES[:9] + ("loc", "conf", "det"))
    assert 0 <= tie <= ref_err, (tie, ref_err)
    for prefix in ("c1", "c2.0", "c2.1"):
        for n in STAT_KEYS:
            mx, mean = bar[f"{prefix}.{n}"]
            assert 0 < mean <= mx < 1.0, (prefix, n)
    # autocast's error is a bf16 error: orders above the reference's float32 error on the same frames
    assert float(bar["c1.conv5_3"][0]) > 1000 * float(fx["ref_err.conv5_3"])


def _logit(p):
    return float(np.log(p / (1.0 - p)))


def _iou_matrix(b):
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(0.0, np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]))
    h = np.maximum(0.0, np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]))
    return w * h / (area[:, None] + area[None, :] - w * h)


@pytest.mark.parametrize("i", [0, 1])
def test_stable_frames_meet_their_conditions(bar, i):
    d32 = bar[f"c2.det32.{i}"]
    assert d32.shape == (P, 5) and d32.dtype == np.float32 and bar[f"c2.det64.{i}"].dtype == np.float64
    # 1. score margins, from the stored scores (the face-logit difference is logit(score))
    s = d32[:, 0].astype(np.float64)
    dl = np.log(s) - np.log1p(-s)
    margin = min(float(np.abs(dl - _logit(th)).min()) for th in (0.05, 0.1, 0.8))
    assert abs(margin - float(bar[f"c2.margin_logit.{i}"])) < 1e-3
    assert float(bar[f"c2.margin_logit.{i}"]) > 1.5 * float(bar[f"c2.dlogit_err.{i}"]) == 1.5 * float(bar[f"c2.{i}.dlogit"][0])
    # 2. IoU margins among the priors above 0.03
    sel = np.nonzero(d32[:, 0] > 0.03)[0]
    iou = _iou_matrix(d32[sel, 1:].astype(np.float64))[np.triu_indices(sel.size, 1)]
    assert float(bar[f"c2.margin_iou.{i}"]) == min(float(np.abs(iou - th).min()) for th in (0.3, 0.1))
    assert float(bar[f"c2.margin_iou.{i}"]) > 4.0 * float(bar[f"c2.iou_change.{i}"]) > 0
    # 3. non-trivial
    assert len(bar[f"c2.faces01.{i}"]) >= 2 and len(bar[f"c2.faces08.{i}"]) >= 1
    assert len(bar[f"c2.priors01.{i}"]) == len(bar[f"c2.faces01.{i}"]) and len(bar[f"c2.priors08.{i}"]) == len(bar[f"c2.faces08.{i}"])
    assert 0 < float(bar[f"c2.displacement.{i}"]) < 1.0
    # the fourth figure is recorded as measured (tests/golden/make_s3fd_bf16_bar.py says why it cannot be a condition)
    xywh = bar[f"c2.boxes.{i}"]
    assert float(bar[f"c2.crop_margin.{i}"]) == float(np.abs(xywh - np.round(xywh)).min())
    assert int(bar[f"c2.crop_condition.{i}"]) == int(float(bar[f"c2.crop_margin.{i}"]) > float(bar[f"c2.displacement.{i}"]))


@pytest.mark.parametrize("i", [0, 1])
def test_stable_frames_regenerate_and_post_processing_equals_the_references_faces(bar, i):
    seed = int(bar["c2.seeds"][i])
    frame = recipe.make_s3fd_inputs(1, H, W, seed=seed)[0]
    assert np.array_equal(frame, bar[f"c2.frame.{i}"])
    d32 = bar[f"c2.det32.{i}"]
    detect = facedet.detect_output(d32[None])[0]
    assert np.array_equal(detect, bar[f"c2.detect32.{i}"])
    for tag, th in (("01", 0.1), ("08", 0.8)):
        rows = facedet.detect_faces_rows(detect, W, H, th)
        want = bar[f"c2.faces{tag}.{i}"]
        assert rows.dtype == np.float64 and np.array_equal(rows, want), (tag, i)
        priors = [int(np.argmin(np.abs(d32[:, 0] - s))) for s in rows[:, 4]]
        assert priors == list(bar[f"c2.priors{tag}.{i}"])

    class Dense:
        def forward_u8(self, frames):
            return d32[None]

    det = facedet.S3FDDetector.__new__(facedet.S3FDDetector)
    det.conf_threshold, det.scale, det.last_detection, det.det_net = 0.1, 1, None, Dense()
    boxes, idx = det.detect([frame])[0]
    assert np.array_equal(boxes, bar[f"c2.boxes.{i}"]) and idx == list(range(len(boxes)))
