"""-m gpu: frames resident on the device to int32 landmarks (S3FDDetector.detect_device, LandmarkDetector.
detect_landmarks_device), held bit for bit to the host path with the oracle's resize_linear_u8 put in place of cv2 / Pillow
(facedet.resize_scale and landmarks.resize192 monkeypatched).  The frames are the recipe's two 77 x 93 detector frames
replicated 4x to 308 x 372: at the reference's scale 0.25 the network sees the recipe frames themselves
(tests/test_face_ops.py, fact (a)), so the fixture's detections, times 4, are the expected boxes."""
import os

import numpy as np
import pytest
import torch

from calipsync_amd import face_ops, facedet, landmarks, recipe
from conftest import GOLDEN
from oracle import frame_ops_oracle as fo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W = 77, 93
# explicit (x, y, w, h) boxes per frame: crops of 141 (upscale), 192 (identity), 384 (2x area) and 2106 pixels, the last two
# far over the borders of the 308 x 372 frame; one not square once cut (it misses the frame on the left); frame 1 has its own
BOXES = [[(100, 80, 135, 120), (50, 40, 183, 170), (-20, -30, 366, 300), (-800, -900, 2006, 1500), (-260, 100, 120, 90)],
         [(300, 250, 100, 140), (10.6, 20.9, 150.2, 135.7)]]


@pytest.fixture(scope="module")
def frames():
    f = np.repeat(np.repeat(recipe.make_s3fd_inputs(2), 4, 1), 4, 2)
    assert f.shape == (2, 4 * H, 4 * W, 3)
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def sd():
    return recipe.make_s3fd_state_dict()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "s3fd_b2.npz"))


@pytest.fixture(scope="module")
def detectors(sd):
    out = {p: facedet.S3FDDetector(state_dict=sd, scale=0.25, device=DEV, precision=p) for p in ("fp32", "bf16")}
    yield out
    for d in out.values():
        d.release()


@pytest.fixture(scope="module")
def lm():
    return landmarks.LandmarkDetector(state_dict=recipe.make_pfld_state_dict(), mean_face=np.full(220, 0.5, np.float32), device=DEV)


@pytest.fixture
def oracle_resizes(monkeypatch):
    """the host path with OpenCV's arithmetic as the oracle restates it, whatever cv2 / Pillow this box has"""
    monkeypatch.setattr(facedet, "resize_scale", lambda img, s: fo.resize_linear_u8(img, face_ops.scaled_size(img.shape[0], img.shape[1], s)))
    monkeypatch.setattr(landmarks, "resize192", lambda crop: fo.resize_linear_u8(crop, (192, 192)))


def _same_detections(a, b):
    assert len(a) == len(b)
    for (ba, ia), (bb, ib) in zip(a, b):
        assert ia == ib and ba.dtype == bb.dtype and np.array_equal(ba, bb)


def _same_landmarks(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert (fa is None) == (fb is None)
        if fa is not None:
            assert len(fa) == len(fb)
            for la, lb in zip(fa, fb):
                assert la.dtype == lb.dtype == np.int32 and la.shape == lb.shape == (110, 2) and np.array_equal(la, lb)


def test_detect_device_returns_the_fixtures_boxes_times_four(detectors, frames, fx):
    det = detectors["fp32"]
    got = det.detect_device(torch.from_numpy(frames.copy()).to(DEV))
    tol = 4.0 * float(fx["ref_err.box"]) * 4 * max(W, H)
    assert len(got) == 2
    for i, (boxes, idx) in enumerate(got):
        want = fx[f"detect.{i}.boxes"] * 4.0
        assert boxes.shape == want.shape and boxes.dtype == np.float64 and idx == list(fx[f"detect.{i}.indices"])
        d = np.abs(boxes - want).max()
        print(f"frame {i}: {len(idx)} boxes, max|d| {d:.3e} pixel (bar {tol:.3e})")
        assert d <= tol


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_detect_device_equals_detect_with_the_oracles_resize(detectors, frames, oracle_resizes, precision):
    det = detectors[precision]
    host = det.detect(list(frames))
    resident = det.detect_device(torch.from_numpy(frames.copy()).to(DEV))
    from_host = det.detect_device(list(frames))                         # numpy frames: one pinned upload
    _same_detections(resident, host)
    _same_detections(from_host, host)
    assert sum(len(i) for _, i in host) >= 2
    # a frame of a batch is the frame alone; the dense output stays on the device
    _same_detections(det.detect_device([frames[1]]), host[1:])
    dense = det.dense_device(list(frames))
    assert dense.is_cuda and tuple(dense.shape) == (2, 596, 5)
    assert all(np.array_equal(a, b) for a, b in zip(dense.cpu().numpy(), det.dense(list(frames))))
    # a cap below a frame's count: that frame falls back to its dense rows, the result is the same
    counts = [(d[:, 0] > np.float32(facedet.CONF_THRESH)).sum() for d in dense.cpu().numpy()]
    det.candidate_cap = max(1, int(min(counts)) - 1)
    try:
        _same_detections(det.detect_device(list(frames)), host)
    finally:
        det.candidate_cap = 1024


def test_mixed_sizes_name_the_host_path(detectors, frames):
    with pytest.raises(ValueError, match="mixed sizes go through detect / dense"):
        detectors["fp32"].detect_device([frames[0], frames[1][:-4]])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_landmarks_device_with_the_detector_equal_the_host_path(detectors, lm, frames, oracle_resizes, precision):
    lm.face_detector = detectors[precision]
    try:
        host = lm.detect_landmarks(list(frames))
        _same_landmarks(lm.detect_landmarks_device(list(frames)), host)
        _same_landmarks(lm.detect_landmarks_device(torch.from_numpy(frames.copy()).to(DEV)), host)
        assert all(f is not None and len(f) >= 1 for f in host)
    finally:
        lm.face_detector = None


def test_landmarks_device_with_explicit_boxes_equal_the_host_path(lm, frames, oracle_resizes):
    widths = [lm._crop_geometry(4 * H, 4 * W, b)[2] for b in BOXES[0]]
    assert widths[:4] == [141, 192, 384, 2106] and lm._crop_geometry(4 * H, 4 * W, BOXES[0][4])[2:] != (126, 126)
    host = lm.detect_landmarks(list(frames), boxes=BOXES)
    got = lm.detect_landmarks_device(list(frames), boxes=BOXES)
    _same_landmarks(got, host)
    assert [len(f) for f in got] == [5, 2]
    # a frame of a batch equals the frame alone
    _same_landmarks(lm.detect_landmarks_device([frames[1]], boxes=BOXES[1:]), host[1:])
    _same_landmarks(lm.detect_landmarks_device(torch.from_numpy(frames[:1].copy()).to(DEV), boxes=BOXES[:1]), host[:1])
    # a frame without a box gives None, as on the host
    for boxes in ([BOXES[0], None], [[], BOXES[1]], [None, None]):
        host_n = lm.detect_landmarks(list(frames), boxes=boxes)
        got_n = lm.detect_landmarks_device(list(frames), boxes=boxes)
        _same_landmarks(got_n, host_n)
        assert [f is None for f in got_n] == [not b for b in boxes]
    with pytest.raises(ValueError, match="no boxes and no face_detector"):
        lm.detect_landmarks_device(list(frames))


def test_a_unet_forward_before_and_after_the_device_pipeline_is_unchanged(detectors, lm, frames, recipe_sd, golden):
    from calipsync_amd.unet import Model
    net = Model(6, "hubert").to(DEV)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe_sd.items()})
    net.eval()
    x, a = recipe.make_inputs(2)
    xd, ad = torch.from_numpy(x).to(DEV), torch.from_numpy(a).to(DEV)
    before = net(xd, ad).clone()
    lm.face_detector = detectors["bf16"]
    try:
        first = lm.detect_landmarks_device(list(frames))
        after = net(xd, ad).clone()
        second = lm.detect_landmarks_device(list(frames))
    finally:
        lm.face_detector = None
    torch.cuda.synchronize()
    assert torch.equal(before, after)
    assert np.abs(after.cpu().numpy() - golden["out.full"]).max() < 1e-3
    _same_landmarks(first, second)
