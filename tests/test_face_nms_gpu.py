"""-m gpu: casync_op_s3fd_nms (csrc/face_nms.hip) against the host code it replaces, bit for bit: status, faces, and the
stage-1 rows detect_out / detect_n, every output in a sentinel-filled buffer that must stay untouched past its end and past the
rows a frame's status / detect_n name.  Cases and expected values are in tests/nms_cases.py (facedet.detect_output and
facedet.detect_faces_rows on the same rows).  Then the detector end to end: S3FDDetector.detect_device with nms="device" against
nms="host" and against detect() with the oracle's resize, on the 308 x 372 frames of tests/test_face_pipeline_gpu.py."""
import numpy as np
import pytest
import torch

import nms_cases as nc
from calipsync_amd import face_ops, facedet, landmarks, recipe
from oracle import frame_ops_oracle as fo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _check(got, wants):
    assert got["fence"], "a sentinel around an output changed"
    for b, want in enumerate(wants):
        bad = nc.frame_differences(got, b, want)
        print(f"frame {b}: status {got['status'][b]}, detect_n {got['detect_n'][b]}: {bad} elements differ")
        assert bad == 0, (b, got["status"][b], None if want is None else want.status)


# ---------------------------------------------------------------------------------------------- the operator
@pytest.mark.parametrize("case", nc.TABLE, ids=[f"n{c[0]}-c{c[1]}{'-ties' if c[2] else ''}" for c in nc.TABLE])
def test_a_frame_alone_is_the_host_codes_result(case):
    rows, want = nc.table_case(*case)
    got = nc.run_nms([rows], len(rows))
    print(f"n {len(rows)}: stage 1 keeps {want.detect_n}, {want.passing} pass, {want.status} faces")
    _check(got, [want])


def test_a_batch_of_four_with_an_empty_frame_equals_its_frames_alone():
    cases = [nc.table_case(*nc.TABLE[i]) for i in (3, 6, 1)]                 # 65, 1024 and 2 rows
    frames = [nc.candidate_rows(0, 1)] + [c[0] for c in cases]
    assert [len(f) for f in frames] == [0, 65, 1024, 2]
    got = nc.run_nms(frames, 1024)
    assert got["status"][0] == 0 and got["detect_n"][0] == 0
    _check(got, [nc.Expected(frames[0])] + [c[1] for c in cases])
    for b in (1, 2, 3):                                                      # ... and the same frame run alone, with its own cap
        alone = nc.run_nms([frames[b]], len(frames[b]))
        k, m = alone["status"][0], alone["detect_n"][0]
        assert k == got["status"][b] and m == got["detect_n"][b]
        assert np.array_equal(alone["faces"][0, :k].view(np.uint64), got["faces"][b, :k].view(np.uint64))
        assert np.array_equal(alone["detect_out"][0, :m].view(np.uint32), got["detect_out"][b, :m].view(np.uint32))


def test_a_frame_over_the_cap_is_left_alone_and_the_others_are_right():
    cases = [nc.table_case(*nc.TABLE[i]) for i in (2, 4, 3)]                 # 64, 257 and 65 rows
    cap = 100
    frames = [c[0][:cap] for c in cases]
    got = nc.run_nms(frames, cap, counts=[64, 257, 65])
    assert got["status"].tolist()[1] == -1
    _check(got, [cases[0][1], None, cases[2][1]])
    # a count of exactly cap is still taken
    rows = cases[1][0][:cap]
    _check(nc.run_nms([rows], cap), [nc.Expected(rows)])


def test_zero_area_rows_drop_their_twins_and_survive_alone():
    twins, far = nc.degenerate_rows()
    wants = [nc.Expected(twins), nc.Expected(far)]
    got = nc.run_nms([twins, far], 32)
    _check(got, wants)
    for b, box in enumerate((nc.ZERO_AREA, nc.FAR_ZERO_AREA)):
        kept = got["detect_out"][b, :got["detect_n"][b], 1:]
        assert (kept == box).all(axis=1).sum() == 1


def test_equal_scores_are_visited_from_the_higher_row_index():
    tied = nc.tied_clusters()
    want = nc.Expected(tied)
    got = nc.run_nms([tied], 40)
    _check(got, [want])
    assert got["detect_n"][0] == 8 and np.array_equal(got["detect_out"][0, :8], tied[39:31:-1])


def test_750_rows_above_the_threshold_are_the_references_index_error():
    grid = nc.disjoint_grid()
    want = nc.Expected(grid)
    assert want.status == -2 and want.detect_n == 750
    got = nc.run_nms([grid, grid[:700]], 1024)
    _check(got, [want, nc.Expected(grid[:700])])
    assert got["status"].tolist() == [-2, 700]


def test_the_same_call_twice_gives_identical_bytes():
    frames = [nc.table_case(*nc.TABLE[i])[0] for i in (7, 5, 6)]
    a, b = nc.run_nms(frames, 1024), nc.run_nms(frames, 1024)
    for key in ("status", "detect_n", "faces", "detect_out"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_the_wrapper_allocates_and_skips_stage_one_outputs():
    rows, want = nc.table_case(*nc.TABLE[4])
    counts = torch.tensor([len(rows)], dtype=torch.int32, device=DEV)
    status, faces = face_ops.s3fd_nms(counts, torch.from_numpy(rows.copy()).to(DEV)[None], nc.WIDTH, nc.HEIGHT, nc.CONF_TH)
    assert tuple(faces.shape) == (1, 750, 5) and faces.dtype == torch.float64 and int(status[0]) == want.status
    assert np.array_equal(faces[0, :want.status].cpu().numpy(), want.faces)
    with pytest.raises(ValueError, match="1..1024"):
        face_ops.s3fd_nms(counts, torch.zeros((1, 1025, 5), device=DEV), nc.WIDTH, nc.HEIGHT, nc.CONF_TH)
    with pytest.raises(ValueError, match="counts must be 1 int32"):
        face_ops.s3fd_nms(counts.long(), torch.zeros((1, 8, 5), device=DEV), nc.WIDTH, nc.HEIGHT, nc.CONF_TH)


# ---------------------------------------------------------------------------------------------- the detector, end to end
H, W = 77, 93


@pytest.fixture(scope="module")
def frames():
    f = np.repeat(np.repeat(recipe.make_s3fd_inputs(2), 4, 1), 4, 2)
    assert f.shape == (2, 4 * H, 4 * W, 3)
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def detectors():
    sd = recipe.make_s3fd_state_dict()
    out = {p: facedet.S3FDDetector(state_dict=sd, scale=0.25, device=DEV, precision=p, nms="device") for p in ("fp32", "bf16")}
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
        assert ia == ib and ba.dtype == bb.dtype and ba.shape == bb.shape and np.array_equal(ba, bb)


def _detect_device(det, nms, frames_in):
    """detect_device with the NMS in `nms`, from a detector that has seen nothing before"""
    det.nms, det.last_detection = nms, None
    try:
        return det.detect_device(frames_in)
    finally:
        det.nms = "device"


def _detect(det, frames_in):
    det.last_detection = None
    return det.detect(frames_in)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_detect_device_is_the_same_with_the_nms_on_either_side(detectors, frames, oracle_resizes, precision):
    det = detectors[precision]
    assert det.nms == "device"
    host = _detect(det, list(frames))
    assert sum(len(i) for _, i in host) >= 2
    resident = torch.from_numpy(frames.copy()).to(DEV)
    for frames_in in (resident, list(frames)):                              # resident frames, host frames (one pinned upload)
        on_device, on_host = _detect_device(det, "device", frames_in), _detect_device(det, "host", frames_in)
        _same_detections(on_device, on_host)
        _same_detections(on_device, host)
    _same_detections(_detect_device(det, "device", [frames[1]]), _detect(det, [frames[1]]))       # a frame alone
    # a cap below a frame's count: status -1, that frame goes through the host code on its dense rows
    dense = det.dense_device(list(frames)).cpu().numpy()
    counts = [int((d[:, 0] > np.float32(facedet.CONF_THRESH)).sum()) for d in dense]
    det.candidate_cap = max(1, min(counts) - 1)
    try:
        _same_detections(_detect_device(det, "device", list(frames)), host)
        _same_detections(_detect_device(det, "host", list(frames)), host)
    finally:
        det.candidate_cap = 1024
    det.nms = "nowhere"
    try:
        with pytest.raises(ValueError, match="nms 'nowhere'"):
            det.detect_device(list(frames))
    finally:
        det.nms = "device"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_frame_without_a_face_takes_the_last_detection_on_both_sides(detectors, frames, oracle_resizes, precision):
    det = detectors[precision]
    best = [float(facedet.detect_output(d[None])[0][1, 0, 0]) for d in det.dense(list(frames))]      # the host's own best score per frame
    assert best[0] != best[1] and min(best) > 0.05
    order = [0, 1] if best[0] > best[1] else [1, 0]                         # the frame with the better face first
    seq = [frames[i] for i in order]
    old = det.conf_threshold
    det.conf_threshold = min(best)                                          # nothing of the second frame is above it, the first has some
    try:
        host = _detect(det, seq)
        assert len(host[0][1]) >= 1 and host[1] is host[0]                  # the fallback: the second frame is handed the first's detection
        for nms in ("device", "host"):
            got = _detect_device(det, nms, seq)
            _same_detections(got, host)
            assert got[1] is got[0]
        # the other way round there is nothing to fall back on
        got = _detect_device(det, "device", seq[::-1])
        assert len(got[0][1]) == 0 and got[0][0].size == 0
        _same_detections(got, _detect(det, seq[::-1]))
    finally:
        det.conf_threshold = old


def test_the_detector_raises_the_references_index_error(detectors):
    """detect_device's code behind the candidate rows, on rows that make the host walk raise: the 28 x 28 grid"""
    det = detectors["fp32"]
    grid = nc.disjoint_grid()
    first = np.zeros_like(grid)
    first[:64] = nc.table_case(*nc.TABLE[2])[0]
    rows = torch.from_numpy(np.stack([first, grid])).to(DEV)
    counts = torch.tensor([64, 784], dtype=torch.int32, device=DEV)
    dense = torch.zeros((2, 8, 5), device=DEV)
    det.last_detection = None
    with pytest.raises(IndexError):
        det._faces_device(dense, counts, rows, nc.WIDTH, nc.HEIGHT)
    assert det.last_detection is not None                                   # frame 0 was taken before frame 1 raised, as in the host loop
    det.last_detection = None


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_landmarks_device_with_the_nms_on_the_device_equal_the_host_path(detectors, lm, frames, oracle_resizes, precision):
    det = detectors[precision]
    det.last_detection = None
    lm.face_detector = det
    try:
        host = lm.detect_landmarks(list(frames))
        assert all(f is not None and len(f) >= 1 for f in host)
        for frames_in in (list(frames), torch.from_numpy(frames.copy()).to(DEV)):
            det.last_detection = None
            got = lm.detect_landmarks_device(frames_in)
            assert len(got) == len(host)
            for fa, fb in zip(got, host):
                assert len(fa) == len(fb) and all(a.dtype == np.int32 and np.array_equal(a, b) for a, b in zip(fa, fb))
    finally:
        lm.face_detector = None
