"""S3FD's NMS on the device, the parts that need no GPU: the symbol and its argument checks (refused before any device call),
the seventh object directory, the keyword of S3FDDetector, and what tests/test_face_nms_gpu.py leans on in tests/nms_cases.py:
the stable restatement of nms_ is nms_ where no score is tied, both passes suppress rows in every table case, and the host code
itself raises IndexError on the 28 x 28 grid."""
import ctypes as C
import os

import numpy as np
import pytest

import nms_cases as nc
from calipsync_amd import _lib, build, face_ops, facedet


def test_the_symbol_is_exported_and_bound_and_the_abi_version_is_unchanged():
    assert "casync_op_s3fd_nms" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.casync_op_s3fd_nms.restype is C.c_int and len(lib.casync_op_s3fd_nms.argtypes) == 12
    assert _lib.ABI_VERSION == 13 and lib.casync_abi_version() == 13
    header = open(os.path.join(os.path.dirname(build.HERE), "include", "casync_hip.h")).read()
    assert "casync_op_s3fd_nms(" in header and "#define CASYNC_ABI_VERSION 13" in header


def test_seventh_object_directory_is_part_of_the_build(monkeypatch):
    others = (build.OBJ_DIR, build.OBJ_DIR_HB16, build.OBJ_DIR_LMK, build.OBJ_DIR_DET, build.OBJ_DIR_DET16, build.OBJ_DIR_FACE)
    assert build.OBJ_DIR_NMS == os.path.join(build.LIB_DIR, "obj_nms") and build.OBJ_DIR_NMS not in others and len(set(others)) == 6
    assert build.SOURCES_NMS == ["face_nms.hip"] and "face_nms.hip" in build.SOURCES
    assert "face_nms.hip" not in build.SOURCES_HB16 + build.SOURCES_LMK + build.SOURCES_DET + build.SOURCES_DET16 + build.SOURCES_FACE
    assert os.path.exists(os.path.join(build.CSRC, "face_nms.hip"))
    with_nms = build.source_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "face_nms.hip"])
    assert build.source_hash() != with_nms


# ---------------------------------------------------------------------------------------------- argument checks
@pytest.fixture(scope="module")
def host():
    """a host buffer standing in for device pointers: a refused call never touches it"""
    buf = (C.c_uint8 * 4096)()
    return _lib.load(), C.addressof(buf), buf


def _refused(lib, status, *words):
    assert status == -1
    msg = lib.casync_last_error().decode()
    assert all(w in msg for w in words), msg


def test_nms_refuses_bad_arguments_before_any_device_call(host):
    lib, p, _ = host
    nms = lib.casync_op_s3fd_nms
    _refused(lib, nms(None, p, 1, 16, 372, 308, 0.1, p, p, None, None, None), "s3fd_nms", "null")
    _refused(lib, nms(p, None, 1, 16, 372, 308, 0.1, p, p, None, None, None), "s3fd_nms", "null")
    _refused(lib, nms(p, p, 1, 16, 372, 308, 0.1, None, p, None, None, None), "s3fd_nms", "null")
    _refused(lib, nms(p, p, 1, 16, 372, 308, 0.1, p, None, None, None, None), "s3fd_nms", "null")
    _refused(lib, nms(p, p, 1, 16, 372, 308, 0.1, p, p, p, None, None), "s3fd_nms", "detect_out and detect_n")
    _refused(lib, nms(p, p, 1, 16, 372, 308, 0.1, p, p, None, p, None), "s3fd_nms", "detect_out and detect_n")
    _refused(lib, nms(p, p, 0, 16, 372, 308, 0.1, p, p, None, None, None), "s3fd_nms", "batch 0")
    _refused(lib, nms(p, p, 65536, 16, 372, 308, 0.1, p, p, None, None, None), "s3fd_nms", "batch 65536")
    _refused(lib, nms(p, p, -1, 16, 372, 308, 0.1, p, p, None, None, None), "s3fd_nms", "batch -1")
    _refused(lib, nms(p, p, 1, 0, 372, 308, 0.1, p, p, None, None, None), "s3fd_nms", "cap 0")
    _refused(lib, nms(p, p, 1, 1025, 372, 308, 0.1, p, p, None, None, None), "s3fd_nms", "cap 1025", "1024")
    _refused(lib, nms(p, p, 1, 16, 0, 308, 0.1, p, p, None, None, None), "s3fd_nms", "0 x 308")
    _refused(lib, nms(p, p, 1, 16, 372, -2, 0.1, p, p, None, None, None), "s3fd_nms", "372 x -2")


def test_the_wrapper_refuses_host_tensors_and_wrong_shapes():
    import torch
    with pytest.raises(ValueError, match="rows must be a float32"):
        face_ops.s3fd_nms(torch.zeros(1, dtype=torch.int32), torch.zeros(1, 8, 5), 372, 308, 0.1)
    with pytest.raises(ValueError, match="rows must be a float32"):
        face_ops.s3fd_nms(torch.zeros(1, dtype=torch.int32), np.zeros((1, 8, 5), np.float32), 372, 308, 0.1)
    assert face_ops.NMS_TOP_K == facedet.TOP_K == nc.TOP_K == 750 and face_ops.NMS_MAX_CAP == 1024


def test_the_detector_refuses_an_unknown_nms_before_a_device_is_touched(monkeypatch):
    monkeypatch.setattr(facedet.S3FDDetector, "_make_engine", staticmethod(lambda *a, **k: pytest.fail("an engine was made")))
    with pytest.raises(ValueError, match="nms 'gpu'"):
        facedet.S3FDDetector(state_dict={}, nms="gpu")
    with pytest.raises(ValueError, match="nms 'gpu'"):
        facedet.S3FDDetector("/nowhere", nms="gpu")
    assert facedet.NMS_PLACES == ("device", "host")


# ---------------------------------------------------------------------------------------------- the cases the GPU tests use
def _stage2_rows(rows):
    """the float64 rows detect_faces_rows hands to nms_ (main.py:45-57), rebuilt here"""
    out = facedet.detect_output(np.asarray(rows)[None])[0][1]
    scale = np.array([nc.WIDTH, nc.HEIGHT, nc.WIDTH, nc.HEIGHT], dtype=np.float32)
    n = int((out[:, 0] > np.float32(nc.CONF_TH)).sum())
    assert (out[:n, 0] > np.float32(nc.CONF_TH)).all()              # a prefix: the kept rows are in descending score
    return np.column_stack([(out[:n, 1:] * scale).astype(np.float64), out[:n, 0].astype(np.float64)])


def test_the_stable_restatement_is_nms_where_no_score_is_tied():
    free = 0
    for case in nc.TABLE:
        rows, want = nc.table_case(*case)
        boxes = _stage2_rows(rows)
        assert len(boxes) == want.passing
        if not want.tied:
            free += 1
            assert np.array_equal(nc.nms_stable(boxes, facedet.FINAL_NMS), facedet.nms_(boxes, facedet.FINAL_NMS)), case
            assert np.array_equal(boxes[facedet.nms_(boxes, facedet.FINAL_NMS)], want.faces)
    assert free >= 5 and sum(nc.table_case(*c)[1].tied for c in nc.TABLE) == 2


def test_both_passes_suppress_rows_in_every_table_case():
    assert [c[0] for c in nc.TABLE] == [1, 2, 64, 65, 257, 777, 1024, 1024]
    for case in nc.TABLE:
        rows, want = nc.table_case(*case)
        n = case[0]
        assert rows.shape == (n, 5) and rows.dtype == np.float32 and (rows[:, 0] > np.float32(0.05)).all()
        print(f"n {n}, {case[1]} clusters, ties {case[2]}: stage 1 keeps {want.detect_n}, {want.passing} pass 0.1, {want.status} faces")
        assert want.status == len(want.faces) >= 1 and want.passing <= want.detect_n
        if n >= 64:
            assert want.status < want.detect_n < n, case
        if case[2]:
            assert want.tied and len(np.unique(rows[:, 0])) <= 16


def test_the_special_frames_are_what_their_tests_say():
    twins, far = nc.degenerate_rows()
    for rows, box in ((twins, nc.ZERO_AREA), (far, nc.FAR_ZERO_AREA)):
        want = nc.Expected(rows)
        assert (want.detect_out[:, 1:] == box).all(axis=1).sum() == 1                 # of three twins one is kept; the far one is
        assert (want.faces[:, 0] == want.faces[:, 2]).sum() == 1 and want.detect_n < len(rows) - 2
    assert (twins[:, 1:] == nc.ZERO_AREA).all(axis=1).sum() == 3
    tied = nc.tied_clusters()
    want = nc.Expected(tied)
    assert len(np.unique(tied[:, 0])) == 1 and want.detect_n == 8 and want.tied
    assert [int(np.flatnonzero((tied == d).all(axis=1))[0]) for d in want.detect_out] == list(range(39, 31, -1))     # higher index first


def test_the_host_walk_runs_off_the_array_on_the_grid():
    grid = nc.disjoint_grid()
    assert grid.shape == (784, 5) and grid[:, 0].min() > 0.1
    out = facedet.detect_output(grid[None])[0]
    assert (out[1, :, 0] > np.float32(nc.CONF_TH)).all()                              # 750 kept, all above conf_th
    with pytest.raises(IndexError):
        facedet.detect_faces_rows(out, nc.WIDTH, nc.HEIGHT, nc.CONF_TH)
    want = nc.Expected(grid)
    assert want.status == -2 and want.detect_n == 750
