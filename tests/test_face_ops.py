"""The face pipeline's device path, the parts that need no GPU: the build lists, the argument checks of the four operators
(refused before any device call), LandmarkDetector._crop_geometry against _crop, and two facts about the oracle's
resize_linear_u8 that tests/test_face_ops_gpu.py and tests/test_face_pipeline_gpu.py lean on."""
import ctypes as C
import os

import numpy as np
import pytest

from calipsync_amd import _lib, build, face_ops, landmarks, recipe
from face_cases import quarter_canvas, virtual_crop
from oracle import frame_ops_oracle as fo


# ---------------------------------------------------------------------------------------------- build lists
def test_sixth_object_directory_is_part_of_the_build(monkeypatch, tmp_path):
    others = (build.OBJ_DIR, build.OBJ_DIR_HB16, build.OBJ_DIR_LMK, build.OBJ_DIR_DET, build.OBJ_DIR_DET16)
    assert build.OBJ_DIR_FACE == os.path.join(build.LIB_DIR, "obj_face") and build.OBJ_DIR_FACE not in others
    assert build.SOURCES_FACE == ["face_ops.hip"] and "face_ops.hip" in build.SOURCES
    assert "face_ops.hip" not in build.SOURCES_HB16 + build.SOURCES_LMK + build.SOURCES_DET + build.SOURCES_DET16
    src = os.path.join(build.CSRC, "face_ops.hip")
    assert os.path.exists(src)
    with_face = build.source_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "face_ops.hip"])
    assert build.source_hash() != with_face
    monkeypatch.undo()
    # is_stale() looks at it (a stand-in library file, nothing is touched)
    lib = tmp_path / "libcasync_hip.so"
    lib.write_bytes(b"")
    os.utime(lib, (os.path.getmtime(src) - 10, os.path.getmtime(src) - 10))
    monkeypatch.setattr(build, "LIB_PATH", str(lib))
    monkeypatch.setattr(build, "SOURCES", ["face_ops.hip"])
    monkeypatch.setattr(build, "SOURCES_HB16", [])
    monkeypatch.setattr(build, "SOURCES_LMK", [])
    monkeypatch.setattr(build, "HEADERS", [])
    assert build.is_stale()
    monkeypatch.setattr(build, "SOURCES", [])
    assert not build.is_stale()


def test_the_operators_are_bound_and_the_abi_version_is_unchanged():
    for name in ("casync_op_resize_linear_u8", "casync_op_face_crops192", "casync_op_s3fd_candidates", "casync_op_landmarks_finalize"):
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 13 and _lib.load().casync_abi_version() == 13


# ---------------------------------------------------------------------------------------------- argument checks
@pytest.fixture(scope="module")
def host():
    """host buffers standing in for device pointers: a refused call never touches them"""
    buf = (C.c_uint8 * 4096)()
    return _lib.load(), C.addressof(buf), buf


def _refused(lib, status, *words):
    assert status == -1
    msg = lib.casync_last_error().decode()
    assert all(w in msg for w in words), msg


def test_resize_refuses_bad_arguments_before_any_device_call(host):
    lib, p, _ = host
    _refused(lib, lib.casync_op_resize_linear_u8(None, 1, 4, 4, p, 2, 2, 2.0, 2.0, None), "resize_linear_u8", "null")
    _refused(lib, lib.casync_op_resize_linear_u8(p, 0, 4, 4, p, 2, 2, 2.0, 2.0, None), "resize_linear_u8", "batch 0")
    _refused(lib, lib.casync_op_resize_linear_u8(p, 1, 0, 4, p, 2, 2, 2.0, 2.0, None), "resize_linear_u8", "0 x 4")
    _refused(lib, lib.casync_op_resize_linear_u8(p, 1, 4, 4, p, 2, 0, 2.0, 2.0, None), "resize_linear_u8", "2 x 0")
    _refused(lib, lib.casync_op_resize_linear_u8(p, 1, 4, 40000, p, 2, 2, 2.0, 2.0, None), "resize_linear_u8", "40000")
    _refused(lib, lib.casync_op_resize_linear_u8(p, 1, 4, 4, p, 2, 2, 0.0, 2.0, None), "resize_linear_u8", "scale")
    _refused(lib, lib.casync_op_resize_linear_u8(p, 1, 4, 4, p, 2, 2, 2.0, float("nan"), None), "resize_linear_u8", "scale")


def test_crops_refuse_bad_records_before_any_device_call(host):
    lib, p, _ = host

    def call(rows, n_frames=2, h=60, w=80):
        g = np.asarray(rows, dtype=np.int32).reshape(-1, 5)
        return lib.casync_op_face_crops192(p, n_frames, h, w, g.ctypes.data, g.shape[0], p, None)

    good = [0, -5, -5, 30, 30]
    _refused(lib, call([good, [0, 0, 0, 0, 10]]), "face_crops192", "crop 1", "0 x 10")
    _refused(lib, call([[0, 0, 0, 10, -3]]), "face_crops192", "crop 0", "10 x -3")
    _refused(lib, call([good, good, [2, 0, 0, 10, 10]]), "face_crops192", "crop 2", "frame 2 of 2")
    _refused(lib, call([[-1, 0, 0, 10, 10]]), "face_crops192", "frame -1")
    _refused(lib, call([[0, 1 << 25, 0, 10, 10]]), "face_crops192", "starts at")
    _refused(lib, call([good] * 70 + [[0, 0, 0, 10, 0]]), "face_crops192", "crop 70")      # beyond the first launch's records
    _refused(lib, call([good], h=0), "face_crops192", "0 x 80")
    _refused(lib, lib.casync_op_face_crops192(p, 2, 60, 80, None, 1, p, None), "face_crops192", "null")
    _refused(lib, lib.casync_op_face_crops192(p, 2, 60, 80, p, 0, p, None), "face_crops192", "0 crops")


def test_candidates_and_finalize_refuse_bad_arguments_before_any_device_call(host):
    lib, p, _ = host
    _refused(lib, lib.casync_op_s3fd_candidates(p, 0, 596, 0.05, 16, p, p, None), "s3fd_candidates", "batch 0")
    _refused(lib, lib.casync_op_s3fd_candidates(p, 1, 0, 0.05, 16, p, p, None), "s3fd_candidates", "0 priors")
    _refused(lib, lib.casync_op_s3fd_candidates(p, 1, 596, 0.05, 0, p, p, None), "s3fd_candidates", "cap 0")
    _refused(lib, lib.casync_op_s3fd_candidates(p, 1, 596, 0.05, 597, p, p, None), "s3fd_candidates", "cap 597")
    _refused(lib, lib.casync_op_s3fd_candidates(p, 1, 596, 0.05, 16, None, p, None), "s3fd_candidates", "null")
    g = np.asarray([[0, 0, 0, 10, 10], [0, 0, 0, 10, 0]], dtype=np.int32)
    _refused(lib, lib.casync_op_landmarks_finalize(p, p, g.ctypes.data, 2, p, None), "landmarks_finalize", "crop 1")
    _refused(lib, lib.casync_op_landmarks_finalize(p, p, g.ctypes.data, 0, p, None), "landmarks_finalize", "0 rows")
    _refused(lib, lib.casync_op_landmarks_finalize(p, None, g.ctypes.data, 1, p, None), "landmarks_finalize", "null")


def test_the_wrappers_refuse_host_tensors_and_the_unpinned_half_scale():
    import torch
    with pytest.raises(ValueError, match="device tensor"):
        face_ops.resize_frames_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), dsize=(2, 2))
    with pytest.raises(ValueError, match="device tensor"):
        face_ops.face_crops192(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), [[0, 0, 0, 2, 2]])
    with pytest.raises(ValueError, match="device tensor"):
        face_ops.s3fd_candidates(torch.zeros(1, 8, 5), 0.05, 4)
    assert face_ops.scaled_size(42, 54, 0.25) == (14, 10) and face_ops.scaled_size(41, 50, 0.25) == (12, 10)     # half to even
    stager = face_ops.FrameStager("cpu")
    with pytest.raises(ValueError, match="mixed sizes go through detect_landmarks"):
        stager.upload([np.zeros((4, 4, 3), np.uint8), np.zeros((4, 5, 3), np.uint8)], "x", "detect_landmarks")


# ---------------------------------------------------------------------------------------------- crop geometry
FH, FW = 60, 80


def geometry_boxes():
    """(x, y, w, h) boxes over a 60 x 80 frame: each border crossed, all four at once, wholly outside on each side (near and
    far), degenerate ones, and a few hundred seeded ones around and beyond the frame"""
    boxes = [(20, 15, 20, 20), (-10, 20, 30, 20), (60, 20, 30, 25), (30, -12, 20, 30), (30, 40, 25, 30),      # inside, left, right, top, bottom
             (-20, -20, 130, 110), (-5, -5, 90, 70),                                                          # all four borders
             (-70, 10, 30, 30), (-200, 10, 30, 30), (100, 10, 30, 30), (300, 10, 20, 30),                     # wholly left / right
             (10, -70, 30, 30), (10, -300, 30, 20), (10, 90, 30, 30), (10, 400, 30, 20),                      # wholly above / below
             (-90, -90, 30, 30), (120, 100, 25, 25), (-31, 10, 30, 30), (80, 10, 30, 30), (10, 60, 30, 30),   # corners, touching
             (10, 10, 0, 0), (10, 10, 1, 1), (10, 10, 0, 7), (10, 10, -4, -9), (-30, 5, -3, 2), (90, 70, 1, 0),   # degenerate
             (10.7, 11.9, 20.2, 30.99), (-0.5, -0.5, 79.9, 59.9), (0, 0, 80, 60), (0, 0, 79, 59)]
    rng = np.random.default_rng(0xFACE)
    for _ in range(300):
        x, y = rng.integers(-150, 200), rng.integers(-150, 160)
        w, h = rng.integers(-5, 140), rng.integers(-5, 140)
        boxes.append((float(x) + rng.random(), float(y) + rng.random(), float(w) + rng.random(), float(h)))
    return boxes


def test_crop_geometry_is_crops_arithmetic_without_the_pixels():
    rng = np.random.default_rng(7)
    img = rng.integers(1, 256, (FH, FW, 3), dtype=np.uint8)          # no zero pixel: padding is told apart from the image
    crop_fn, geom_fn = landmarks.LandmarkDetector._crop, landmarks.LandmarkDetector._crop_geometry
    seen = {"square": 0, "not square": 0, "empty": 0, "all outside": 0}
    for box in geometry_boxes():
        crop, (ox, oy) = crop_fn(img, box)
        x1, y1, w, h = geom_fn(FH, FW, box)
        assert all(isinstance(v, int) for v in (x1, y1, w, h))
        assert crop.shape[:2] == (h, w), (box, crop.shape, (x1, y1, w, h))
        if w < 1 or h < 1:
            seen["empty"] += 1
            continue
        assert (ox, oy) == (x1, y1), box
        assert np.array_equal(crop, virtual_crop(img, x1, y1, w, h)), box
        seen["square" if w == h else "not square"] += 1
        seen["all outside"] += int(not crop.any())
    assert seen["empty"] >= 2 and min(seen["square"], seen["not square"], seen["all outside"]) >= 20, seen


# ---------------------------------------------------------------------------------------------- two facts about the oracle
def test_oracle_quarter_resize_of_a_4x_replicated_frame_is_the_frame():
    """(a) tests/test_face_pipeline_gpu.py replicates the recipe's 77 x 93 frames 4x and expects the detector at scale 0.25
    to see the frames themselves"""
    for f in recipe.make_s3fd_inputs(2):
        big = np.repeat(np.repeat(f, 4, 0), 4, 1)
        assert big.shape == (308, 372, 3)
        assert np.array_equal(fo.resize_linear_u8(big, (93, 77)), f)


def _quarter(img):
    """cv2.resize(img, (0, 0), fx=0.25, fy=0.25) in the oracle's arithmetic with the scale given (4.0), not derived from the
    sizes: the tables of resize_linear_u8 written out per destination index"""
    sh, sw = img.shape[:2]
    dw, dh = face_ops.scaled_size(sh, sw, 0.25)

    def table(n_dst, n_src, clamp):
        idx, c0, c1 = [], [], []
        for d in range(n_dst):
            f = np.float32((d + 0.5) * 4.0 - 0.5)
            s = int(np.floor(f))
            f = np.float32(f - np.float32(s))
            if clamp and s < 0:
                s, f = 0, np.float32(0)
            if clamp and s >= n_src - 1:
                s, f = n_src - 1, np.float32(0)
            a0, a1 = fo._fixed_coefs(np.asarray([f], dtype=np.float32))
            idx.append((min(max(s, 0), n_src - 1), min(max(s + 1, 0), n_src - 1)))
            c0.append(int(a0[0]))
            c1.append(int(a1[0]))
        return idx, c0, c1

    xi, a0, a1 = table(dw, sw, True)
    yi, b0, b1 = table(dh, sh, False)
    s = img.astype(np.int64)
    out = np.empty((dh, dw, 3), dtype=np.uint8)
    for y in range(dh):
        for x in range(dw):
            top = s[yi[y][0], xi[x][0]] * a0[x] + s[yi[y][0], xi[x][1]] * a1[x]
            bot = s[yi[y][1], xi[x][0]] * a0[x] + s[yi[y][1], xi[x][1]] * a1[x]
            out[y, x] = np.clip((((b0[y] * (top >> 4)) >> 16) + ((b1[y] * (bot >> 4)) >> 16) + 2) >> 2, 0, 255)
    return out


def test_oracle_on_an_edge_replicated_canvas_is_the_quarter_scale_form():
    """(b) for sides 40 .. 58: edge padding holds everywhere, zero padding is wrong where a side is 2 mod 4 (the last
    destination index then reads one source index past the end, which the fx form clamps)"""
    rng = np.random.default_rng(25)
    sides = list(range(40, 59))
    zero_pad_differs = 0
    for h, w in zip(sides, sides[5:] + sides[:5]):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        canvas, dsize = quarter_canvas(img)
        want = _quarter(img)
        assert want.shape[:2] == dsize[::-1]
        assert np.array_equal(fo.resize_linear_u8(canvas, dsize), want), (h, w)
        zeros, _ = quarter_canvas(img, "constant")
        if h % 4 == 2 or w % 4 == 2:
            zero_pad_differs += int(not np.array_equal(fo.resize_linear_u8(zeros, dsize), want))
    assert zero_pad_differs >= 4
