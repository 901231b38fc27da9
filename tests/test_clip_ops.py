"""A clip resident on the device, the parts that need no GPU: the two symbols and their argument checks (refused before any
device call, on a host buffer that stays untouched), the eighth object directory, clip_geometry against frame_loop.crop_box
and the reference's point arithmetic, the clip-size cap, and who owns the pinned block behind the frames of a batch."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import clip_cases as cc
from calipsync_amd import _lib, build, frame_loop, resident_clip
from frame_data import make_frames


def test_the_symbols_are_exported_and_bound_and_the_abi_version_is_unchanged():
    lib = _lib.load()
    for name, nargs in (("casync_op_clip_gather", 9), ("casync_op_clip_compose", 10)):
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    assert _lib.ABI_VERSION == 13 and lib.casync_abi_version() == 13
    header = open(os.path.join(os.path.dirname(build.HERE), "include", "casync_hip.h")).read()
    assert "casync_op_clip_gather(" in header and "casync_op_clip_compose(" in header and "#define CASYNC_ABI_VERSION 13" in header
    assert "{ frame, y0, x0, h, w, valid, region byte offset, 0 }" in header


def test_eighth_object_directory_is_part_of_the_build(monkeypatch):
    others = (build.OBJ_DIR, build.OBJ_DIR_HB16, build.OBJ_DIR_LMK, build.OBJ_DIR_DET, build.OBJ_DIR_DET16, build.OBJ_DIR_FACE,
              build.OBJ_DIR_NMS)
    assert build.OBJ_DIR_CLIP == os.path.join(build.LIB_DIR, "obj_clip") and build.OBJ_DIR_CLIP not in others and len(set(others)) == 7
    assert build.SOURCES_CLIP == ["clip_ops.hip"] and "clip_ops.hip" in build.SOURCES
    assert "clip_ops.hip" not in build.SOURCES_HB16 + build.SOURCES_LMK + build.SOURCES_DET + build.SOURCES_DET16 + build.SOURCES_FACE + \
        build.SOURCES_NMS
    assert os.path.exists(os.path.join(build.CSRC, "clip_ops.hip"))
    with_clip = build.source_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "clip_ops.hip"])
    assert build.source_hash() != with_clip


# ---------------------------------------------------------------------------------------------- argument checks
N, H, W = 4, 20, 30          # the frames the refused calls pretend to have
REGIONS = 2048


@pytest.fixture(scope="module")
def host():
    buf = cc.host_buffer(4096)
    return _lib.load(), C.addressof(buf), buf


def _refused(lib, buf, status, *words):
    assert status == -1
    msg = lib.casync_last_error().decode()
    assert all(w in msg for w in words), msg
    assert bytes(buf) == bytes([cc.FILL]) * len(buf), "a refused call wrote to a buffer"


def _rec(*rows):
    r = np.zeros((len(rows), 8), dtype=np.int32)
    for i, row in enumerate(rows):
        r[i, :len(row)] = row
    return r


GOOD = (1, 2, 3, 4, 5, 1, 16)         # frame 1, a 4 x 5 box at (2, 3), valid, offset 16
BAD_RECORDS = [                       # (record, words of the message); each is refused behind a good record
    ((-1, 2, 3, 4, 5, 1, 16), ("frame -1 of 4",)),
    ((4, 2, 3, 4, 5, 1, 16), ("frame 4 of 4",)),
    ((1, 2, 3, 0, 5, 1, 16), ("0 x 5",)),
    ((1, 2, 3, 4, -1, 1, 16), ("4 x -1",)),
    ((1, -1, 3, 4, 5, 1, 16), ("not inside",)),
    ((1, 2, -1, 4, 5, 1, 16), ("not inside",)),
    ((1, 17, 3, 4, 5, 1, 16), ("not inside",)),                   # y0 + h = 21 > 20
    ((1, 2, 26, 4, 5, 1, 16), ("not inside",)),                   # x0 + w = 31 > 30
    ((1, 2, 3, 2 ** 31 - 1, 5, 1, 16), ("not inside",)),          # y0 + h beyond int
    ((1, 2, 3, 4, 5, 1, -1), ("offset -1",)),
    ((1, 2, 3, 4, 5, 1, REGIONS - 59), ("do not fit",)),          # 60 bytes, one too many
]


def test_gather_refuses_bad_arguments_before_any_device_call(host):
    lib, p, buf = host
    gather = lib.casync_op_clip_gather
    rec = _rec(GOOD)
    _refused(lib, buf, gather(None, N, H, W, rec.ctypes.data, 1, p, REGIONS, None), "clip_gather", "null")
    _refused(lib, buf, gather(p, N, H, W, None, 1, p, REGIONS, None), "clip_gather", "null")
    _refused(lib, buf, gather(p, N, H, W, rec.ctypes.data, 1, None, REGIONS, None), "clip_gather", "null")
    _refused(lib, buf, gather(p, N, 0, W, rec.ctypes.data, 1, p, REGIONS, None), "clip_gather", "0 x 30")
    _refused(lib, buf, gather(p, N, H, -3, rec.ctypes.data, 1, p, REGIONS, None), "clip_gather", "20 x -3")
    _refused(lib, buf, gather(p, N, H, W, rec.ctypes.data, -1, p, REGIONS, None), "clip_gather", "batch -1")
    assert gather(p, N, H, W, rec.ctypes.data, 0, p, REGIONS, None) == 0          # nothing to do, nothing launched
    for bad, words in BAD_RECORDS:
        for valid in (1, 0):                                                       # gather checks the box whatever valid says
            row = list(bad)
            row[5] = valid
            for rec in (_rec(row), _rec(GOOD, row), _rec(*([GOOD] * 70 + [row]))):   # alone, second, in the second launch's block
                _refused(lib, buf, gather(p, N, H, W, rec.ctypes.data, len(rec), p, REGIONS, None), "clip_gather", f"record {len(rec) - 1}",
                         *words)
    _refused(lib, buf, gather(p, 0, H, W, _rec(GOOD).ctypes.data, 1, p, REGIONS, None), "clip_gather", "of 0")


def test_compose_refuses_bad_arguments_before_any_device_call(host):
    lib, p, buf = host
    compose = lib.casync_op_clip_compose
    rec = _rec(GOOD)
    _refused(lib, buf, compose(None, N, H, W, rec.ctypes.data, 1, p, REGIONS, p, None), "clip_compose", "null")
    _refused(lib, buf, compose(p, N, H, W, None, 1, p, REGIONS, p, None), "clip_compose", "null")
    _refused(lib, buf, compose(p, N, H, W, rec.ctypes.data, 1, p, REGIONS, None, None), "clip_compose", "null")
    _refused(lib, buf, compose(p, N, 0, W, rec.ctypes.data, 1, p, REGIONS, p, None), "clip_compose", "0 x 30")
    _refused(lib, buf, compose(p, N, H, 0, rec.ctypes.data, 1, p, REGIONS, p, None), "clip_compose", "20 x 0")
    _refused(lib, buf, compose(p, N, H, W, rec.ctypes.data, -2, p, REGIONS, p, None), "clip_compose", "batch -2")
    assert compose(p, N, H, W, rec.ctypes.data, 0, p, REGIONS, p, None) == 0
    assert compose(p, N, H, W, rec.ctypes.data, 0, None, 0, p, None) == 0
    # a valid record needs out_regions
    _refused(lib, buf, compose(p, N, H, W, rec.ctypes.data, 1, None, 0, p, None), "clip_compose", "record 0", "out_regions is null")
    plain = _rec((1, 2, 3, 4, 5, 0, 16))
    _refused(lib, buf, compose(p, N, H, W, _rec(plain[0], GOOD).ctypes.data, 2, None, 0, p, None), "clip_compose", "record 1",
             "out_regions is null")
    for bad, words in BAD_RECORDS:
        for rec in (_rec(bad), _rec(GOOD, bad), _rec(*([GOOD] * 70 + [bad]))):
            _refused(lib, buf, compose(p, N, H, W, rec.ctypes.data, len(rec), p, REGIONS, p, None), "clip_compose", f"record {len(rec) - 1}",
                     *words)
    # the frame index is checked on an invalid record too; its box is not (see the accepted call in the GPU ledger:
    # clip_cases' plain batches)
    for frame in (-1, 4):
        _refused(lib, buf, compose(p, N, H, W, _rec((frame, 2, 3, 4, 5, 0, 16)).ctypes.data, 1, p, REGIONS, p, None), "clip_compose",
                 f"frame {frame} of 4")


def test_the_cases_are_what_the_gpu_tests_say():
    for h, w in cc.SIZES + [cc.REAL]:
        c = cc.case(h, w)
        box_bytes = c.rec[:, 3] * c.rec[:, 4] * 3
        gaps = c.rec[1:, 6] - (c.rec[:-1, 6] + box_bytes[:-1])
        assert 1 <= c.rec[0, 6] <= 15 and ((gaps >= 1) & (gaps <= 15)).all()
        assert (c.rec[:, 1] + c.rec[:, 3] <= h).all() and (c.rec[:, 2] + c.rec[:, 4] <= w).all()
        assert ((h, w) == cc.REAL or c.rec[0, 5] == 0) and c.rec[-1, 5] == 0 and c.rec[:, 5].any() and not c.rec_plain[:, 5].any()
        assert not np.array_equal(c.want_out, c.want_plain)
        assert int((c.want_regions != cc.FILL).sum()) >= 0.9 * box_bytes.sum()
    assert [(h * w * 3) % 16 == 0 for h, w in cc.SIZES] == [False, False, False, True, True]
    c = cc.case(33, 31)
    assert any(r[2] % 2 == 1 and r[4] % 2 == 1 and r[4] > 1 for r in c.rec)                 # odd x0, odd w
    assert len({tuple(r[1:5]) for r in c.rec if r[0] == 1}) == 3                             # frame 1 three times, three boxes
    assert any(a > b for a, b in zip(c.rec[:-1, 0], c.rec[1:, 0]))                           # descending
    assert cc.case(5, 7, 10).batch == 80 > 64
    assert tuple(cc.case(*cc.REAL).rec[0]) == (1, 233, 611, 700, 700, 1, 1, 0)


# ---------------------------------------------------------------------------------------------- geometry
def _border_landmarks():
    """make_frames(7, 420, 560, seed=21) with frames 3 and 5 moved to the borders as tests/test_frame_ops.py does, and
    frame 6 given an empty crop box (xmax <= xmin)"""
    _, lms, _ = make_frames(7, 420, 560, seed=21)
    lms[3] = lms[3].copy()
    lms[3][:, 0] += 560 - lms[3][31, 0] + 25
    lms[5] = lms[5].copy()
    lms[5][:, 1] += 420 - (lms[5][52, 1] + (lms[5][31, 0] - lms[5][1, 0])) + 12
    lms[6] = lms[6].copy()
    lms[6][31, 0] = lms[6][1, 0] - 3
    return lms


def test_clip_geometry_is_crop_box_and_the_point_arithmetic():
    lms = _border_landmarks()
    geo = resident_clip.clip_geometry(lms, 420, 560)
    assert geo.box.shape == (7, 5) and geo.pts.shape == (7, 33, 2) and geo.pts.dtype == np.int32
    assert geo.empty.tolist() == [False] * 6 + [True]
    assert geo.valid.tolist()[3] == 0 and geo.valid.tolist()[6] == 0 and geo.valid[[0, 1, 2, 4, 5]].all()
    for i, l in enumerate(lms):
        ymin, ymax, xmin, xmax, width = frame_loop.crop_box(l, 420, 560)
        assert tuple(geo.box[i]) == (ymin, ymax, xmin, xmax, width)
        if geo.empty[i]:
            assert width <= 0 and not geo.pts[i].any()
            continue
        fp = np.array(l[:33], dtype=np.float64)                      # infer_api.py:281-289
        fp[:, 0] -= xmin
        fp[:, 1] -= ymin
        fp[:, 0] *= width / (xmax - xmin)
        fp[:, 1] *= width / (ymax - ymin)
        assert np.array_equal(geo.pts[i], fp.astype(np.int32))
        assert geo.valid[i] == int(width == ymax - ymin and width == xmax - xmin)
    assert geo.box[5, 1] == 420 and geo.box[3, 3] == 560                # the two border cases are at the borders
    # int32 landmarks (what detect_landmarks_device returns) give the geometry of their values
    as_int = [np.asarray(l).astype(np.int32) for l in lms]
    again = resident_clip.clip_geometry(as_int, 420, 560)
    assert np.array_equal(again.box, resident_clip.clip_geometry([a.astype(np.float64) for a in as_int], 420, 560).box)


def test_the_clip_size_cap_and_mixed_sizes_raise_before_anything_is_allocated(monkeypatch):
    monkeypatch.setattr(frame_loop, "_acquire_pinned", lambda n: pytest.fail("a pinned buffer was asked for"))
    monkeypatch.setattr(resident_clip, "_CLIP_CAP", 1 << 20)
    imgs, lms, _ = make_frames(3, 400, 400, seed=1)                      # 3 x 480 000 bytes
    with pytest.raises(ValueError, match="CASYNC_RESIDENT_CLIP_MB"):
        resident_clip.ResidentClip(imgs, lms)
    import torch
    with pytest.raises(ValueError, match="CASYNC_RESIDENT_CLIP_MB"):
        resident_clip.ResidentClip(torch.from_numpy(np.stack(imgs)), lms)
    with pytest.raises(ValueError, match="mixed sizes go through frame_loop.submit_batch_device"):
        resident_clip.ResidentClip([imgs[0][:100, :100], imgs[1][:100, :90]], lms[:2])
    assert resident_clip._CLIP_CAP == 1 << 20 and int(os.environ.get("CASYNC_RESIDENT_CLIP_MB", "16384")) > 0


# ---------------------------------------------------------------------------------------------- who owns the pinned block
class Buf:
    """stands in for a pinned tensor"""

    def __init__(self, n):
        self.raw = bytearray(np.arange(n, dtype=np.uint32).astype(np.uint8).tobytes())
        self.a = self.numpy()

    def numel(self):
        return len(self.raw)

    def numpy(self):
        """a new array per call over memory that an object which is no ndarray owns, as Tensor.numpy() gives"""
        return np.frombuffer(self.raw, dtype=np.uint8)


def test_frames_are_views_of_the_block_until_the_last_one_is_gone(monkeypatch):
    released = []
    monkeypatch.setattr(frame_loop, "_release_pinned", released.append)
    monkeypatch.setattr(resident_clip, "_PINNED_VIEW_CAP", 1000)
    monkeypatch.setattr(resident_clip, "_OUTSTANDING", 0)
    b1 = Buf(2 * 4 * 5 * 3 + 8)
    frames = resident_clip._hand_out(b1, 2, 4, 5)
    assert [f.shape for f in frames] == [(4, 5, 3)] * 2 and all(np.shares_memory(f, b1.a) for f in frames)
    assert np.array_equal(frames[1].reshape(-1), b1.a[60:120])
    assert resident_clip.outstanding_pinned_bytes() == 128 and not released
    row = frames[1][2:3]                         # a view of a view
    first = frames[0].copy()
    del frames
    gc.collect()
    assert resident_clip.outstanding_pinned_bytes() == 128 and not released          # `row` keeps the block out
    b2 = Buf(900)                                # 128 + 900 > 1000: over the cap, copies, the block goes back at once
    copies = resident_clip._hand_out(b2, 3, 10, 10)
    assert released == [b2] and resident_clip.outstanding_pinned_bytes() == 128
    assert not any(np.shares_memory(c, b2.a) for c in copies) and np.array_equal(copies[2].reshape(-1), b2.a[600:900])
    assert np.array_equal(row, b1.a[60:120].reshape(4, 5, 3)[2:3])
    del row
    gc.collect()
    assert released == [b2, b1] and resident_clip.outstanding_pinned_bytes() == 0
    assert np.array_equal(first.reshape(-1), b1.a[:60])
    b3 = Buf(872)                                # 872 <= 1000 again
    views = resident_clip._hand_out(b3, 1, 2, 2)
    assert resident_clip.outstanding_pinned_bytes() == 872 and np.shares_memory(views[0], b3.a)
    monkeypatch.setattr(resident_clip, "_PINNED_VIEW_CAP", 0)                          # the cap forced to 0: always copies
    b4 = Buf(12)
    assert not np.shares_memory(resident_clip._hand_out(b4, 1, 2, 2)[0], b4.a) and released[-1] is b4
    del views
    gc.collect()
    assert resident_clip.outstanding_pinned_bytes() == 0 and released[-1] is b3


def test_a_real_tensor_behaves_like_the_stand_in(monkeypatch):
    import torch
    released = []
    monkeypatch.setattr(frame_loop, "_release_pinned", released.append)
    monkeypatch.setattr(resident_clip, "_OUTSTANDING", 0)
    t = torch.arange(96, dtype=torch.uint8)      # pageable here: the ownership is the tensor's either way
    frames = resident_clip._hand_out(t, 2, 4, 4)
    keep = frames[1][1]
    del frames
    gc.collect()
    assert not released and resident_clip.outstanding_pinned_bytes() == 96
    assert keep.tolist() == t[48 + 12:48 + 24].view(4, 3).tolist()
    del keep
    gc.collect()
    assert released == [t] and resident_clip.outstanding_pinned_bytes() == 0
