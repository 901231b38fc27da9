"""The 4:2:0 JPEG encoder without a GPU: the numpy twin against the recorded libjpeg-turbo bytes and against live Pillow, the
header, the `subsampling` keyword and what it leaves alone, and the three new entries of the C ABI."""
import os
import re

import numpy as np
import pytest

import jpeg420_cases as j4
import jpeg_cases as jc
from calipsync_amd import jpeg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB = j4.SUB


@pytest.mark.parametrize("name", j4.names())
def test_host_twin_equals_the_recorded_bytes(name):
    frame, q, want = j4.case(name)
    got = jpeg.encode_jpeg_host(frame, q, SUB)
    assert len(got) == len(want) and got == want
    assert got == jpeg.encode_jpeg_host(frame, q, 2)                                 # Pillow's spelling
    assert jpeg.jpeg_header(frame.shape[0], frame.shape[1], q, SUB) == want[:jpeg.HEADER_BYTES]


def test_host_twin_equals_the_recorded_hash_of_the_full_size_case():
    frame, q, sha, length = j4.full_case()
    got = jpeg.encode_jpeg_host(frame, q, SUB)
    assert len(got) == length and jc.sha256(got) == sha
    assert jc.decode(got).shape == (1080, 1920, 3)


# sizes around every edge rule: 1 x 1, whole MCUs, one past, right / bottom / both dummies, odd sizes, more than 64 MCUs a row
LIVE = [(1, 1), (2, 3), (8, 8), (9, 9), (15, 17), (16, 16), (17, 17), (8, 24), (31, 18), (24, 40), (33, 47), (147, 8), (24, 1048)]


@pytest.mark.parametrize("h,w", LIVE)
def test_host_twin_equals_live_pillow_on_seeded_shapes(h, w):
    if not jc.pillow_restart_rows():
        pytest.skip("this Pillow does not know restart_marker_rows")
    for q in (10, 50, 95, 100):
        frame = j4.seeded(h, w, 100 + q)
        assert jpeg.encode_jpeg_host(frame, q, SUB) == j4.generator().pillow(frame, q), (h, w, q)


def test_header_differs_from_444_in_the_sampling_byte_and_the_restart_interval_only():
    for h, w, q in ((8, 8, 95), (19, 37, 1), (1080, 1920, 100), (65535, 65535, 50)):
        a, b = jpeg.jpeg_header(h, w, q, "4:4:4"), jpeg.jpeg_header(h, w, q, SUB)
        assert len(a) == len(b) == 629 == jpeg.HEADER_BYTES
        sof, dri = a.index(b"\xff\xc0"), a.index(b"\xff\xdd")
        assert a[sof + 11] == 0x11 and b[sof + 11] == 0x22                           # component 1: Y samples 2 x 2
        assert a[dri + 4:dri + 6] == ((w + 7) // 8).to_bytes(2, "big") and b[dri + 4:dri + 6] == ((w + 15) // 16).to_bytes(2, "big")
        differ = {i for i in range(629) if a[i] != b[i]}
        assert sof + 11 in differ and differ <= {sof + 11, dri + 4, dri + 5}


@pytest.mark.parametrize("name", j4.names())
def test_pillow_decodes_the_files_to_the_right_size(name):
    frame, q, want = j4.case(name)
    got = jc.decode(jpeg.encode_jpeg_host(frame, q, SUB))
    assert got.shape == frame.shape and np.array_equal(got, jc.decode(want))


@pytest.mark.parametrize("name", jc.names())
def test_without_the_keyword_the_bytes_are_todays(name):
    frame, q, want = jc.case(name)                                                   # the recorded 4:4:4 files
    assert jpeg.encode_jpeg_host(frame, q) == want == jpeg.encode_jpeg_host(frame, q, 0) == jpeg.encode_jpeg_host(frame, q, "4:4:4")
    assert jpeg.jpeg_header(frame.shape[0], frame.shape[1], q) == want[:629]
    assert jpeg.default_slot_bytes(frame.shape[1]) == 2 * 8 * 3 * 8 * ((frame.shape[1] + 7) // 8)
    assert jpeg.symbol_statistics(frame, q) == jpeg.symbol_statistics(frame, q, "4:4:4")


def test_a_bad_subsampling_value_raises():
    import torch
    ok = np.zeros((8, 8, 3), dtype=np.uint8)
    for bad in ("4:2:2", "420", 1, 3, None, 2.0, True, "", (2,)):
        with pytest.raises(ValueError, match="subsampling"):
            jpeg.encode_jpeg_host(ok, 95, bad)
        with pytest.raises(ValueError, match="subsampling"):
            jpeg.jpeg_header(8, 8, 95, subsampling=bad)
        with pytest.raises(ValueError, match="subsampling"):
            jpeg.symbol_statistics(ok, 95, subsampling=bad)
        with pytest.raises(ValueError, match="subsampling"):
            jpeg.default_slot_bytes(8, subsampling=bad)
        with pytest.raises(ValueError, match="subsampling"):                          # before a device is asked for
            jpeg.encode_jpeg_device(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 95, subsampling=bad)
    with pytest.raises(RuntimeError, match="ROCm device"):
        jpeg.encode_jpeg_device(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 95, subsampling=SUB)
    assert jpeg.default_slot_bytes(1920, SUB) == 2 * 384 * 120 and jpeg.default_slot_bytes(17, 2) == 2 * 384 * 2
    assert jpeg.restart_rows(1080, SUB) == 68 and jpeg.restart_rows(1080) == 135


def test_dummy_blocks_code_as_difference_zero_and_end_of_block():
    frame, q, _ = j4.case("noise_8x24_q95")                                          # 2 MCUs; Y01 of the second and both Y1x are dummies
    blocks, dummy = jpeg.quantized_blocks_420(frame, q)
    assert blocks.shape == (1, 2, 6, 64) and dummy.tolist() == [[[False, False, True, True, False, False],
                                                                 [False, True, True, True, False, False]]]
    assert not blocks[dummy][:, 1:].any()
    assert blocks[0, 0, 2, 0] == blocks[0, 0, 3, 0] == blocks[0, 0, 1, 0] and blocks[0, 1, 3, 0] == blocks[0, 1, 0, 0]


def test_the_three_new_entries_are_exported_and_declared():
    from calipsync_amd import _lib, build
    build.build()
    lib = _lib.load()
    counts = {"casync_op_jpeg420_header": 5, "casync_op_jpeg420_workspace_bytes": 4, "casync_op_jpeg420_encode": 13}
    header = open(os.path.join(REPO, "include", "casync_hip.h")).read()
    assert "#define CASYNC_ABI_VERSION 13" in header and _lib.ABI_VERSION == 13 and lib.casync_abi_version() == 13
    for name, n in counts.items():
        assert name in _lib.EXPORTS and len(_lib._PROTOS[name][1]) == n and hasattr(lib, name)
        assert _lib._PROTOS[name] == _lib._PROTOS[name.replace("jpeg420", "jpeg")]     # the argument lists of the 4:4:4 trio
        proto = re.search(name + r"\(([^;]*?)\);", header, re.S)
        assert proto and len(proto.group(1).split(",")) == n, name
    for words in ("4:2:0 baseline JPEG of finished frames", "status 1", "status 2", "one restart interval per MCU row", "dummy"):
        assert words in header, words


def test_header_and_workspace_entries_agree_with_the_twin():
    import ctypes
    from calipsync_amd import _lib, build
    build.build()
    lib = _lib.load()
    for h, w, q in ((8, 8, 95), (19, 37, 1), (1080, 1920, 100), (65535, 1, 50)):
        assert jpeg._header_from_lib(h, w, q, SUB) == jpeg.jpeg_header(h, w, q, SUB)
        assert jpeg._header_from_lib(h, w, q) == jpeg.jpeg_header(h, w, q)
    buf = (ctypes.c_uint8 * 629)()
    for args in ((0, 8, 95, buf, 629), (8, 65536, 95, buf, 629), (8, 8, 0, buf, 629), (8, 8, 101, buf, 629), (8, 8, 95, buf, 628),
                 (8, 8, 95, None, 629)):
        assert lib.casync_op_jpeg420_header(*args) < 0
    rows = 68
    assert lib.casync_op_jpeg420_workspace_bytes(16, 1080, 1920, 0) >= 16 * rows * (4 + 2 * 384 * 120)
    assert lib.casync_op_jpeg420_workspace_bytes(16, 1080, 1920, 0) == lib.casync_op_jpeg420_workspace_bytes(16, 1080, 1920, 2 * 384 * 120)
    assert lib.casync_op_jpeg420_workspace_bytes(3, 19, 37, 100) >= 3 * 2 * 104
    assert lib.casync_op_jpeg420_workspace_bytes(0, 8, 8, 0) == 0
    assert lib.casync_op_jpeg420_workspace_bytes(-1, 8, 8, 0) < 0 and lib.casync_op_jpeg420_workspace_bytes(1, 0, 8, 0) < 0
    # the encode refuses bad arguments before anything is launched: host buffers stand in for device memory
    host = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(host)
    good = [p, 1, 8, 8, 95, 0, p, 4096, p, 4096, p, p, None]
    for i, v in ((1, -1), (2, 0), (2, 65536), (3, 0), (3, 65536), (4, 0), (4, 101), (5, -1), (7, 16), (9, -1), (0, None), (6, None), (8, None),
                 (10, None), (11, None)):
        args = list(good)
        args[i] = v
        assert lib.casync_op_jpeg420_encode(*args) < 0, (i, v)
    args = list(good)
    args[1] = 0
    assert lib.casync_op_jpeg420_encode(*args) == 0          # batch 0: a no-op
    assert bytes(host) == bytes(4096)


def test_frame_synthesizer_validates_the_subsampling_without_a_gpu():
    from calipsync_amd.frame_synth import FrameSynthesizer
    with pytest.raises(ValueError, match="subsampling"):
        FrameSynthesizer(None, "/nonexistent", output="jpeg", resident=True, net=object(), jpeg_subsampling="4:2:2")
    with pytest.raises(ValueError, match="resident"):
        FrameSynthesizer(None, "/nonexistent", output="jpeg", net=object(), jpeg_subsampling=SUB)
    with pytest.raises(ValueError, match="quality"):
        FrameSynthesizer(None, "/nonexistent", output="jpeg", resident=True, net=object(), jpeg_quality=0, jpeg_subsampling=SUB)

    class Net:
        def eval(self):
            return self

    for sub in (SUB, 2, "4:4:4", 0):                                                  # a clip made elsewhere: nothing is loaded
        synth = FrameSynthesizer(None, None, clip=[None] * 3, net=Net(), output="jpeg", jpeg_subsampling=sub)
        assert synth.output == "jpeg" and synth.jpeg_subsampling == sub and synth.jpeg_quality == 95
        synth.executor.shutdown()
    synth = FrameSynthesizer(None, None, clip=[None] * 3, net=Net(), output="jpeg")
    assert synth.jpeg_subsampling == "4:4:4"                                          # the default is unchanged
    synth.executor.shutdown()
