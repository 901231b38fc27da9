"""The JPEG encoder without a GPU: the numpy twin against the recorded libjpeg-turbo bytes and against live Pillow, the header,
the argument checks, encoded items in the Motion-JPEG AVI writer, and the three entries of the C ABI."""
import io
import os
import re

import numpy as np
import pytest

import jpeg_cases as jc
from calipsync_amd import jpeg, mjpeg_avi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", jc.names())
def test_host_twin_equals_the_recorded_bytes(name):
    frame, q, want = jc.case(name)
    got = jpeg.encode_jpeg_host(frame, q)
    assert len(got) == len(want) and got == want
    assert jpeg.jpeg_header(frame.shape[0], frame.shape[1], q) == want[:jpeg.HEADER_BYTES] and jpeg.HEADER_BYTES == 629


def test_host_twin_equals_the_recorded_hash_of_the_full_size_case():
    frame, q, sha, length = jc.full_case()
    got = jpeg.encode_jpeg_host(frame, q)
    assert len(got) == length and jc.sha256(got) == sha
    assert jc.decode(got).shape == (1080, 1920, 3)


@pytest.mark.parametrize("name", jc.names())
def test_host_twin_equals_live_pillow(name):
    if not jc.pillow_restart_rows():
        pytest.skip("this Pillow does not know restart_marker_rows")
    frame, q, _ = jc.case(name)
    assert jpeg.encode_jpeg_host(frame, q) == jc.generator().pillow(frame, q)


@pytest.mark.parametrize("name", jc.names())
def test_output_opens_and_decodes_to_the_fixtures_pixels(name):
    frame, q, want = jc.case(name)
    got = jc.decode(jpeg.encode_jpeg_host(frame, q))
    assert got.shape == frame.shape and np.array_equal(got, jc.decode(want))


def test_quantisation_tables_are_clamped_at_both_ends():
    luma, chroma = jpeg.quant_tables(1)
    assert luma.max() == 255 and chroma.min() == 255
    luma, chroma = jpeg.quant_tables(100)
    assert luma.max() == 1 and chroma.max() == 1
    luma, _ = jpeg.quant_tables(50)
    assert tuple(luma) == jpeg.BASE_LUMA


def test_bad_arguments_raise_value_error():
    ok = np.zeros((8, 8, 3), dtype=np.uint8)
    for bad in (ok.astype(np.float32), ok[:, :, :2], ok[0], np.zeros((2, 8, 8, 3), dtype=np.uint8)):
        with pytest.raises(ValueError):
            jpeg.encode_jpeg_host(bad, 95)
    for q in (0, 101, -3, 50.5):
        with pytest.raises(ValueError):
            jpeg.encode_jpeg_host(ok, q)
        with pytest.raises(ValueError):
            jpeg.jpeg_header(8, 8, q)
    for h, w in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
        with pytest.raises(ValueError):
            jpeg.jpeg_header(h, w, 95)
    assert len(jpeg.jpeg_header(65535, 65535, 1)) == 629


def test_device_entry_refuses_bad_input_before_a_device_is_touched():
    import torch
    ok = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)       # a host tensor: a device would be the next thing asked for
    for bad in (ok.float(), ok[0], ok[..., :2], np.zeros((2, 8, 8, 3), dtype=np.uint8)):
        with pytest.raises(ValueError):
            jpeg.encode_jpeg_device(bad, 95)
    for q in (0, 101):
        with pytest.raises(ValueError):
            jpeg.encode_jpeg_device(ok, q)
    with pytest.raises(ValueError):
        jpeg.encode_jpeg_device(ok, 95, slot_bytes=-1)
    with pytest.raises(RuntimeError, match="ROCm device"):
        jpeg.encode_jpeg_device(ok, 95)


def test_frame_synthesizer_checks_output_before_anything_is_loaded():
    from calipsync_amd.frame_synth import FrameSynthesizer
    with pytest.raises(ValueError, match="resident"):
        FrameSynthesizer(None, "/nonexistent", output="jpeg", net=object())
    with pytest.raises(ValueError, match="resident"):
        FrameSynthesizer(None, "/nonexistent", output="jpeg", resident=False, net=object())
    with pytest.raises(ValueError, match="output"):
        FrameSynthesizer(None, "/nonexistent", output="png", resident=True, net=object())


# ---------------------------------------------------------------------------------------------------------------- the AVI writer
def _files(names):
    return [jc.case(n) for n in names]


def test_avi_writer_stores_encoded_items_as_they_are(tmp_path):
    frame, q, data = jc.case("noise_19x37_q95")
    other = np.ascontiguousarray(frame[::-1])
    path = str(tmp_path / "mixed.avi")
    items = [data, other, bytearray(data), memoryview(jpeg.encode_jpeg_host(other, 75))]
    assert mjpeg_avi.write_mjpeg_avi(path, items, fps=25) == 4
    raw = open(path, "rb").read()
    assert raw.count(data) == 2 and jpeg.encode_jpeg_host(other, 75) in raw       # stored byte for byte
    fps, frames = mjpeg_avi.read_mjpeg_avi(path)
    assert fps == 25 and len(frames) == 4
    bgr = lambda d: np.ascontiguousarray(jc.decode(d)[:, :, ::-1])
    assert np.array_equal(frames[0], bgr(data)) and np.array_equal(frames[2], bgr(data))
    assert np.array_equal(frames[1], bgr(mjpeg_avi.encode_jpeg(other, 95)))        # arrays still go through Pillow
    assert np.array_equal(frames[3], bgr(jpeg.encode_jpeg_host(other, 75)))
    assert mjpeg_avi.jpeg_size(data) == (19, 37)


def test_avi_writer_refuses_items_of_different_sizes(tmp_path):
    _, _, data = jc.case("noise_19x37_q95")
    for items in ([data, np.zeros((19, 38, 3), dtype=np.uint8)], [np.zeros((16, 16, 3), dtype=np.uint8), data],
                  [data, jc.case("noise_16x16_q100")[2]]):
        path = str(tmp_path / "bad.avi")
        with pytest.raises(ValueError, match="same size"):
            mjpeg_avi.write_mjpeg_avi(path, items)
        assert not os.path.exists(path)
    with pytest.raises(ValueError, match="JPEG"):
        mjpeg_avi.write_mjpeg_avi(str(tmp_path / "bad.avi"), [b"not a jpeg"])


def test_avi_writer_applies_the_size_limit_to_encoded_items(tmp_path, monkeypatch):
    _, _, data = jc.case("noise_19x37_q95")
    monkeypatch.setattr(mjpeg_avi, "RIFF_LIMIT", 3 * len(data))
    path = str(tmp_path / "long.avi")
    with pytest.raises(ValueError, match="4 GiB"):
        mjpeg_avi.write_mjpeg_avi(path, [data] * 4)
    assert not os.path.exists(path)


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_three_entries_are_exported_and_declared():
    from calipsync_amd import _lib, build
    build.build()
    lib = _lib.load()
    counts = {"casync_op_jpeg_header": 5, "casync_op_jpeg_workspace_bytes": 4, "casync_op_jpeg_encode": 13}
    header = open(os.path.join(REPO, "include", "casync_hip.h")).read()
    assert "#define CASYNC_ABI_VERSION 13" in header and _lib.ABI_VERSION == 13 and lib.casync_abi_version() == 13
    for name, n in counts.items():
        assert name in _lib.EXPORTS and len(_lib._PROTOS[name][1]) == n and hasattr(lib, name)
        proto = re.search(name + r"\(([^;]*?)\);", header, re.S)
        assert proto and len(proto.group(1).split(",")) == n, name
    for words in ("baseline JPEG of finished frames", "status 1", "status 2", "one restart interval per block row"):
        assert words in header, words


def test_header_and_workspace_entries_agree_with_the_twin():
    import ctypes
    from calipsync_amd import _lib, build
    build.build()
    lib = _lib.load()
    for h, w, q in ((8, 8, 95), (19, 37, 1), (1080, 1920, 100), (65535, 1, 50)):
        assert jpeg._header_from_lib(h, w, q) == jpeg.jpeg_header(h, w, q)
    buf = (ctypes.c_uint8 * 629)()
    for args in ((0, 8, 95, buf, 629), (8, 65536, 95, buf, 629), (8, 8, 0, buf, 629), (8, 8, 101, buf, 629), (8, 8, 95, buf, 628),
                 (8, 8, 95, None, 629)):
        assert lib.casync_op_jpeg_header(*args) < 0
    rows = 135
    assert lib.casync_op_jpeg_workspace_bytes(16, 1080, 1920, 0) >= 16 * rows * (4 + 2 * 8 * 3 * 1920)
    assert lib.casync_op_jpeg_workspace_bytes(16, 1080, 1920, 0) == lib.casync_op_jpeg_workspace_bytes(16, 1080, 1920, 2 * 8 * 3 * 1920)
    assert lib.casync_op_jpeg_workspace_bytes(3, 19, 37, 100) >= 3 * 3 * 104
    assert lib.casync_op_jpeg_workspace_bytes(0, 8, 8, 0) == 0
    assert lib.casync_op_jpeg_workspace_bytes(-1, 8, 8, 0) < 0 and lib.casync_op_jpeg_workspace_bytes(1, 0, 8, 0) < 0
    # the encode refuses bad arguments before anything is launched: host buffers stand in for device memory
    host = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(host)
    good = [p, 1, 8, 8, 95, 0, p, 4096, p, 4096, p, p, None]
    for i, v in ((1, -1), (2, 0), (2, 65536), (3, 0), (3, 65536), (4, 0), (4, 101), (5, -1), (7, 16), (9, -1), (0, None), (6, None), (8, None),
                 (10, None), (11, None)):
        args = list(good)
        args[i] = v
        assert lib.casync_op_jpeg_encode(*args) < 0, (i, v)
    args = list(good)
    args[1] = 0
    assert lib.casync_op_jpeg_encode(*args) == 0          # batch 0: a no-op
    assert bytes(host) == bytes(4096)
