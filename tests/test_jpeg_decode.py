"""The JPEG decoder without a GPU: calipsync_amd/jpeg.py parse_jpeg, decode_jpeg_host (the numpy twin of csrc/jpeg_dec.hip) and
sync_states (the host model of the device's entropy plan).  Every comparison is byte equality with Pillow (libjpeg-turbo)."""
import io

import numpy as np
import pytest

import jpeg420_cases as j4
import jpeg_cases as jc
import jpeg_decode_cases as jd
from calipsync_amd import jpeg


def _pillow(data):
    return np.ascontiguousarray(jc.decode(data)[:, :, ::-1])


@pytest.mark.parametrize("name", jd.names())
def test_host_decoder_equals_the_fixture_and_live_pillow(name):
    data, _, _ = jd.case(name)
    got = jpeg.decode_jpeg_host(data)
    assert got.shape == jd.size_of(name) + (3,) and got.dtype == np.uint8
    diff = jd.differences(got, name)
    live = int((got != _pillow(data)).sum())
    print(f"{name}: {diff:.0f} bytes differ from the fixture, {live} from live Pillow")
    assert diff == 0 and live == 0


def test_the_fixture_is_what_its_generator_writes_here():
    gen = jd.generator()
    for name in ("noise_17x33_default", "smooth_33x18_optimize", "noise_48x64_rstblocks", "noise_7x5_q100"):
        kind, size, setting = name.split("_")
        h, w = jd.size_of(name)
        data = gen.pillow_write(gen.frame(kind, h, w), **gen.SETTINGS[setting])
        assert data == jd.case(name)[0], name


@pytest.mark.parametrize("sub", ["4:4:4", "4:2:0"])
def test_host_decoder_reads_this_repos_encoder(sub):
    for h, w, seed in ((1, 1, 1), (17, 33, 2), (33, 18, 3), (48, 64, 4)):
        data = jpeg.encode_jpeg_host(j4.seeded(h, w, seed), 90, sub)
        assert int((jpeg.decode_jpeg_host(data) != _pillow(data)).sum()) == 0, (h, w)


@pytest.mark.parametrize("cases", [jc, j4], ids=["jpeg_cases", "jpeg420_cases"])
def test_host_decoder_reads_the_encoders_recorded_files(cases):
    for name in cases.names():
        data = cases.case(name)[2]
        got = jpeg.decode_jpeg_host(data)
        assert int((got != _pillow(data)).sum()) == 0, name


def test_parse_reads_what_the_headers_say():
    info = jpeg.parse_jpeg(jd.case("noise_33x18_rstblocks")[0])
    assert (info.H, info.W, info.subsampling, info.restart_interval) == (33, 18, 2, 3)
    assert len(info.restart_offsets) == info.expected_segments() - 1 == 1 and info.blocks_per_mcu == 6
    assert [len(q) for q in info.qtables] == [64, 64, 64] and info.dc_sel == (0, 1, 1) and info.ac_sel == (0, 1, 1)
    info = jpeg.parse_jpeg(jd.case("noise_33x18_sub0")[0])
    assert (info.subsampling, info.restart_interval, len(info.restart_offsets), info.mcu_grid) == (0, 0, 0, (5, 3))
    data = jd.case("smooth_48x64_optimize")[0]
    info = jpeg.parse_jpeg(data)
    assert info.dc_tables[0] != jpeg.DC_LUMA and data[info.scan_offset + info.scan_length:] == b"\xff\xd9"


def _written(mode, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.new(mode, (24, 16)).save(buf, format="JPEG", **kw)
    return buf.getvalue()


@pytest.mark.parametrize("what,data", [("progressive", lambda: _written("RGB", progressive=True)), ("grayscale", lambda: _written("L")),
                                       ("CMYK", lambda: _written("CMYK")), ("sampling", lambda: _written("RGB", subsampling=1)),
                                       ("ends inside its headers", lambda: jd.case("noise_8x8_default")[0][:300])])
def test_parse_refuses_what_is_outside_the_subset(what, data):
    with pytest.raises(jpeg.JpegUnsupported, match=what):
        jpeg.parse_jpeg(data())
    assert issubclass(jpeg.JpegUnsupported, ValueError)


def _q95_256():
    """the 256 x 256 quality-95 file without restart markers: a smooth frame with a patch of noise"""
    return jd.generator().pillow_write(j4.seeded(256, 256, 11), quality=95)


SYNC_FILES = {"q95_256x256": _q95_256, "noise_48x64_q100": lambda: jd.case("noise_48x64_q100")[0],
              "smooth_256x256_rstblocks": lambda: jd.case("smooth_256x256_rstblocks")[0]}


@pytest.mark.parametrize("chunk_bits", [32, 64, 256, 1024, jd.BIG_CHUNK])
@pytest.mark.parametrize("which", list(SYNC_FILES))
def test_sync_states_are_the_serial_decoders(which, chunk_bits):
    data = SYNC_FILES[which]()
    info = jpeg.parse_jpeg(data)
    if which == "noise_48x64_q100":
        assert data.count(b"\xff\x00") > 20                       # dense in stuffed bytes
    got = jpeg.sync_states(info, data, chunk_bits)
    want = jpeg.serial_states(info, data, chunk_bits)
    late = int((got.rounds > 2).sum())
    print(f"{which} chunk_bits {chunk_bits}: {len(want)} subsequences, {got.total_rounds} rounds, {late} needed more than two")
    assert got.states.shape == want.shape and int((got.states != want).sum()) == 0
    segs = info.segments()
    assert len(want) == sum(max(1, -(-(b - a) * 8 // chunk_bits)) for a, b in segs)
    if chunk_bits == jd.BIG_CHUNK:
        assert len(want) == len(segs) and got.total_rounds == 1
    if which == "smooth_256x256_rstblocks" and chunk_bits == 1024:
        assert max(b - a for a, b in segs) * 8 < chunk_bits        # every segment is shorter than a subsequence
    if chunk_bits == 32:
        assert late > 0                                            # the late-synchronisation path is reached


def test_chunk_bits_are_checked():
    data = jd.case("noise_8x8_default")[0]
    for bad in (8, 33, -32, (1 << 30) + 32):
        with pytest.raises(ValueError, match="chunk_bits"):
            jpeg.sync_states(jpeg.parse_jpeg(data), data, bad)


def test_malformed_scans_are_classified():
    for name, (_, bad, _) in jd.malformed().items():
        st = jpeg.scan_status(bad)
        print(name, st)
        assert st in (1, 2, 3), name
        with pytest.raises(jpeg.JpegCorrupt) as exc:
            jpeg.decode_jpeg_host(bad)
        assert exc.value.status == st
    assert jpeg.scan_status(jd.malformed()["zrl_overrun"][1]) == 1
    assert jpeg.scan_status(jd.malformed()["too_many_blocks"][1]) == 3
    assert jpeg.scan_status(jd.malformed()["cut_in_half"][1]) == 2
    for name in ("noise_48x64_default", "smooth_17x33_rstrows"):
        assert jpeg.scan_status(jd.case(name)[0]) == 0


def test_the_device_tables_hold_every_code():
    """the table block of csrc/jpeg_dec.hip decodes every code of every table to its symbol and length"""
    for name in ("noise_48x64_default", "smooth_48x64_optimize"):
        info = jpeg.parse_jpeg(jd.case(name)[0])
        for bits, vals in info.dc_tables + info.ac_tables:
            blob = jpeg._device_huffman(bits, vals)
            lut = np.frombuffer(blob[:512], dtype=np.uint16)
            maxcode, valoff = np.frombuffer(blob[512:544], dtype=np.int32), np.frombuffer(blob[544:576], dtype=np.int32)
            code, k = 0, 0
            for length in range(1, 17):
                for _ in range(bits[length - 1]):
                    if length <= 8:
                        assert lut[code << (8 - length)] == (length << 8 | vals[k])
                    else:
                        assert lut[code >> (length - 8)] == 0 and code <= maxcode[length - 9]
                        assert all(code >> (length - l) > maxcode[l - 9] for l in range(9, length))
                        assert blob[576 + code + valoff[length - 9]] == vals[k]
                    code += 1
                    k += 1
                code <<= 1
        assert len(jpeg._device_tables(info)) == jpeg.TAB_BYTES


def test_decode_against_cv2(tmp_path):
    cv2 = pytest.importorskip("cv2")
    for name in ("noise_33x18_default", "smooth_48x64_sub0"):
        data = jd.case(name)[0]
        path = tmp_path / "f.jpg"
        path.write_bytes(data)
        assert int((jpeg.decode_jpeg_host(data) != cv2.imread(str(path))).sum()) == 0, name


def test_a_short_dri_segment_is_refused_not_crashed_on():
    data = jd.case("noise_33x18_rstblocks")[0]
    at = data.index(b"\xff\xdd\x00\x04")
    short = data[:at] + b"\xff\xdd\x00\x03\x00" + data[at + 6:]
    with pytest.raises(jpeg.JpegUnsupported, match="DRI"):
        jpeg.parse_jpeg(short)
    plan = jpeg.plan_decode([data, short])
    assert isinstance(plan.infos[1], jpeg.JpegUnsupported) and list(plan.rec[:, 9]) == [0, 1]


def test_a_frame_above_the_subsequence_cap_takes_the_host_path(monkeypatch):
    data = jd.case("noise_256x256_q100")[0]
    plan = jpeg.plan_decode([data], 32)
    assert isinstance(plan.infos[0], jpeg.JpegInfo) and 0 < plan.total_sub <= jpeg.MAX_SUBSEQUENCES
    monkeypatch.setattr(jpeg, "MAX_SUBSEQUENCES", plan.total_sub - 1)
    over = jpeg.plan_decode([data, jd.case("smooth_256x256_default")[0]], 32)
    assert isinstance(over.infos[0], jpeg.JpegUnsupported) and "subsequences" in str(over.infos[0])
    assert list(over.rec[:, 9]) == [1, 0] and list(over.rec[0, :8]) == [0] * 8 and over.rec[1, 8] == 0
