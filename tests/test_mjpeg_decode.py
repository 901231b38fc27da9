"""The wider decoder subset on the host (no GPU): decode_jpeg_host(subset="mjpeg") against the recorded pixels of
tests/golden/mjpeg_decode_cases.npz and against live Pillow, what parse_jpeg still refuses, the default subset unchanged, and the
fixed-point twin of the device's entropy plan under the new slot maps.  Every comparison is byte equality."""
import io
import struct

import numpy as np
import pytest

import jpeg_decode_cases as jd
import mjpeg_decode_cases as mj
from calipsync_amd import jpeg

NAMES = mj.names()


def test_the_fixture_holds_the_cases_the_generator_lists():
    gen = mj.generator()
    want = [gen.case_name(s, k, h, w, st) for s, sizes in (("422", gen.SIZES_422), ("gray", gen.SIZES_GRAY)) for h, w in sizes
            for st in gen.settings_of(h, w) for k in gen.KINDS] + list(gen.NO_DHT)
    assert NAMES == want
    assert {mj.size_of(n) for n in NAMES if n.startswith("c422")} == {(1, 1), (1, 2), (8, 16), (8, 9), (9, 17), (17, 23), (48, 64), (8, 1031)}
    assert {mj.size_of(n) for n in NAMES if n.startswith("gray")} == {(1, 1), (8, 8), (9, 9), (17, 23), (48, 64)}
    for n in NAMES:                                              # the samplings, and the tables that are really gone
        data = mj.case(n)[0]
        info = jpeg.parse_jpeg(data, subset="mjpeg")
        assert (info.H, info.W) == mj.size_of(n)
        if n.startswith("c422"):
            assert info.subsampling == 1 and info.blocks_per_mcu == 4 and info.slot_components == (0, 0, 1, 2)
            assert info.mcu_grid == ((info.H + 7) // 8, (info.W + 15) // 16)
        if n.startswith("gray"):
            assert info.subsampling == 3 and info.blocks_per_mcu == 1 and info.mcu_grid == ((info.H + 7) // 8, (info.W + 7) // 8)
        if n.endswith("_rstblocks"):
            assert info.restart_interval == 3
    head = lambda n: mj.case(n)[0][:jpeg.parse_jpeg(mj.case(n)[0], subset="mjpeg").scan_offset]
    for n in gen.NO_DHT:
        assert (b"\xff\xc4" in head(n)) == (not n.endswith("_all")), n
    assert [jpeg.parse_jpeg(mj.case(n)[0], subset="mjpeg").subsampling for n in list(gen.NO_DHT)[:4]] == [0, 1, 2, 3]


@pytest.mark.parametrize("name", NAMES)
def test_the_host_twin_equals_the_recorded_pixels_and_live_pillow(name):
    data = mj.case(name)[0]
    got = jpeg.decode_jpeg_host(data, subset="mjpeg")
    assert mj.differences(got, name) == 0
    live = mj.generator().pillow_read(data)
    assert got.shape == live.shape and got.dtype == np.uint8 and int((got != live).sum()) == 0
    assert jpeg.scan_status(data, subset="mjpeg") == 0


@pytest.mark.parametrize("name", NAMES)
def test_sync_states_end_with_the_serial_decoder(name):
    data = mj.case(name)[0]
    info = jpeg.parse_jpeg(data, subset="mjpeg")
    for chunk in mj.CHUNKS:
        res = jpeg.sync_states(info, data, chunk)
        assert (res.states == jpeg.serial_states(info, data, chunk)).all(), chunk
        assert (res.states[:, 1] < info.blocks_per_mcu).all() and (res.states[:, 2] < 64).all()


def _sof_sampling(data: bytes, samp) -> bytes:
    """the file with the sampling bytes of its SOF0 components replaced"""
    at = data.index(b"\xff\xc0")
    out = bytearray(data)
    for i, s in enumerate(samp):
        out[at + 4 + 6 + 3 * i + 1] = s
    return bytes(out)


def test_the_wide_subset_still_refuses_what_is_outside_it():
    from PIL import Image
    rgb = Image.fromarray(mj.generator().frame("smooth", 16, 16)[:, :, ::-1].copy())
    buf = io.BytesIO()
    rgb.save(buf, format="JPEG", progressive=True)
    with pytest.raises(jpeg.JpegUnsupported, match="progressive"):
        jpeg.parse_jpeg(buf.getvalue(), subset="mjpeg")
    buf = io.BytesIO()
    rgb.convert("CMYK").save(buf, format="JPEG")
    with pytest.raises(jpeg.JpegUnsupported, match="CMYK"):
        jpeg.parse_jpeg(buf.getvalue(), subset="mjpeg")
    good = mj.case("c422smooth_8x16_default")[0]
    for samp in ((0x12, 0x11, 0x11), (0x41, 0x11, 0x11)):        # 4:4:0, 4:1:1
        with pytest.raises(jpeg.JpegUnsupported, match="chroma sampling"):
            jpeg.parse_jpeg(_sof_sampling(good, samp), subset="mjpeg")
    # a table id above 1 stays outside, defined or not
    at = good.index(b"\xff\xda")
    bad = bytearray(good)
    bad[at + 4 + 2] = 0x20
    with pytest.raises(jpeg.JpegUnsupported, match="table id above 1"):
        jpeg.parse_jpeg(bytes(bad), subset="mjpeg")
    with pytest.raises(jpeg.JpegUnsupported):
        jpeg.decode_jpeg_host(_sof_sampling(good, (0x12, 0x11, 0x11)), subset="mjpeg")


def test_the_default_subset_is_unchanged():
    for name, what in (("graynoise_8x8_default", "grayscale"), ("c422noise_8x16_default", "chroma sampling other than 4:4:4 and 4:2:0 \\(2x1, 1x1, 1x1\\)"),
                       ("nodht444_48x64_all", "names a table the file does not define")):
        data = mj.case(name)[0]
        for call in (jpeg.parse_jpeg, jpeg.decode_jpeg_host, jpeg.scan_status, lambda d, **kw: jpeg.parse_jpeg(d, subset="baseline")):
            with pytest.raises(jpeg.JpegUnsupported, match=what):
                call(data)
        plan = jpeg.plan_decode([data])
        assert plan.subset == "baseline" and isinstance(plan.infos[0], jpeg.JpegUnsupported) and plan.rec[0, 9] == 1
    # and what the default admits parses alike under both
    for name in ("noise_33x18_default", "smooth_33x18_sub0"):
        data = jd.case(name)[0]
        a, b = jpeg.parse_jpeg(data), jpeg.parse_jpeg(data, subset="mjpeg")
        assert all(repr(getattr(a, k)) == repr(getattr(b, k)) for k in jpeg.JpegInfo.__slots__)
        assert (jpeg.decode_jpeg_host(data, subset="mjpeg") == jpeg.decode_jpeg_host(data)).all()
        pa, pb = jpeg.plan_decode([data]), jpeg.plan_decode([data], subset="mjpeg")
        assert (pa.rec == pb.rec).all() and (pa.blob == pb.blob).all()


def test_a_bad_subset_value_raises():
    data = mj.case("c422noise_8x16_default")[0]
    for call in (lambda: jpeg.parse_jpeg(data, subset="wide"), lambda: jpeg.decode_jpeg_host(data, subset="MJPEG"),
                 lambda: jpeg.scan_status(data, subset=None), lambda: jpeg.plan_decode([data], 0, subset=1),
                 lambda: jpeg.decode_jpeg_device([data], subset="all")):         # raises before any device call
        with pytest.raises(ValueError, match="subset"):
            call()


def test_the_plan_of_a_mixed_batch():
    files = [f for f, _, _ in mj.mixed_batch()]
    plan = jpeg.plan_decode(files, 32, subset="mjpeg")
    assert plan.subset == "mjpeg" and list(plan.rec[:, 2]) == [0, 1, 2, 3] and list(plan.rec[:, 9]) == [0, 0, 0, 0]
    assert (plan.H, plan.W) == (48, 64)
    tab = plan.blob[plan.rec[3, 6]:plan.rec[3, 6] + jpeg.TAB_BYTES]                     # gray: component 0 alone
    q = np.frombuffer(tab[:384].tobytes(), dtype=np.uint16).reshape(3, 64)
    assert q[0].min() >= 1 and not q[1:].any() and not tab[384:392].any()


@pytest.mark.parametrize("name", mj.MALFORMED)
def test_malformed_scans_have_a_status(name):
    a, bad, b = mj.malformed()[name]
    want = {"invalid_code": 1, "zrl_overrun": 1, "too_few_blocks": 2, "too_many_blocks": 3, "cut_in_half": (1, 2)}[name.split("_", 1)[1]]
    st = jpeg.scan_status(bad, subset="mjpeg")
    assert st in want if isinstance(want, tuple) else st == want
    with pytest.raises(jpeg.JpegCorrupt):
        jpeg.decode_jpeg_host(bad, subset="mjpeg")
    assert jpeg.scan_status(a, subset="mjpeg") == 0 and jpeg.scan_status(b, subset="mjpeg") == 0
    assert struct.unpack(">HH", a[a.index(b"\xff\xc0") + 5:][:4]) == struct.unpack(">HH", bad[bad.index(b"\xff\xc0") + 5:][:4])
