"""The ledger rule for the fifteenth object directory, calipsync_amd/lib/obj_mjpegdec/ (no GPU): every kernel compiled from
csrc/jpeg_dec_mjpeg.hip has a case in tests/kernel_ledger_mjpegdec.py and the other way round, no kernel name occurs in another
object directory or another ledger (the baseline decoder's four kernels keep their names in lib/obj_jpegdec/), the kernels use no
scratch, the plan kernel's LDS leaves room for two workgroups on a CU, and the build's op_sel check stays clean on the object."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

import kernel_ledger  # noqa: E402
import kernel_ledger_audio  # noqa: E402
import kernel_ledger_clip  # noqa: E402
import kernel_ledger_det  # noqa: E402
import kernel_ledger_det16  # noqa: E402
import kernel_ledger_face  # noqa: E402
import kernel_ledger_hb16  # noqa: E402
import kernel_ledger_jpeg  # noqa: E402
import kernel_ledger_jpeg420  # noqa: E402
import kernel_ledger_jpegdec  # noqa: E402
import kernel_ledger_lmk  # noqa: E402
import kernel_ledger_mjpegdec  # noqa: E402
import kernel_ledger_nms  # noqa: E402
import kernel_ledger_sync  # noqa: E402
import kernel_ledger_sync16  # noqa: E402
from calipsync_amd import build  # noqa: E402

pytestmark = pytest.mark.skipif(not kernel_resources.tools_available(), reason="llvm binutils of the ROCm image not found")

OTHER_DIRS = (build.OBJ_DIR, build.OBJ_DIR_HB16, build.OBJ_DIR_LMK, build.OBJ_DIR_DET, build.OBJ_DIR_DET16, build.OBJ_DIR_FACE,
              build.OBJ_DIR_NMS, build.OBJ_DIR_CLIP, build.OBJ_DIR_JPEG, build.OBJ_DIR_JPEG420, build.OBJ_DIR_JPEGDEC, build.OBJ_DIR_SYNC,
              build.OBJ_DIR_SYNC16, build.OBJ_DIR_AUDIO)
OTHER_LEDGERS = (kernel_ledger, kernel_ledger_hb16, kernel_ledger_lmk, kernel_ledger_det, kernel_ledger_det16, kernel_ledger_face,
                 kernel_ledger_nms, kernel_ledger_clip, kernel_ledger_jpeg, kernel_ledger_jpeg420, kernel_ledger_jpegdec, kernel_ledger_sync,
                 kernel_ledger_sync16, kernel_ledger_audio)
KERNELS = ["mjpegdec_color_kernel", "mjpegdec_idct_kernel", "mjpegdec_sync_kernel", "mjpegdec_write_kernel"]
BASELINE_KERNELS = ["jpegdec_color_kernel", "jpegdec_idct_kernel", "jpegdec_sync_kernel", "jpegdec_write_kernel"]


@pytest.fixture(scope="module")
def objects():
    build.build()                      # no-op when the library is up to date
    d = build.OBJ_DIR_MJPEGDEC
    if not os.path.isdir(d) or not any(f.endswith(".o") for f in os.listdir(d)):
        build.build(force=True)        # a library shipped without its objects: compile them
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".o")]


@pytest.fixture(scope="module")
def table(objects):
    return kernel_resources.table(build.OBJ_DIR_MJPEGDEC)


def test_the_mjpegdec_object_is_in_its_own_directory(objects):
    assert [os.path.basename(o) for o in objects] == ["jpeg_dec_mjpeg.o"]
    assert build.SOURCES_MJPEGDEC == ["jpeg_dec_mjpeg.hip"] and "jpeg_dec_mjpeg.hip" in build.SOURCES
    assert build.OBJ_DIR_MJPEGDEC == os.path.join(build.LIB_DIR, "obj_mjpegdec")
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    assert len({build.OBJ_DIR_MJPEGDEC, *OTHER_DIRS}) == 15
    for d in OTHER_DIRS:
        assert not os.path.exists(os.path.join(d, "jpeg_dec_mjpeg.o")), d
    assert sorted(f for f in os.listdir(build.OBJ_DIR_JPEGDEC) if f.endswith(".o")) == ["jpeg_dec.o"]
    # source_hash() covers the new source and the header the two decoders share: without either the hash is another one
    with_dec = build.source_hash()
    sources, headers = build.SOURCES, build.HEADERS
    assert "jpeg_dec_common.h" in headers
    try:
        build.SOURCES = [s for s in sources if s not in build.SOURCES_MJPEGDEC]
        assert build.source_hash() != with_dec
        build.SOURCES, build.HEADERS = sources, [h for h in headers if h != "jpeg_dec_common.h"]
        assert build.source_hash() != with_dec
    finally:
        build.SOURCES, build.HEADERS = sources, headers
    assert build.source_hash() == with_dec


def test_is_stale_sees_the_mjpegdec_source_and_the_shared_header(objects, monkeypatch):
    """is_stale() walks SOURCES and HEADERS: either file newer than the library makes it stale"""
    assert not build.is_stale()
    lib_time = os.path.getmtime(build.LIB_PATH)
    real = os.path.getmtime
    for name in ("jpeg_dec_mjpeg.hip", "jpeg_dec_common.h"):
        src = os.path.join(build.CSRC, name)
        with monkeypatch.context() as m:
            m.setattr(os.path, "getmtime", lambda p, src=src: lib_time + 10 if os.path.abspath(p) == src else real(p))
            assert build.is_stale(), name
    assert not build.is_stale()


def test_every_mjpegdec_kernel_has_a_ledger_case(table):
    assert sorted(table) == KERNELS, sorted(table)
    missing = sorted(set(table) - set(kernel_ledger_mjpegdec.LEDGER))
    stale = sorted(set(kernel_ledger_mjpegdec.LEDGER) - set(table))
    assert not missing, f"kernel instances without a case in tests/kernel_ledger_mjpegdec.py: {missing}"
    assert not stale, f"ledger entries for kernels lib/obj_mjpegdec no longer has: {stale}"
    empty = [k for k, cs in kernel_ledger_mjpegdec.LEDGER.items() if not cs or not all(isinstance(c, kernel_ledger.Case) for c in cs)]
    assert not empty, empty
    listed = {c for cs in kernel_ledger_mjpegdec.LEDGER.values() for c in cs}
    assert listed == {c for _, _, c in kernel_ledger_mjpegdec.cases()}              # every case is one GPU test


def test_no_kernel_name_is_in_another_directory_or_ledger(table):
    other_ledgers = set()
    for ledger in OTHER_LEDGERS:
        other_ledgers |= set(ledger.LEDGER)
    others = set(other_ledgers)
    for d in OTHER_DIRS:
        others |= set(kernel_resources.table(d))
    both = sorted(set(table) & others)
    assert not both, both
    assert not set(kernel_ledger_mjpegdec.LEDGER) & other_ledgers
    assert sorted(kernel_resources.table(build.OBJ_DIR_JPEGDEC)) == BASELINE_KERNELS          # the baseline decoder kept its four names


def test_the_mjpegdec_kernels_use_no_scratch(table):
    spills = {k: v["scratch"] for k, v in table.items() if v["scratch"]}
    assert not spills, spills
    assert table["mjpegdec_sync_kernel"]["static_lds"] <= 65536, table      # two workgroups of it fit a CU's 160 KB


def test_mjpegdec_object_is_free_of_the_op_sel_erratum(objects):
    assert objects
    for obj in objects:
        assert build.erratum_instructions(obj) == [], obj
