"""The ledger rule for the thirteenth object directory, calipsync_amd/lib/obj_sync16/ (no GPU): every kernel compiled from
csrc/syncnet_bf16.hip has a case in tests/kernel_ledger_sync16.py and the other way round, no kernel name occurs in another
object directory or another ledger, the kernels use no scratch and stay within 32 KB of LDS, and the build's op_sel check stays
clean on the object (these kernels issue v_mfma_f32_16x16x32_bf16 on a device where fp32 handles may run)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

import kernel_ledger  # noqa: E402
import kernel_ledger_clip  # noqa: E402
import kernel_ledger_det  # noqa: E402
import kernel_ledger_det16  # noqa: E402
import kernel_ledger_face  # noqa: E402
import kernel_ledger_hb16  # noqa: E402
import kernel_ledger_jpeg  # noqa: E402
import kernel_ledger_jpeg420  # noqa: E402
import kernel_ledger_jpegdec  # noqa: E402
import kernel_ledger_lmk  # noqa: E402
import kernel_ledger_nms  # noqa: E402
import kernel_ledger_sync  # noqa: E402
import kernel_ledger_sync16  # noqa: E402
from calipsync_amd import build  # noqa: E402

pytestmark = pytest.mark.skipif(not kernel_resources.tools_available(), reason="llvm binutils of the ROCm image not found")

OTHER_DIRS = (build.OBJ_DIR, build.OBJ_DIR_HB16, build.OBJ_DIR_LMK, build.OBJ_DIR_DET, build.OBJ_DIR_DET16, build.OBJ_DIR_FACE,
              build.OBJ_DIR_NMS, build.OBJ_DIR_CLIP, build.OBJ_DIR_JPEG, build.OBJ_DIR_JPEG420, build.OBJ_DIR_JPEGDEC, build.OBJ_DIR_SYNC)
OTHER_LEDGERS = (kernel_ledger, kernel_ledger_hb16, kernel_ledger_lmk, kernel_ledger_det, kernel_ledger_det16, kernel_ledger_face,
                 kernel_ledger_nms, kernel_ledger_clip, kernel_ledger_jpeg, kernel_ledger_jpeg420, kernel_ledger_jpegdec, kernel_ledger_sync)
KERNELS = ["sync16_conv_kernel<1, 16>", "sync16_conv_kernel<3, 16>", "sync16_conv_kernel<3, 64>", "sync16_conv_kernel<5, 64>", "sync16_stem7_kernel",
           "sync16_to_nchw_kernel"]


@pytest.fixture(scope="module")
def objects():
    build.build()                      # no-op when the library is up to date
    d = build.OBJ_DIR_SYNC16
    if not os.path.isdir(d) or not any(f.endswith(".o") for f in os.listdir(d)):
        build.build(force=True)        # a library shipped without its objects: compile them
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".o")]


@pytest.fixture(scope="module")
def table(objects):
    return kernel_resources.table(build.OBJ_DIR_SYNC16)


def test_the_sync16_object_is_in_its_own_directory(objects):
    assert [os.path.basename(o) for o in objects] == ["syncnet_bf16.o"]
    assert build.SOURCES_SYNC16 == ["syncnet_bf16.hip"] and "syncnet_bf16.hip" in build.SOURCES
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    assert len({build.OBJ_DIR_SYNC16, *OTHER_DIRS}) == 13
    for d in OTHER_DIRS:
        assert not os.path.exists(os.path.join(d, "syncnet_bf16.o")), d
    assert sorted(f for f in os.listdir(build.OBJ_DIR_SYNC) if f.endswith(".o")) == ["syncnet.o"]
    # source_hash() covers the new source: without it the hash is another one
    with_sync16 = build.source_hash()
    sources = build.SOURCES
    try:
        build.SOURCES = [s for s in sources if s not in build.SOURCES_SYNC16]
        assert build.source_hash() != with_sync16
    finally:
        build.SOURCES = sources


@pytest.mark.parametrize("name", ["syncnet_bf16.hip", "syncnet_common.h"])
def test_is_stale_sees_the_sync16_source_and_the_shared_header(objects, monkeypatch, name):
    """is_stale() walks SOURCES and HEADERS: either file newer than the library makes it stale"""
    assert not build.is_stale()
    src = os.path.join(build.CSRC, name)
    lib_time = os.path.getmtime(build.LIB_PATH)
    real = os.path.getmtime
    monkeypatch.setattr(os.path, "getmtime", lambda p: lib_time + 10 if os.path.abspath(p) == src else real(p))
    assert build.is_stale()


def test_every_sync16_kernel_has_a_ledger_case(table):
    assert sorted(table) == KERNELS, sorted(table)
    missing = sorted(set(table) - set(kernel_ledger_sync16.LEDGER))
    stale = sorted(set(kernel_ledger_sync16.LEDGER) - set(table))
    assert not missing, f"kernel instances without a case in tests/kernel_ledger_sync16.py: {missing}"
    assert not stale, f"ledger entries for kernels lib/obj_sync16 no longer has: {stale}"
    empty = [k for k, cs in kernel_ledger_sync16.LEDGER.items() if not cs or not all(isinstance(c, kernel_ledger.Case) for c in cs)]
    assert not empty, empty
    listed = {c for cs in kernel_ledger_sync16.LEDGER.values() for c in cs}
    assert listed == {c for _, _, c in kernel_ledger_sync16.cases()}              # every case is one GPU test


def test_no_kernel_name_is_in_another_directory_or_ledger(table):
    other_ledgers = set()
    for ledger in OTHER_LEDGERS:
        other_ledgers |= set(ledger.LEDGER)
    others = set(other_ledgers)
    for d in OTHER_DIRS:
        others |= set(kernel_resources.table(d))
    both = sorted(set(table) & others)
    assert not both, both
    assert not set(kernel_ledger_sync16.LEDGER) & other_ledgers


def test_the_sync16_kernels_use_no_scratch_and_at_most_32_kb_of_lds(table):
    spills = {k: v["scratch"] for k, v in table.items() if v["scratch"]}
    assert not spills, spills
    assert all(v["static_lds"] <= 32768 for v in table.values()), table


def test_sync16_object_is_free_of_the_op_sel_erratum(objects):
    assert objects
    for obj in objects:
        assert build.erratum_instructions(obj) == [], obj
