"""The ledger rule for the tenth object directory, calipsync_amd/lib/obj_jpeg420/ (no GPU): every kernel compiled from
csrc/jpeg_enc420.hip has a case in tests/kernel_ledger_jpeg420.py and the other way round, no kernel name occurs in another
object directory or another ledger, the kernels use no scratch (a spilling DCT is a defect), the row kernel's LDS leaves room for
two waves on a CU, and the build's op_sel check stays clean on the object."""
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
import kernel_ledger_lmk  # noqa: E402
import kernel_ledger_nms  # noqa: E402
from calipsync_amd import build  # noqa: E402

pytestmark = pytest.mark.skipif(not kernel_resources.tools_available(), reason="llvm binutils of the ROCm image not found")

OTHER_DIRS = (build.OBJ_DIR, build.OBJ_DIR_HB16, build.OBJ_DIR_LMK, build.OBJ_DIR_DET, build.OBJ_DIR_DET16, build.OBJ_DIR_FACE,
              build.OBJ_DIR_NMS, build.OBJ_DIR_CLIP, build.OBJ_DIR_JPEG)
OTHER_LEDGERS = (kernel_ledger, kernel_ledger_hb16, kernel_ledger_lmk, kernel_ledger_det, kernel_ledger_det16, kernel_ledger_face,
                 kernel_ledger_nms, kernel_ledger_clip, kernel_ledger_jpeg)
KERNELS = ["jpeg420_encode_rows_kernel", "jpeg420_pack_kernel", "jpeg420_plan_kernel"]


@pytest.fixture(scope="module")
def objects():
    build.build()                      # no-op when the library is up to date
    d = build.OBJ_DIR_JPEG420
    if not os.path.isdir(d) or not any(f.endswith(".o") for f in os.listdir(d)):
        build.build(force=True)        # a library shipped without its objects: compile them
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".o")]


@pytest.fixture(scope="module")
def table(objects):
    return kernel_resources.table(build.OBJ_DIR_JPEG420)


def test_the_jpeg420_object_is_in_its_own_directory(objects):
    assert [os.path.basename(o) for o in objects] == ["jpeg_enc420.o"]
    assert build.SOURCES_JPEG420 == ["jpeg_enc420.hip"] and "jpeg_enc420.hip" in build.SOURCES
    assert build.SOURCES_JPEG == ["jpeg_enc.hip"] and len(set(build.SOURCES)) == len(build.SOURCES)
    assert len({build.OBJ_DIR_JPEG420, *OTHER_DIRS}) == 10
    for d in OTHER_DIRS:
        assert not os.path.exists(os.path.join(d, "jpeg_enc420.o")), d
    # source_hash() covers the new source: without it the hash is another one
    with_420 = build.source_hash()
    sources = build.SOURCES
    try:
        build.SOURCES = [s for s in sources if s not in build.SOURCES_JPEG420]
        assert build.source_hash() != with_420
    finally:
        build.SOURCES = sources
    # ... and the header the two encoders share
    headers = build.HEADERS
    assert "jpeg_enc_common.h" in headers
    try:
        build.HEADERS = [h for h in headers if h != "jpeg_enc_common.h"]
        assert build.source_hash() != with_420
    finally:
        build.HEADERS = headers


def test_every_jpeg420_kernel_has_a_ledger_case(table):
    assert sorted(table) == KERNELS, sorted(table)
    missing = sorted(set(table) - set(kernel_ledger_jpeg420.LEDGER))
    stale = sorted(set(kernel_ledger_jpeg420.LEDGER) - set(table))
    assert not missing, f"kernel instances without a case in tests/kernel_ledger_jpeg420.py: {missing}"
    assert not stale, f"ledger entries for kernels lib/obj_jpeg420 no longer has: {stale}"
    empty = [k for k, cs in kernel_ledger_jpeg420.LEDGER.items() if not cs or not all(isinstance(c, kernel_ledger.Case) for c in cs)]
    assert not empty, empty
    listed = {c for cs in kernel_ledger_jpeg420.LEDGER.values() for c in cs}
    assert listed == {c for _, _, c in kernel_ledger_jpeg420.cases()}              # every case is one GPU test


def test_no_kernel_name_is_in_another_directory_or_ledger(table):
    other_ledgers = set()
    for ledger in OTHER_LEDGERS:
        other_ledgers |= set(ledger.LEDGER)
    others = set(other_ledgers)
    for d in OTHER_DIRS:
        others |= set(kernel_resources.table(d))
    both = sorted(set(table) & others)
    assert not both, both
    assert not set(kernel_ledger_jpeg420.LEDGER) & other_ledgers


def test_the_jpeg420_kernels_use_no_scratch(table):
    spills = {k: v["scratch"] for k, v in table.items() if v["scratch"]}
    assert not spills, spills
    assert table["jpeg420_encode_rows_kernel"]["static_lds"] <= 65536, table      # two waves of it fit a CU's 160 KB


def test_jpeg420_object_is_free_of_the_op_sel_erratum(objects):
    assert objects
    for obj in objects:
        assert build.erratum_instructions(obj) == [], obj
