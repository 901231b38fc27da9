"""The ledger rule for the fourth object directory, calipsync_amd/lib/obj_det/ (no GPU): every kernel compiled from
csrc/facedet.hip has a case in tests/kernel_ledger_det.py and the other way round, no kernel name occurs in another object
directory or another ledger, none of these kernels uses scratch, and their code is free of the packed-fp32 op_sel forms the
build refuses to link."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

import kernel_ledger  # noqa: E402
import kernel_ledger_det  # noqa: E402
import kernel_ledger_hb16  # noqa: E402
import kernel_ledger_lmk  # noqa: E402
from calipsync_amd import build  # noqa: E402

pytestmark = pytest.mark.skipif(not kernel_resources.tools_available(), reason="llvm binutils of the ROCm image not found")


@pytest.fixture(scope="module")
def objects():
    build.build()                      # no-op when the library is up to date
    d = build.OBJ_DIR_DET
    if not os.path.isdir(d) or not any(f.endswith(".o") for f in os.listdir(d)):
        build.build(force=True)        # a library shipped without its objects: compile them
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".o")]


@pytest.fixture(scope="module")
def table(objects):
    return kernel_resources.table(build.OBJ_DIR_DET)


def test_fourth_object_directory_is_part_of_the_build(monkeypatch, tmp_path):
    assert build.OBJ_DIR_DET not in (build.OBJ_DIR, build.OBJ_DIR_HB16, build.OBJ_DIR_LMK) and build.SOURCES_DET == ["facedet.hip"]
    assert "facedet.hip" in build.SOURCES and "facedet.hip" not in build.SOURCES_HB16 + build.SOURCES_LMK
    src = os.path.join(build.CSRC, "facedet.hip")
    assert os.path.exists(src)
    rest = [s for s in build.SOURCES if s != "facedet.hip"]
    # source_hash() covers the new source: without it the hash is another one
    with_det = build.source_hash()
    monkeypatch.setattr(build, "SOURCES", rest)
    assert build.source_hash() != with_det
    monkeypatch.undo()
    # is_stale() looks at it: a library older than facedet.hip alone is stale (a stand-in library file, nothing is touched)
    lib = tmp_path / "libcasync_hip.so"
    lib.write_bytes(b"")
    os.utime(lib, (os.path.getmtime(src) - 10, os.path.getmtime(src) - 10))
    monkeypatch.setattr(build, "LIB_PATH", str(lib))
    monkeypatch.setattr(build, "SOURCES", ["facedet.hip"])
    monkeypatch.setattr(build, "SOURCES_HB16", [])
    monkeypatch.setattr(build, "SOURCES_LMK", [])
    monkeypatch.setattr(build, "HEADERS", [])
    assert build.is_stale()
    monkeypatch.setattr(build, "SOURCES", [])
    assert not build.is_stale()


def test_the_detector_object_is_not_in_the_main_directory(objects):
    assert [os.path.basename(o) for o in objects] == ["facedet.o"]
    assert not os.path.exists(os.path.join(build.OBJ_DIR, "facedet.o"))


def test_every_det_kernel_has_a_ledger_case(table):
    assert table, "no kernel found in lib/obj_det"
    missing = sorted(set(table) - set(kernel_ledger_det.LEDGER))
    stale = sorted(set(kernel_ledger_det.LEDGER) - set(table))
    assert not missing, f"kernel instances without a case in tests/kernel_ledger_det.py: {missing}"
    assert not stale, f"ledger entries for kernels lib/obj_det no longer has: {stale}"
    empty = [k for k, cs in kernel_ledger_det.LEDGER.items() if not cs or not all(isinstance(c, kernel_ledger.Case) for c in cs)]
    assert not empty, empty


def test_no_kernel_name_is_in_another_directory_or_ledger(table):
    other_ledgers = set(kernel_ledger.LEDGER) | set(kernel_ledger_hb16.LEDGER) | set(kernel_ledger_lmk.LEDGER)
    others = set(kernel_resources.table()) | set(kernel_resources.table(build.OBJ_DIR_HB16)) | set(kernel_resources.table(build.OBJ_DIR_LMK)) | \
        other_ledgers
    both = sorted(set(table) & others)
    assert not both, both
    assert not set(kernel_ledger_det.LEDGER) & other_ledgers


def test_det_kernels_use_no_scratch(table):
    spills = {k: v["scratch"] for k, v in table.items() if v["scratch"]}
    assert not spills, spills


def test_det_objects_are_free_of_the_op_sel_erratum(objects):
    assert objects
    for obj in objects:
        assert build.erratum_instructions(obj) == [], obj
