"""The ledger rule for the fifth object directory, calipsync_amd/lib/obj_det16/ (no GPU): every kernel compiled from
csrc/facedet_bf16.hip has a case in tests/kernel_ledger_det16.py and the other way round, no kernel name occurs in another
object directory or another ledger, none of these kernels uses scratch, and their code is free of the packed-fp32 op_sel forms
the build refuses to link (the handle issues v_mfma_f32_16x16x32_bf16 on a device where fp32 handles may run)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

import kernel_ledger  # noqa: E402
import kernel_ledger_det  # noqa: E402
import kernel_ledger_det16  # noqa: E402
import kernel_ledger_hb16  # noqa: E402
import kernel_ledger_lmk  # noqa: E402
from calipsync_amd import build  # noqa: E402

pytestmark = pytest.mark.skipif(not kernel_resources.tools_available(), reason="llvm binutils of the ROCm image not found")

OTHER_DIRS = (build.OBJ_DIR, build.OBJ_DIR_HB16, build.OBJ_DIR_LMK, build.OBJ_DIR_DET)


@pytest.fixture(scope="module")
def objects():
    build.build()                      # no-op when the library is up to date
    d = build.OBJ_DIR_DET16
    if not os.path.isdir(d) or not any(f.endswith(".o") for f in os.listdir(d)):
        build.build(force=True)        # a library shipped without its objects: compile them
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".o")]


@pytest.fixture(scope="module")
def table(objects):
    return kernel_resources.table(build.OBJ_DIR_DET16)


def test_fifth_object_directory_is_part_of_the_build(monkeypatch, tmp_path):
    assert build.OBJ_DIR_DET16 not in OTHER_DIRS and build.SOURCES_DET16 == ["facedet_bf16.hip"] and build.SOURCES_DET == ["facedet.hip"]
    assert "facedet_bf16.hip" in build.SOURCES and "facedet_bf16.hip" not in build.SOURCES_HB16 + build.SOURCES_LMK + build.SOURCES_DET
    src = os.path.join(build.CSRC, "facedet_bf16.hip")
    assert os.path.exists(src)
    rest = [s for s in build.SOURCES if s != "facedet_bf16.hip"]
    with_det16 = build.source_hash()
    monkeypatch.setattr(build, "SOURCES", rest)
    assert build.source_hash() != with_det16
    monkeypatch.undo()
    # is_stale() looks at it: a library older than facedet_bf16.hip alone is stale (a stand-in library file, nothing is touched)
    lib = tmp_path / "libcasync_hip.so"
    lib.write_bytes(b"")
    os.utime(lib, (os.path.getmtime(src) - 10, os.path.getmtime(src) - 10))
    monkeypatch.setattr(build, "LIB_PATH", str(lib))
    monkeypatch.setattr(build, "SOURCES", ["facedet_bf16.hip"])
    monkeypatch.setattr(build, "SOURCES_HB16", [])
    monkeypatch.setattr(build, "SOURCES_LMK", [])
    monkeypatch.setattr(build, "HEADERS", [])
    assert build.is_stale()
    monkeypatch.setattr(build, "SOURCES", [])
    assert not build.is_stale()


def test_the_bf16_detector_object_is_in_its_own_directory(objects):
    assert [os.path.basename(o) for o in objects] == ["facedet_bf16.o"]
    for d in OTHER_DIRS:
        assert not os.path.exists(os.path.join(d, "facedet_bf16.o")), d
    assert sorted(f for f in os.listdir(build.OBJ_DIR_DET) if f.endswith(".o")) == ["facedet.o"]


def test_every_det16_kernel_has_a_ledger_case(table):
    assert table, "no kernel found in lib/obj_det16"
    missing = sorted(set(table) - set(kernel_ledger_det16.LEDGER))
    stale = sorted(set(kernel_ledger_det16.LEDGER) - set(table))
    assert not missing, f"kernel instances without a case in tests/kernel_ledger_det16.py: {missing}"
    assert not stale, f"ledger entries for kernels lib/obj_det16 no longer has: {stale}"
    empty = [k for k, cs in kernel_ledger_det16.LEDGER.items() if not cs or not all(isinstance(c, kernel_ledger.Case) for c in cs)]
    assert not empty, empty


def test_no_kernel_name_is_in_another_directory_or_ledger(table):
    other_ledgers = set(kernel_ledger.LEDGER) | set(kernel_ledger_hb16.LEDGER) | set(kernel_ledger_lmk.LEDGER) | set(kernel_ledger_det.LEDGER)
    others = set(other_ledgers)
    for d in OTHER_DIRS:
        others |= set(kernel_resources.table(d))
    both = sorted(set(table) & others)
    assert not both, both
    assert not set(kernel_ledger_det16.LEDGER) & other_ledgers


def test_det16_kernels_use_no_scratch(table):
    spills = {k: v["scratch"] for k, v in table.items() if v["scratch"]}
    assert not spills, spills


def test_det16_objects_are_free_of_the_op_sel_erratum(objects):
    assert objects
    for obj in objects:
        assert build.erratum_instructions(obj) == [], obj
