"""The ledger rule for the seventeenth object directory, calipsync_amd/lib/obj_ploss/ (no GPU): every kernel compiled from
csrc/ploss.hip has a case in tests/kernel_ledger_ploss.py and the other way round, no kernel name occurs in another object
directory or another ledger, the kernels use no scratch, only the three reductions use LDS (2 KB each), the source uses no
global atomic, and the build's op_sel check stays clean on the object."""
import os
import re
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
import kernel_ledger_ploss  # noqa: E402
import kernel_ledger_sync  # noqa: E402
import kernel_ledger_sync16  # noqa: E402
import kernel_ledger_train  # noqa: E402
from calipsync_amd import build  # noqa: E402

pytestmark = pytest.mark.skipif(not kernel_resources.tools_available(), reason="llvm binutils of the ROCm image not found")

OTHER_DIRS = (build.OBJ_DIR, build.OBJ_DIR_HB16, build.OBJ_DIR_LMK, build.OBJ_DIR_DET, build.OBJ_DIR_DET16, build.OBJ_DIR_FACE,
              build.OBJ_DIR_NMS, build.OBJ_DIR_CLIP, build.OBJ_DIR_JPEG, build.OBJ_DIR_JPEG420, build.OBJ_DIR_JPEGDEC, build.OBJ_DIR_SYNC,
              build.OBJ_DIR_SYNC16, build.OBJ_DIR_AUDIO, build.OBJ_DIR_MJPEGDEC, build.OBJ_DIR_TRAIN)
OTHER_LEDGERS = (kernel_ledger, kernel_ledger_hb16, kernel_ledger_lmk, kernel_ledger_det, kernel_ledger_det16, kernel_ledger_face,
                 kernel_ledger_nms, kernel_ledger_clip, kernel_ledger_jpeg, kernel_ledger_jpeg420, kernel_ledger_jpegdec, kernel_ledger_sync,
                 kernel_ledger_sync16, kernel_ledger_audio, kernel_ledger_mjpegdec, kernel_ledger_train)
KERNELS = sorted(["ploss_stem_kernel", "ploss_pool_kernel", "ploss_wflip_kernel", "ploss_relu_bwd_kernel", "ploss_pool_bwd_kernel",
                  "ploss_stem_bwd_kernel", "ploss_split_kernel", "ploss_combine_kernel", "ploss_sqdiff_kernel", "ploss_absdiff_kernel", "ploss_finish_kernel"])
REDUCTIONS = {"ploss_sqdiff_kernel", "ploss_absdiff_kernel", "ploss_finish_kernel"}
PLOSS_H = os.path.join("..", "..", "include", "casync_ploss.h")


@pytest.fixture(scope="module")
def objects():
    build.build()                      # no-op when the library is up to date
    d = build.OBJ_DIR_PLOSS
    if not os.path.isdir(d) or not any(f.endswith(".o") for f in os.listdir(d)):
        build.build(force=True)        # a library shipped without its objects: compile them
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".o")]


@pytest.fixture(scope="module")
def table(objects):
    return kernel_resources.table(build.OBJ_DIR_PLOSS)


def test_the_ploss_object_is_in_its_own_directory(objects):
    assert [os.path.basename(o) for o in objects] == ["ploss.o"]
    assert build.SOURCES_PLOSS == ["ploss.hip"] and "ploss.hip" in build.SOURCES
    assert build.OBJ_DIR_PLOSS == os.path.join(build.LIB_DIR, "obj_ploss")
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    assert len({build.OBJ_DIR_PLOSS, *OTHER_DIRS}) == 17
    for d in OTHER_DIRS:
        assert not os.path.exists(os.path.join(d, "ploss.o")), d
    assert sorted(f for f in os.listdir(build.OBJ_DIR_TRAIN) if f.endswith(".o")) == ["train_ops.o"]


def test_source_hash_and_is_stale_cover_the_source_and_its_header(objects, monkeypatch):
    full = build.source_hash()
    assert PLOSS_H in build.HEADERS and os.path.exists(os.path.join(build.CSRC, PLOSS_H))
    sources, headers = build.SOURCES, build.HEADERS
    try:
        build.SOURCES = [s for s in sources if s not in build.SOURCES_PLOSS]
        assert build.source_hash() != full
        build.SOURCES = sources
        build.HEADERS = [h for h in headers if h != PLOSS_H]
        assert build.source_hash() != full
    finally:
        build.SOURCES, build.HEADERS = sources, headers
    assert build.source_hash() == full and not build.is_stale()
    lib_time = os.path.getmtime(build.LIB_PATH)
    real = os.path.getmtime
    for name in ("ploss.hip", PLOSS_H):
        path = os.path.abspath(os.path.join(build.CSRC, name))
        monkeypatch.setattr(os.path, "getmtime", lambda p, path=path: lib_time + 10 if os.path.abspath(p) == path else real(p))
        assert build.is_stale(), name
        monkeypatch.setattr(os.path, "getmtime", real)


def test_every_ploss_kernel_has_a_ledger_case(table):
    assert sorted(table) == KERNELS, sorted(table)
    missing = sorted(set(table) - set(kernel_ledger_ploss.LEDGER))
    stale = sorted(set(kernel_ledger_ploss.LEDGER) - set(table))
    assert not missing, f"kernels without a case in tests/kernel_ledger_ploss.py: {missing}"
    assert not stale, f"ledger entries for kernels lib/obj_ploss no longer has: {stale}"
    empty = [k for k, cs in kernel_ledger_ploss.LEDGER.items() if not cs or not all(isinstance(c, kernel_ledger.Case) for c in cs)]
    assert not empty, empty
    listed = {c for cs in kernel_ledger_ploss.LEDGER.values() for c in cs}
    assert listed == {c for _, _, c in kernel_ledger_ploss.cases()}              # every case is one GPU test
    assert all(len(kernel_ledger_ploss.launched_by(c)) == 1 for c in listed)      # an entry launches one kernel


def test_no_kernel_name_is_in_another_directory_or_ledger(table):
    other_ledgers = set()
    for ledger in OTHER_LEDGERS:
        other_ledgers |= set(ledger.LEDGER)
    others = set(other_ledgers)
    for d in OTHER_DIRS:
        others |= set(kernel_resources.table(d))
    both = sorted(set(table) & others)
    assert not both, both
    assert not set(kernel_ledger_ploss.LEDGER) & other_ledgers


def test_the_ploss_kernels_use_no_scratch_no_atomics_and_little_lds(table):
    spills = {k: v["scratch"] for k, v in table.items() if v["scratch"]}
    assert not spills, spills
    for k, v in table.items():
        assert v["static_lds"] == (2048 if k in REDUCTIONS else 0), (k, v)
    code = re.sub(r"//.*", "", open(os.path.join(build.CSRC, "ploss.hip")).read())
    assert not re.search(r"\batomic\w*\s*\(", code, flags=re.I)          # every output element is written once by one lane
    assert "hipMalloc" not in code.split("int refresh_wt")[0]            # nothing in front of the weight load allocates
    assert "conv3x3_positions" not in code                               # (the table of a geometry would be built inside a forward)


def test_ploss_object_is_free_of_the_op_sel_erratum(objects):
    assert objects
    for obj in objects:
        assert build.erratum_instructions(obj) == [], obj
