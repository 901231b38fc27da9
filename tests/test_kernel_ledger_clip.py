"""The ledger rule for the eighth object directory, calipsync_amd/lib/obj_clip/ (no GPU): every kernel compiled from
csrc/clip_ops.hip has a case in tests/kernel_ledger_clip.py and the other way round, no kernel name occurs in another object
directory or another ledger, the kernels use neither scratch nor LDS, and the build's op_sel check stays clean on the object."""
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
import kernel_ledger_lmk  # noqa: E402
import kernel_ledger_nms  # noqa: E402
from calipsync_amd import build  # noqa: E402

pytestmark = pytest.mark.skipif(not kernel_resources.tools_available(), reason="llvm binutils of the ROCm image not found")

OTHER_DIRS = (build.OBJ_DIR, build.OBJ_DIR_HB16, build.OBJ_DIR_LMK, build.OBJ_DIR_DET, build.OBJ_DIR_DET16, build.OBJ_DIR_FACE,
              build.OBJ_DIR_NMS)


@pytest.fixture(scope="module")
def objects():
    build.build()                      # no-op when the library is up to date
    d = build.OBJ_DIR_CLIP
    if not os.path.isdir(d) or not any(f.endswith(".o") for f in os.listdir(d)):
        build.build(force=True)        # a library shipped without its objects: compile them
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".o")]


@pytest.fixture(scope="module")
def table(objects):
    return kernel_resources.table(build.OBJ_DIR_CLIP)


def test_the_clip_object_is_in_its_own_directory(objects):
    assert [os.path.basename(o) for o in objects] == ["clip_ops.o"]
    for d in OTHER_DIRS:
        assert not os.path.exists(os.path.join(d, "clip_ops.o")), d


def test_every_clip_kernel_has_a_ledger_case(table):
    assert table, "no kernel found in lib/obj_clip"
    missing = sorted(set(table) - set(kernel_ledger_clip.LEDGER))
    stale = sorted(set(kernel_ledger_clip.LEDGER) - set(table))
    assert not missing, f"kernel instances without a case in tests/kernel_ledger_clip.py: {missing}"
    assert not stale, f"ledger entries for kernels lib/obj_clip no longer has: {stale}"
    empty = [k for k, cs in kernel_ledger_clip.LEDGER.items() if not cs or not all(isinstance(c, kernel_ledger.Case) for c in cs)]
    assert not empty, empty


def test_no_kernel_name_is_in_another_directory_or_ledger(table):
    other_ledgers = set(kernel_ledger.LEDGER) | set(kernel_ledger_hb16.LEDGER) | set(kernel_ledger_lmk.LEDGER) | \
        set(kernel_ledger_det.LEDGER) | set(kernel_ledger_det16.LEDGER) | set(kernel_ledger_face.LEDGER) | set(kernel_ledger_nms.LEDGER)
    others = set(other_ledgers)
    for d in OTHER_DIRS:
        others |= set(kernel_resources.table(d))
    both = sorted(set(table) & others)
    assert not both, both
    assert not set(kernel_ledger_clip.LEDGER) & other_ledgers


def test_the_clip_kernels_use_no_scratch_and_no_lds(table):
    spills = {k: v["scratch"] for k, v in table.items() if v["scratch"]}
    assert not spills, spills
    assert all(v["static_lds"] == 0 for v in table.values()), table


def test_clip_object_is_free_of_the_op_sel_erratum(objects):
    assert objects
    for obj in objects:
        assert build.erratum_instructions(obj) == [], obj
