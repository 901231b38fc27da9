"""The ledger rule for the sixteenth object directory, calipsync_amd/lib/obj_train/ (no GPU): every kernel compiled from
csrc/train_ops.hip has a case in tests/kernel_ledger_train.py and the other way round, no kernel name occurs in another object
directory or another ledger, the kernels use no scratch and no LDS (the source declares none), the source holds no inline
assembly and switches contraction off, and the build's op_sel check stays clean on the object."""
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
import kernel_ledger_sync  # noqa: E402
import kernel_ledger_sync16  # noqa: E402
import kernel_ledger_train  # noqa: E402
from calipsync_amd import build  # noqa: E402

pytestmark = pytest.mark.skipif(not kernel_resources.tools_available(), reason="llvm binutils of the ROCm image not found")

OTHER_DIRS = (build.OBJ_DIR, build.OBJ_DIR_HB16, build.OBJ_DIR_LMK, build.OBJ_DIR_DET, build.OBJ_DIR_DET16, build.OBJ_DIR_FACE,
              build.OBJ_DIR_NMS, build.OBJ_DIR_CLIP, build.OBJ_DIR_JPEG, build.OBJ_DIR_JPEG420, build.OBJ_DIR_JPEGDEC, build.OBJ_DIR_SYNC,
              build.OBJ_DIR_SYNC16, build.OBJ_DIR_AUDIO, build.OBJ_DIR_MJPEGDEC)
OTHER_LEDGERS = (kernel_ledger, kernel_ledger_hb16, kernel_ledger_lmk, kernel_ledger_det, kernel_ledger_det16, kernel_ledger_face,
                 kernel_ledger_nms, kernel_ledger_clip, kernel_ledger_jpeg, kernel_ledger_jpeg420, kernel_ledger_jpegdec, kernel_ledger_sync,
                 kernel_ledger_sync16, kernel_ledger_audio, kernel_ledger_mjpegdec)
KERNELS = ["train_batch_kernel<false>", "train_batch_kernel<true>"]


@pytest.fixture(scope="module")
def objects():
    build.build()                      # no-op when the library is up to date
    d = build.OBJ_DIR_TRAIN
    if not os.path.isdir(d) or not any(f.endswith(".o") for f in os.listdir(d)):
        build.build(force=True)        # a library shipped without its objects: compile them
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".o")]


@pytest.fixture(scope="module")
def table(objects):
    return kernel_resources.table(build.OBJ_DIR_TRAIN)


def test_the_train_object_is_in_its_own_directory(objects):
    assert [os.path.basename(o) for o in objects] == ["train_ops.o"]
    assert build.SOURCES_TRAIN == ["train_ops.hip"] and "train_ops.hip" in build.SOURCES
    assert build.OBJ_DIR_TRAIN == os.path.join(build.LIB_DIR, "obj_train")
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    assert len({build.OBJ_DIR_TRAIN, *OTHER_DIRS}) == 16
    for d in OTHER_DIRS:
        assert not os.path.exists(os.path.join(d, "train_ops.o")), d
    assert sorted(f for f in os.listdir(build.OBJ_DIR_MJPEGDEC) if f.endswith(".o")) == ["jpeg_dec_mjpeg.o"]


def test_source_hash_covers_the_source_and_both_new_headers(objects):
    """source_hash() changes without the source, without the shared resize header and without the entry's header"""
    full = build.source_hash()
    train_h = os.path.join("..", "..", "include", "casync_train.h")
    assert "resize_u8.h" in build.HEADERS and train_h in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "resize_u8.h")) and os.path.exists(os.path.join(build.CSRC, train_h))
    sources, headers = build.SOURCES, build.HEADERS
    try:
        build.SOURCES = [s for s in sources if s not in build.SOURCES_TRAIN]
        assert build.source_hash() != full
        build.SOURCES = sources
        for drop in ("resize_u8.h", train_h):
            build.HEADERS = [h for h in headers if h != drop]
            assert build.source_hash() != full, drop
    finally:
        build.SOURCES, build.HEADERS = sources, headers
    assert build.source_hash() == full


def test_is_stale_sees_the_train_source_and_headers(objects, monkeypatch):
    """is_stale() walks SOURCES and HEADERS: any of the three files newer than the library makes it stale"""
    assert not build.is_stale()
    lib_time = os.path.getmtime(build.LIB_PATH)
    real = os.path.getmtime
    for name in ("train_ops.hip", "resize_u8.h", os.path.join("..", "..", "include", "casync_train.h")):
        path = os.path.abspath(os.path.join(build.CSRC, name))
        monkeypatch.setattr(os.path, "getmtime", lambda p, path=path: lib_time + 10 if os.path.abspath(p) == path else real(p))
        assert build.is_stale(), name
        monkeypatch.setattr(os.path, "getmtime", real)


def test_the_resize_arithmetic_has_one_copy():
    """Tap, linear_tap_x / _y, coef and resize_u8_at are defined in csrc/resize_u8.h alone; both users include it"""
    defined = re.compile(r"^(?:struct Tap\b|__device__ __forceinline__ \w[\w ]* (?:linear_tap_x|linear_tap_y|coef|resize_u8_at)\()", re.M)
    for name in os.listdir(build.CSRC):
        text = open(os.path.join(build.CSRC, name)).read()
        assert len(defined.findall(text)) == (5 if name == "resize_u8.h" else 0), name
    for user in ("frame_ops.hip", "train_ops.hip"):
        assert '#include "resize_u8.h"' in open(os.path.join(build.CSRC, user)).read(), user


def test_every_train_kernel_has_a_ledger_case(table):
    assert sorted(table) == KERNELS, sorted(table)
    missing = sorted(set(table) - set(kernel_ledger_train.LEDGER))
    stale = sorted(set(kernel_ledger_train.LEDGER) - set(table))
    assert not missing, f"kernel instances without a case in tests/kernel_ledger_train.py: {missing}"
    assert not stale, f"ledger entries for kernels lib/obj_train no longer has: {stale}"
    empty = [k for k, cs in kernel_ledger_train.LEDGER.items() if not cs or not all(isinstance(c, kernel_ledger.Case) for c in cs)]
    assert not empty, empty
    listed = {c for cs in kernel_ledger_train.LEDGER.values() for c in cs}
    assert listed == {c for _, _, c in kernel_ledger_train.cases()}              # every case is one GPU test
    assert all(len(kernel_ledger_train.launched_by(c)) == 1 for c in listed)      # the entry launches one instance per call


def test_no_kernel_name_is_in_another_directory_or_ledger(table):
    other_ledgers = set()
    for ledger in OTHER_LEDGERS:
        other_ledgers |= set(ledger.LEDGER)
    others = set(other_ledgers)
    for d in OTHER_DIRS:
        others |= set(kernel_resources.table(d))
    both = sorted(set(table) & others)
    assert not both, both
    assert not set(kernel_ledger_train.LEDGER) & other_ledgers


def test_the_train_kernels_use_no_scratch_and_no_lds(table):
    spills = {k: v["scratch"] for k, v in table.items() if v["scratch"]}
    assert not spills, spills
    src = open(os.path.join(build.CSRC, "train_ops.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert "__shared__" not in code and "__shared__" not in re.sub(r"//.*", "", open(os.path.join(build.CSRC, "resize_u8.h")).read())
    for k, v in table.items():
        assert v["static_lds"] == 0, (k, v)
    assert "asm" not in code                                 # no inline assembly
    assert "#pragma clang fp contract(off)" in code
    const = {k: int(v) for k, v in re.findall(r"constexpr int (\w+) = (\d+);", src)}
    assert const["RECORDS_PER_LAUNCH"] == kernel_ledger_train.RECORDS_PER_LAUNCH and const["REC_WORDS"] == 12
    assert const["RECORDS_PER_LAUNCH"] * const["REC_WORDS"] * 4 + 64 <= 4096       # the record block travels as kernel arguments


def test_train_object_is_free_of_the_op_sel_erratum(objects):
    assert objects
    for obj in objects:
        assert build.erratum_instructions(obj) == [], obj
