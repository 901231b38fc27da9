"""The ledger rule for the fourteenth object directory, calipsync_amd/lib/obj_audio/ (no GPU): every kernel compiled from
csrc/audio.hip has a case in tests/kernel_ledger_audio.py and the other way round, no kernel name occurs in another object
directory or another ledger, the kernels use no scratch and no more LDS than the source declares (the resample kernel's input
tile, the moments kernels' float64 tree), and the build's op_sel check stays clean on the object."""
import re
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
import kernel_ledger_nms  # noqa: E402
import kernel_ledger_sync  # noqa: E402
import kernel_ledger_sync16  # noqa: E402
from calipsync_amd import build  # noqa: E402

pytestmark = pytest.mark.skipif(not kernel_resources.tools_available(), reason="llvm binutils of the ROCm image not found")

OTHER_DIRS = (build.OBJ_DIR, build.OBJ_DIR_HB16, build.OBJ_DIR_LMK, build.OBJ_DIR_DET, build.OBJ_DIR_DET16, build.OBJ_DIR_FACE,
              build.OBJ_DIR_NMS, build.OBJ_DIR_CLIP, build.OBJ_DIR_JPEG, build.OBJ_DIR_JPEG420, build.OBJ_DIR_JPEGDEC, build.OBJ_DIR_SYNC, build.OBJ_DIR_SYNC16)
OTHER_LEDGERS = (kernel_ledger, kernel_ledger_hb16, kernel_ledger_lmk, kernel_ledger_det, kernel_ledger_det16, kernel_ledger_face,
                 kernel_ledger_nms, kernel_ledger_clip, kernel_ledger_jpeg, kernel_ledger_jpeg420, kernel_ledger_jpegdec, kernel_ledger_sync, kernel_ledger_sync16)
KERNELS = [f"wav_convert_kernel<{w}>" for w in (1, 2, 3, 4)] + ["wav_moments_final_kernel", "wav_moments_kernel", "wav_normalize_kernel"] + \
          [f"wav_resample_kernel<{w}>" for w in (1, 2, 3, 4)]


@pytest.fixture(scope="module")
def objects():
    build.build()                      # no-op when the library is up to date
    d = build.OBJ_DIR_AUDIO
    if not os.path.isdir(d) or not any(f.endswith(".o") for f in os.listdir(d)):
        build.build(force=True)        # a library shipped without its objects: compile them
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".o")]


@pytest.fixture(scope="module")
def table(objects):
    return kernel_resources.table(build.OBJ_DIR_AUDIO)


def test_the_audio_object_is_in_its_own_directory(objects):
    assert [os.path.basename(o) for o in objects] == ["audio.o"]
    assert build.SOURCES_AUDIO == ["audio.hip"] and "audio.hip" in build.SOURCES
    assert build.OBJ_DIR_AUDIO == os.path.join(build.LIB_DIR, "obj_audio")
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    assert len({build.OBJ_DIR_AUDIO, *OTHER_DIRS}) == 14
    for d in OTHER_DIRS:
        assert not os.path.exists(os.path.join(d, "audio.o")), d
    assert sorted(f for f in os.listdir(build.OBJ_DIR_SYNC16) if f.endswith(".o")) == ["syncnet_bf16.o"]
    # source_hash() covers the new source: without it the hash is another one
    with_audio = build.source_hash()
    sources = build.SOURCES
    try:
        build.SOURCES = [s for s in sources if s not in build.SOURCES_AUDIO]
        assert build.source_hash() != with_audio
    finally:
        build.SOURCES = sources


def test_is_stale_sees_the_audio_source(objects, monkeypatch):
    """is_stale() walks SOURCES: the file newer than the library makes it stale"""
    assert not build.is_stale()
    src = os.path.join(build.CSRC, "audio.hip")
    lib_time = os.path.getmtime(build.LIB_PATH)
    real = os.path.getmtime
    monkeypatch.setattr(os.path, "getmtime", lambda p: lib_time + 10 if os.path.abspath(p) == src else real(p))
    assert build.is_stale()


def test_every_audio_kernel_has_a_ledger_case(table):
    assert sorted(table) == KERNELS, sorted(table)
    missing = sorted(set(table) - set(kernel_ledger_audio.LEDGER))
    stale = sorted(set(kernel_ledger_audio.LEDGER) - set(table))
    assert not missing, f"kernel instances without a case in tests/kernel_ledger_audio.py: {missing}"
    assert not stale, f"ledger entries for kernels lib/obj_audio no longer has: {stale}"
    empty = [k for k, cs in kernel_ledger_audio.LEDGER.items() if not cs or not all(isinstance(c, kernel_ledger.Case) for c in cs)]
    assert not empty, empty
    listed = {c for cs in kernel_ledger_audio.LEDGER.values() for c in cs}
    assert listed == {c for _, _, c in kernel_ledger_audio.cases()}              # every case is one GPU test


def test_no_kernel_name_is_in_another_directory_or_ledger(table):
    other_ledgers = set()
    for ledger in OTHER_LEDGERS:
        other_ledgers |= set(ledger.LEDGER)
    others = set(other_ledgers)
    for d in OTHER_DIRS:
        others |= set(kernel_resources.table(d))
    both = sorted(set(table) & others)
    assert not both, both
    assert not set(kernel_ledger_audio.LEDGER) & other_ledgers


def test_the_audio_kernels_use_no_scratch_and_the_lds_the_source_declares(table):
    spills = {k: v["scratch"] for k, v in table.items() if v["scratch"]}
    assert not spills, spills
    src = open(os.path.join(build.CSRC, "audio.hip")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int (\w+) = (\d+);", src)}
    assert const["OUT_PER_WG"] == kernel_ledger_audio.OUT_PER_WG and const["CONVERT_PER_WG"] == kernel_ledger_audio.CONVERT_PER_WG
    assert const["MOMENT_MIN_SPAN"] == kernel_ledger_audio.MOMENT_SPAN
    assert re.findall(r"__shared__ (\w+) \w+\[(\w+)\];", src) == [("float", "TILE_IN"), ("double", "THREADS"), ("double", "THREADS")]
    tile, tree = 4 * const["TILE_IN"], 8 * const["THREADS"]
    assert tile <= 32768
    for k, v in table.items():
        want = tile if k.startswith("wav_resample_kernel") else tree if k.startswith("wav_moments") else 0
        assert v["static_lds"] <= want, (k, v)
    assert "asm" not in re.sub(r"//.*", "", src)             # no inline assembly


def test_audio_object_is_free_of_the_op_sel_erratum(objects):
    assert objects
    for obj in objects:
        assert build.erratum_instructions(obj) == [], obj
