"""The bf16 precision of the SyncNet_color handle, host side (no GPU): the equal-contract model (tests/syncnet_bf16_model.py)
meets the bars the GPU test holds the engine to, so the contract passes without any kernel; the new symbols of the C ABI; the
refusal of an unknown precision before any device call; the build's view of the new source and header."""
import os
import re

import numpy as np
import pytest
import torch

import syncnet_bf16_bars as bars
import syncnet_bf16_model
import syncnet_ref
from calipsync_amd import _lib, build, recipe, syncnet
from conftest import REPO

CASES = bars.CASES


@pytest.fixture(scope="module")
def modelled():
    """the model on the fixtures' inputs: computed once, shared, never changed"""
    out = {}
    for mode, b in CASES.items():
        x, a = (torch.from_numpy(v) for v in recipe.make_syncnet_inputs(b, mode))
        out[mode] = syncnet_bf16_model.forward(syncnet.fold(recipe.make_syncnet_state_dict(mode), mode), x, a, mode)
    return out


def test_the_bar_file_belongs_to_the_fp32_fixtures():
    bar = bars.bars()
    for mode in CASES:
        assert float(bar[f"{mode}.fp32_vs_fixture"]) <= 1e-12
        for n in bars.NAMES:
            mx, mean = bar[f"{mode}.{n}"]
            assert 0 < mean < mx < 0.2, (mode, n)                    # bf16 noise on values of order 1, never exact
        assert float(bar[f"{mode}.cos_err"]) <= float(bar[f"{mode}.cos_bound"]) < 0.05
    assert len(bar.files) == 2 * (len(bars.NAMES) + 3)
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "syncnet_bf16_bar.npz")) < (1 << 20)


@pytest.mark.parametrize("mode", list(CASES))
def test_the_model_meets_the_bars_of_the_gpu_test(modelled, mode):
    a_emb, f_emb, stages = modelled[mode]
    fx, bar = bars.fixture(mode), bars.bars()
    rat = bars.ratios(mode, bars.errors(mode, a_emb.numpy(), f_emb.numpy(), {k: v.numpy() for k, v in stages.items()}, fx), bar)
    for n, (a, b) in rat.items():
        print(f"{mode} {n:9s} model / autocast: max {a:.3f} mean {b:.3f}")
    assert not bars.failures(rat), bars.failures(rat)
    cos = syncnet_ref.cosine(a_emb.double(), f_emb.double()).numpy()
    d = float(np.abs(cos - fx["cos64"]).max())
    print(f"{mode} cos: |model - fp64| {d:.3e}, 2 x bound {2 * float(bar[f'{mode}.cos_bound']):.3e}")
    assert d <= 2.0 * float(bar[f"{mode}.cos_bound"])


def test_the_model_rounds_where_the_contract_says(modelled):
    _, _, stages = modelled["hubert"]
    for name, t in stages.items():
        exact = bool(torch.equal(t.bfloat16().float(), t))
        assert exact == (name not in syncnet_bf16_model.LAST), name      # bf16 everywhere but the two fp32 stores
        assert float(t.min()) >= 0.0


def test_a_bad_precision_raises_before_any_device_call():
    packed = np.zeros(4, np.float32)
    for bad in ("fp16", "BF16", "", None, 1):
        with pytest.raises(ValueError, match="precision"):
            syncnet.SyncNetEngine(packed, "hubert", "cuda:0", bad)
        with pytest.raises(ValueError, match="precision"):
            syncnet.SyncNetColor("hubert", "cuda:0", None, bad)
    assert syncnet.check_precision("fp32") == 0 and syncnet.check_precision("bf16") == 1
    net = syncnet.SyncNetColor("hubert", "cuda:0", precision="bf16")
    assert net.precision == "bf16" and syncnet.SyncNetColor("wenet").precision == "fp32"
    build.build()
    lib = _lib.load()
    h = _lib.C.c_void_p()
    for bad in (-1, 2, 16):
        assert lib.casync_syncnet_create_ex(0, 0, bad, _lib.C.byref(h)) != 0 and not h.value
        assert b"precision" in lib.casync_last_error()
    assert lib.casync_syncnet_precision(None) == -1


def test_workspace_of_each_precision():
    build.build()
    lib = _lib.load()
    for mode in (0, 1):
        for b in (1, 3, 256, 4000):
            fp32 = lib.casync_sync_workspace_bytes(mode, b)
            assert lib.casync_syncnet_workspace_bytes_ex(mode, 0, b) == fp32
            bf16 = lib.casync_syncnet_workspace_bytes_ex(mode, 1, b)
            assert bf16 * 2 == fp32 and bf16 % 256 == 0
    assert lib.casync_syncnet_workspace_bytes_ex(0, 2, 1) == 0 and lib.casync_syncnet_workspace_bytes_ex(2, 1, 1) == 0
    assert lib.casync_syncnet_workspace_bytes_ex(0, 1, 0) == 0 and lib.casync_syncnet_workspace_bytes_ex(0, 1, 65537) == 0


def test_header_exports_and_library_agree_on_the_new_symbols():
    build.build()
    header = open(os.path.join(REPO, "include", "casync_hip.h")).read()
    declared = {n for n in re.findall(r"\b(casync_[a-z0-9_]+)\s*\(", header) if "_syncnet_" in n or "_sync16_" in n}
    want = {f"casync_syncnet_{n}" for n in ("create_ex", "precision", "workspace_bytes_ex")} | \
        {f"casync_op_sync16_{n}" for n in ("stem7", "conv5", "conv3", "conv1", "to_nchw")}
    assert declared == want == {n for n in _lib.EXPORTS if "_syncnet_" in n or "_sync16_" in n}
    lib = _lib.load()
    for n in want:
        assert hasattr(lib, n) and getattr(lib, n).argtypes is not None, n
    assert _lib.ABI_VERSION == 13 == lib.casync_abi_version() and "#define CASYNC_ABI_VERSION 13" in header
    assert "SyncNet_color, bf16 precision (additive to ABI 13)" in header


def test_the_build_sees_the_new_source_and_header():
    assert build.SOURCES_SYNC16 == ["syncnet_bf16.hip"] and "syncnet_bf16.hip" in build.SOURCES
    assert "syncnet_common.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "syncnet_common.h"))
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    whole = build.source_hash()
    for attr, drop in (("SOURCES", "syncnet_bf16.hip"), ("HEADERS", "syncnet_common.h")):
        kept = getattr(build, attr)
        try:
            setattr(build, attr, [s for s in kept if s != drop])
            assert build.source_hash() != whole, drop
        finally:
            setattr(build, attr, kept)
