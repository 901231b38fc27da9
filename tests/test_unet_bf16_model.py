"""tests/unet_bf16_model.py checked on the CPU: the segments compose to the oracle's forward in both arithmetics, every flag
moves the segments it names and no other, and the full bf16 model on the golden inputs sits within the figures the reference
itself reaches under bf16 autocast (tests/golden/unet_bf16_bar.npz, made by tests/golden/make_unet_bf16_bar.py)."""
import functools
import os

import numpy as np
import pytest
import torch

import unet_bf16_model as um
import wenet_ref
from calipsync_amd import recipe
from conftest import GOLDEN, sample_indices
from oracle import unet_oracle
from test_facedet_bf16_gpu import MAX_BAR, MEAN_BAR        # the factors every bf16 engine here is held to; no new one

TOL = 1e-5                        # tests/test_oracle.py's acceptance, relative to max(1, max|ref|)
TAPS = [n for n, _ in um.SEGMENTS]


@functools.lru_cache(maxsize=None)
def _sd(mode="hubert"):
    return recipe.make_state_dict(mode=mode)


@functools.lru_cache(maxsize=None)
def _inputs(mode="hubert"):
    x, a = recipe.make_inputs(2, mode=mode)
    return torch.from_numpy(x), torch.from_numpy(a)


@functools.lru_cache(maxsize=None)
def _oracle(mode, dtype):
    sd = unet_oracle.to_torch(_sd(mode), dtype)
    x, a = _inputs(mode)
    taps = {}
    taps["out"] = (wenet_ref if mode == "wenet" else unet_oracle).forward(sd, x.to(dtype), a.to(dtype), taps)
    return taps


@functools.lru_cache(maxsize=None)
def _model_taps(mode="hubert"):
    """the full bf16 model (default flags: the single-lane plan from 12 frames per launch) on the golden inputs"""
    m = um.Contract(_sd(mode), mode)
    return um.compose(m.segment, *_inputs(mode))


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max()) / max(1.0, float(ref.abs().max()))


def test_identity_rounding_composes_to_the_oracle():
    """No rounding, fp32 folded weights: the segments composed against unet_oracle.forward in fp32 on recipe.make_inputs(2).  Bit
    equality is impossible -- the model multiplies by BatchNorm-folded weights (pack.fold: folded in float64, rounded once) and
    by the host-composed query projection where the oracle applies conv and BatchNorm one after the other -- so every tap is
    held to the <= 1e-5 of tests/test_oracle.py, relative to max(1, max|ref|)."""
    m = um.Contract(_sd(), rounding=False)
    got, ref = um.compose(m.segment, *_inputs()), _oracle("hubert", torch.float32)
    worst = {n: _rel(got[n], ref[n]) for n in TAPS if n in ref}
    print({k: f"{v:.1e}" for k, v in worst.items()})
    assert set(TAPS) - set(ref) == {"audio_conv1"}            # (the oracle's forward records no tap behind conv1)
    assert max(worst.values()) <= TOL, worst


@pytest.mark.parametrize("mode", ["hubert", "wenet"])
def test_float64_segments_compose_to_the_oracle_in_float64(mode):
    """the same oracle functions in the same order: equal bit for bit, every tap"""
    sd64 = um.to64(_sd(mode))
    got = um.compose(lambda name, *src: um.reference(sd64, name, *src, mode=mode), *_inputs(mode))
    ref = _oracle(mode, torch.float64)
    for n in TAPS:
        assert got[n].dtype == torch.float64
        if n in ref:
            assert torch.equal(got[n], ref[n]), n
    if mode == "wenet":      # tests/wenet_ref.py's audio encoder tap by tap (its forward records audio_conv1 too)
        assert {"audio_conv1", "audio_conv2", "audio_conv3", "audio_conv4", "audio_conv5"} <= set(ref)


def test_rounded_model_really_rounds_and_its_taps_are_bf16_exact():
    t = _model_taps()
    for n in TAPS[:-1]:
        assert torch.equal(t[n], um.bf16(t[n])), n
    assert not torch.equal(t["out"], um.bf16(t["out"]))        # the boundary is fp32
    ref = _oracle("hubert", torch.float64)
    assert float((t["out"].double() - ref["out"]).abs().max()) > 1e-4


@pytest.mark.parametrize("flag,other", [("commute_up", ()), ("commute_up", ("up1",)), ("p_bf16", False), ("dw_taps_bf16", 0),
                                        ("dw_taps_bf16", 2)])
def test_a_flag_changes_the_bits_of_its_segments_and_of_no_other(flag, other):
    """every segment from the SAME start tensors (the default model's taps) under the default flags and with one flag changed"""
    m, t = um.Contract(_sd()), dict(_model_taps())
    t["x"], t["audio"] = _inputs()
    moved = []
    for name, srcs in um.SEGMENTS:
        src = [t[k][:1] for k in srcs]
        if not torch.equal(m.segment(name, *src), m.segment(name, *src, **{flag: other})):
            moved.append(name)
    want = set(um.FLAG_SEGMENTS[flag])
    if flag == "commute_up" and other == ("up1",):
        want = {"u2"}                                          # only up2 leaves the commuted route
    if flag == "dw_taps_bf16" and other == 2:
        want = {"u4"}                                          # 1 -> 2 adds up4.0's taps, nothing else
    assert set(moved) == want, (flag, other, moved)


def test_full_model_on_the_golden_inputs_within_the_references_autocast_figures(mode="hubert"):
    """|model - float64| per tap against the reference's own |autocast - float64| (unet_bf16_bar.npz), in the form the engine is
    held to on the GPU: max <= 2 x, mean <= 1.25 x.  The fixture is tied to the fp32 golden and to the float64 used here."""
    bar = np.load(os.path.join(GOLDEN, "unet_bf16_bar.npz"))
    assert float(bar[f"{mode}.fp32_vs_fixture"]) <= TOL and float(bar[f"{mode}.f64_vs_oracle"]) <= 1e-12
    t, ref = _model_taps(mode), _oracle(mode, torch.float64)
    bad = {}
    for n in TAPS:
        if n not in ref:
            continue
        d = (t[n].double() - ref[n]).abs()
        mx, mean = float(d.max()), float(d.mean())
        amx, amean = bar[f"{mode}.{n}"]
        print(f"{mode} {n:12s} max {mx:.3e} = {mx / amx:.3f} x autocast, mean {mean:.3e} = {mean / amean:.3f} x autocast")
        if not mx <= MAX_BAR * amx or not mean <= MEAN_BAR * amean:
            bad[n] = (round(mx / amx, 3), round(mean / amean, 3))
    assert not bad, bad


def test_fixture_is_tied_to_the_fp32_golden(golden):
    """the oracle in fp32 (which the fixture's float64 equals to 1e-12 in float64) meets the stored fp32 golden at its sample positions"""
    ref = _oracle("hubert", torch.float32)
    for n in ("x1", "kx", "u4"):
        flat = ref[n].numpy().reshape(-1)
        got = flat[sample_indices(flat.size)]
        assert np.abs(got - golden[f"{n}.samples"]).max() <= TOL * max(1.0, float(np.abs(golden[f"{n}.samples"]).max())), n


def test_the_gpu_modules_kernel_names_are_kernels_of_the_built_library():
    """tests/test_model_bf16_contract_gpu.py asserts its plans from the launch log by name: every exact name it asks for (or
    forbids) is a key of tools/kernel_resources.table(), every family a prefix of some key"""
    import gpu_util
    import test_model_bf16_contract_gpu as g
    table = gpu_util.kernel_table()
    if not table:
        pytest.skip("llvm binutils of the ROCm image, or the built objects, not found")
    names = {k for spec in g.PLANS.values() for k in spec["ran"] + spec["not_ran"]} | {g.RECT, g.RING}
    for k in names:
        assert any(n.startswith(k) for n in table) if k in g.FAMILIES else k in table, k
