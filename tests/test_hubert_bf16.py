"""bf16 HuBERT, the checks that need no GPU: the reference-autocast bar file against the fp32 fixtures, the CPU model of
the numerics contract against those bars (it pins the contract: the rounding points of DESIGN section 8b meet the bars in
plain fp32-sum arithmetic), and the argument checks that must fail before any device call."""
import os

import numpy as np
import pytest
import torch

import hubert_bf16_bars as bars
import hubert_bf16_model
import hubert_ref
from calipsync_amd import hubert

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"l2": ("hubert_l2.npz", 2), "l24": ("hubert_l24.npz", 24)}


def test_bar_file_belongs_to_the_fp32_fixtures():
    bar = bars.load()
    for case, (fixture, _) in CASES.items():
        g = np.load(os.path.join(GOLDEN, fixture))
        assert str(bar[f"{case}_wave_sha256"]) == str(g["wave_sha256"])
        # the fp32 run beside the autocast run reproduced the fixture's values (same call, same weights) up to the fp32
        # summation order of another thread count: three orders below the bf16 figures
        assert float(bar[f"{case}_fp32_vs_fixture"]) <= 1e-5
        for key in ("out", "conv", "l0", "conv_idx", "l0_idx"):
            v = bar[f"{case}_{key}"]
            assert np.all(np.isfinite(v)) and np.all(v > 0) and v[0] >= v[1]
    # the reference's own bf16 error (whole output): 24 layers max 1.23e-1 mean 1.04e-2 per-token 1.91e-2 / 1.32e-2,
    # 2 layers 7.5e-2 / 1.13e-2 / 1.83e-2 / 1.41e-2 (the figures DESIGN quotes)
    assert np.allclose(bar["l24_out"], [1.23e-1, 1.04e-2, 1.91e-2, 1.32e-2], rtol=0.02)
    assert np.allclose(bar["l2_out"], [7.5e-2, 1.13e-2, 1.83e-2, 1.41e-2], rtol=0.02)
    assert set(f for f in bar.files if f.startswith("l24_")) >= {"l24_rows", "l24_idx"}


@pytest.mark.parametrize("case", ["l2", "l24"])
def test_cpu_model_of_the_contract_meets_the_bars(case):
    fixture, layers = CASES[case]
    g = np.load(os.path.join(GOLDEN, fixture))
    bar = bars.load()
    P = hubert.packed_tensors(hubert_ref.recipe_state_dict(layers), layers)
    x = torch.from_numpy(hubert.normalize(hubert_ref.golden_wave(int(g["samples"]), int(g["seed"]))))[None]
    first = {}

    def enc(chunks):
        out = []
        for c in chunks:
            taps = {}
            out.append(hubert_bf16_model.forward(P, layers, c, taps)[0])
            if not first:
                first.update(conv=taps["conv"][0].numpy().reshape(-1), l0=taps["layer0_in"][0].numpy().reshape(-1))
        return out
    with torch.no_grad():
        flat = hubert.chunked_features(x, enc).numpy().reshape(-1, 1024)
    bad = bars.check_case(case, bar, g, flat, first["conv"], first["l0"])
    assert not bad, bad


@pytest.mark.parametrize("n", [400, 401, 720, 2000])
def test_cpu_model_meets_the_bars_on_short_waveforms(n):
    P = hubert.packed_tensors(hubert_ref.recipe_state_dict(2), 2)
    w = torch.stack([torch.from_numpy(hubert.normalize(hubert_ref.golden_wave(n, s))) for s in (21, 22)])
    with torch.no_grad():
        ref, got = hubert_ref.forward(P, 2, w), hubert_bf16_model.forward(P, 2, w)
    bad = bars.check_rows(f"n={n}", got.numpy(), ref.numpy(), bars.load())
    assert not bad, bad


def test_unknown_precision_is_refused_before_any_device_call(tmp_path):
    assert hubert.check_precision("fp32") == 0 and hubert.check_precision("bf16") == 1
    with pytest.raises(ValueError, match="fp16"):
        hubert.HubertEngine({}, 2, "cuda:0", precision="fp16")          # (an empty state dict: never reached)
    with pytest.raises(ValueError, match="fp16"):
        hubert.HubertExtractor(str(tmp_path / "nowhere"), "cuda:0", precision="fp16")
    from calipsync_amd.frame_synth import VideoStreamManager
    with pytest.raises(ValueError, match="fp16"):
        VideoStreamManager(str(tmp_path / "nodata"), None, hubert_path=str(tmp_path / "nowhere"), hubert_precision="fp16")


def test_create_ex_checks_its_arguments_without_a_gpu():
    import ctypes
    from calipsync_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.casync_hubert_create_ex(0, 2, 7, ctypes.byref(h)) < 0 and b"dtype" in lib.casync_last_error()
    assert not h.value
    assert lib.casync_hubert_workspace_bytes_h(None, 1, 16000) == 0
    if not torch.cuda.is_available():
        assert lib.casync_hubert_create_ex(0, 2, 1, ctypes.byref(h)) < 0 and b"device" in lib.casync_last_error()
