"""Generate the bar of the bf16 HuBERT engine from the REFERENCE itself: how far the reference's own
``HubertExtractor.extract_features`` moves when it runs under ``torch.autocast("cpu", dtype=torch.bfloat16)``
(build container only; the reference is reached exactly as in make_hubert_golden.py, hooks included).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_hubert_bf16_bar.py
        -> tests/golden/hubert_bf16_bar.npz

Per case (``l2``: 2 layers, 48,000 samples; ``l24``: 24 layers, 328,000 samples -- the waveforms of hubert_l2.npz and
hubert_l24.npz) the file holds the error of the autocast run against the fp32 run of the same call:

    <case>_out        [max |d|, mean |d|, per-token ||d|| / ||ref|| max, mean] over the whole output
    <case>_rows       the same four over the fixture's ``rows``                      (l24 only)
    <case>_idx        [max |d|, mean |d|] over the fixture's strided samples ``idx``  (l24 only)
    <case>_conv       [max, mean] over the whole conv-stack tap of chunk 0, <case>_conv_idx over the fixture's ``conv_idx``
    <case>_l0         ... and over the layer-0-input tap, <case>_l0_idx over ``l0_idx``
    <case>_fp32_vs_fixture   max |fp32 run here - value stored in the fp32 fixture| over every sampled position
    <case>_wave_sha256       digest of the waveform (equal to the fp32 fixture's)

Only statistics and digests are written.  tests/test_hubert_bf16.py checks the file against the fp32 fixtures;
tests/test_hubert_bf16_gpu.py takes the engine's bars from it (1.0 x the mean-type, 1.25 x the max-type figures, on the same
positions).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_hubert_golden as mg  # noqa: E402
import hubert_ref  # noqa: E402  (make_hubert_golden put tests/ on the path)


def mm(a, b):
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return np.array([d.max(), d.mean()])


def four(a, b):
    """[max |d|, mean |d|, per-token relative L2 max, mean] of [T, 1024] arrays"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    rel = np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
    return np.concatenate([mm(a, b), [rel.max(), rel.mean()]])


def main():
    torch.set_num_threads(16)   # fixed: the bf16 GEMMs of the autocast run sum in an order that depends on the thread count
    cls = mg.reference_extractor_class()
    res = {}
    for case, layers, n, seed, fixture in (("l2", 2, mg.L2_SAMPLES, mg.L2_SEED, "hubert_l2.npz"),
                                           ("l24", 24, mg.L24_SAMPLES, mg.L24_SEED, "hubert_l24.npz")):
        g = np.load(os.path.join(HERE, fixture))
        model = mg.make_model(layers)
        rec = mg.hooks(model)
        ex = mg.extractor(cls, model)
        wave = hubert_ref.golden_wave(n, seed)
        f32 = ex.extract_features(wave).numpy().reshape(-1, 1024)
        n_calls = len(rec["conv"])
        with torch.autocast("cpu", dtype=torch.bfloat16):
            b16 = ex.extract_features(wave).float().numpy().reshape(-1, 1024)
        conv32, l032 = rec["conv"][0].float().numpy().reshape(-1), rec["layer0_in"][0].float().numpy().reshape(-1)
        conv16, l016 = rec["conv"][n_calls].float().numpy().reshape(-1), rec["layer0_in"][n_calls].float().numpy().reshape(-1)
        res[f"{case}_wave_sha256"] = mg.sha(wave)
        res[f"{case}_out"] = four(b16, f32)
        res[f"{case}_conv"], res[f"{case}_l0"] = mm(conv16, conv32), mm(l016, l032)
        res[f"{case}_conv_idx"] = mm(conv16[g["conv_idx"]], conv32[g["conv_idx"]])
        res[f"{case}_l0_idx"] = mm(l016[g["l0_idx"]], l032[g["l0_idx"]])
        fix = [np.abs(conv32[g["conv_idx"]] - g["conv_val"]).max(), np.abs(l032[g["l0_idx"]] - g["l0_val"]).max()]
        if "rows" in g.files:
            res[f"{case}_rows"] = four(b16[g["rows"]], f32[g["rows"]])
            res[f"{case}_idx"] = mm(b16.reshape(-1)[g["idx"]], f32.reshape(-1)[g["idx"]])
            fix += [np.abs(f32[g["rows"]] - g["row_val"]).max(), np.abs(f32.reshape(-1)[g["idx"]] - g["val"]).max()]
        else:
            fix.append(np.abs(f32 - g["out"].reshape(-1, 1024)).max())
        res[f"{case}_fp32_vs_fixture"] = np.float64(max(fix))
        print(case, {k: np.asarray(v).round(5).tolist() for k, v in res.items() if k.startswith(case) and not k.endswith("sha256")},
              flush=True)
    np.savez_compressed(os.path.join(HERE, "hubert_bf16_bar.npz"), **res)
    assert not mg._Untouched.touched, f"the reference entered soundfile: {mg._Untouched.touched}"


if __name__ == "__main__":
    main()
