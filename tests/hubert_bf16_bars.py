"""Bars of the bf16 HuBERT engine (helper module, no tests): tests/golden/hubert_bf16_bar.npz holds how far the reference's
own extract_features moves under torch.autocast("cpu", torch.bfloat16), measured by tests/golden/make_hubert_bf16_bar.py
against its fp32 run.  The engine -- and the CPU model of its contract -- are held to the fp32 fixtures with

    mean-type statistics (mean |d|, mean per-token relative L2)  <= 1.0  x the reference-autocast figure
    max-type statistics  (max |d|, max per-token relative L2)    <= 1.25 x the reference-autocast figure

always ON THE SAME POSITIONS the fp32 fixture samples.  Why these factors: the contract keeps more in fp32 than autocast
does (residual stream, LayerNorm inputs, softmax statistics), so an engine above the reference's own MEAN bf16 error has
an unplanned rounding or a bug; a maximum over 1e5-1e6 rounding errors is an extreme-value statistic that moves with the
summation order, and 25 % is the margin the project gives its other bf16 bars.
"""
import os

import numpy as np

MEAN_X, MAX_X = 1.0, 1.25
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load():
    return np.load(os.path.join(GOLDEN, "hubert_bf16_bar.npz"))


def mm(a, b):
    """[max |d|, mean |d|]"""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return np.array([d.max(), d.mean()])


def four(a, b):
    """[max |d|, mean |d|, per-token ||d|| / ||ref|| max, mean] of [T, 1024] arrays (b is the reference)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    rel = np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
    return np.concatenate([mm(a, b), [rel.max(), rel.mean()]])


def hold(what, got, ref):
    """Print `got` beside the reference-autocast figures `ref` and return the statistics above their bar (as text)."""
    names = ["max|d|", "mean|d|", "rel-L2 max", "rel-L2 mean"][:len(got)]
    factors = [MAX_X, MEAN_X, MAX_X, MEAN_X][:len(got)]
    print(f"{what}: " + "  ".join(f"{n} {g:.3e} ({g / r:.2f} x autocast {r:.3e}, bar {f:.2f} x)" for n, g, r, f in zip(names, got, ref, factors)))
    return [f"{what}: {n} {g:.3e} above {f} x {r:.3e}" for n, g, r, f in zip(names, got, ref, factors) if not g <= f * r]


def check_case(case, bar, g, flat, conv, l0):
    """Failures of one fixture case: flat [T,1024] chunked features, conv / l0 the flattened taps of chunk 0 (or None)."""
    bad = []
    if case == "l2":
        bad += hold("l2 output", four(flat, g["out"].reshape(-1, 1024)), bar["l2_out"])
    else:
        bad += hold("l24 rows", four(flat[g["rows"]], g["row_val"]), bar["l24_rows"])
        bad += hold("l24 strided", mm(flat.reshape(-1)[g["idx"]], g["val"]), bar["l24_idx"])
    if conv is not None:
        bad += hold(f"{case} conv tap", mm(conv[g["conv_idx"]], g["conv_val"]), bar[f"{case}_conv_idx"])
    if l0 is not None:
        bad += hold(f"{case} layer-0 input tap", mm(l0[g["l0_idx"]], g["l0_val"]), bar[f"{case}_l0_idx"])
    return bad


def check_rows(what, got, ref, bar):
    """Behaviour cases on the 2-layer recipe model: every batch row [T,1024] against the fp32 restatement, held to the
    2-layer case's whole-output autocast figures (same model, the same kind of waveform; there is no autocast run per case)."""
    bad = []
    for i in range(got.shape[0]):
        bad += hold(f"{what} row {i}", four(got[i], ref[i]), bar["l2_out"])
    return bad
