"""The bars of the bf16 SyncNet_color handle, shared by the CPU test of the equal-contract model and the GPU test of the engine:
tests/golden/syncnet_bf16_bar.npz holds the reference's own bf16-autocast error against its float64 run, per stage [max, mean]
at the 4096 sample positions of tests/golden/syncnet_<mode>_b<B>.npz and for both embeddings in full.  A stage passes within
BAR_MAX x autocast's max and BAR_MEAN x its mean -- the project's bars for the bf16 S3FD and the bf16 U-Net."""
import os

import numpy as np

from calipsync_amd import syncnet
from conftest import GOLDEN, sample_indices

CASES = {"hubert": 3, "wenet": 2}
BAR_MAX, BAR_MEAN = 2.0, 1.25
NAMES = tuple(syncnet.STAGES) + ("audio_emb", "face_emb")


def fixture(mode):
    return np.load(os.path.join(GOLDEN, f"syncnet_{mode}_b{CASES[mode]}.npz"))


def bars():
    return np.load(os.path.join(GOLDEN, "syncnet_bf16_bar.npz"))


def errors(mode, a_emb, f_emb, taps, fx):
    """{name: (max, mean) of |x - float64|}: the taps (name -> [B,C,H,W] array-like, float) at the fixture's sample positions,
    the embeddings in full"""
    out = {}
    for name in syncnet.STAGES:
        flat = np.asarray(taps[name], dtype=np.float64).reshape(-1)
        assert tuple(np.asarray(taps[name]).shape) == tuple(fx[f"{name}.shape"]), name
        d = np.abs(flat[sample_indices(flat.size)] - fx[f"{name}.samples"])
        out[name] = (float(d.max()), float(d.mean()))
    for name, e in (("audio_emb", a_emb), ("face_emb", f_emb)):
        d = np.abs(np.asarray(e, dtype=np.float64) - fx[f"{name}64"])
        out[name] = (float(d.max()), float(d.mean()))
    return out


def ratios(mode, errs, bar):
    """{name: (max / autocast's max, mean / autocast's mean)}"""
    return {n: (errs[n][0] / float(bar[f"{mode}.{n}"][0]), errs[n][1] / float(bar[f"{mode}.{n}"][1])) for n in NAMES}


def failures(rat):
    return {n: (round(a, 3), round(b, 3)) for n, (a, b) in rat.items() if not (a <= BAR_MAX and b <= BAR_MEAN)}
