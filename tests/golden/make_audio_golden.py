"""Writes tests/golden/audio_resample_cases.npz (needs scipy; the tests that read it do not).

Each case is a seeded block of PCM integers [n, C] of one width at one rate, and what scipy makes of it in float64:
``scipy.signal.resample_poly(x, up, down)`` at its defaults, x being the decoded samples (int / 2^(bits-1), 8-bit files offset
by 128) downmixed to one channel ("mean": the channel sum divided by C; "first": channel 0).  Nothing of calipsync_amd is used.

    meta [cases, 5] int64 = rate, n, width (bytes), channels, mono (0 mean, 1 first);  pcm_<i>;  y_<i> float64

Rates 8000 .. 96000; n = 1, 7, the inputs one output reaches (the filter span) -1 / +0 / +1, and about 3000; widths, channel
counts and mono modes cycle across the cases so that each occurs at several rates and lengths, the long cases with a cycle
of their own (every channel count and width at about 3000 frames).

Random ASYMMETRIC taps (the designed ones are symmetric, which hides a reversed tap order), an odd count 2 half + 1 of them:
``scipy.signal.upfirdn(taps, x, up, down)``, whose output j is sum_i x[i] taps[j down - i up].  The cases keep half a multiple of
down, so output k of the front end's formula (taps[k down + half - i up]) is upfirdn's k + half / down; ceil(n up / down) are kept.

    asym_meta [cases, 3] int64 = up, down, n;  asym_taps_<j>, asym_x_<j>, asym_y_<j> float64

    python tests/golden/make_audio_golden.py
"""
import math
import os

import numpy as np
from scipy import signal

RATES = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000)
HERE = os.path.dirname(os.path.abspath(__file__))


def lengths(rate):
    g = math.gcd(rate, 16000)
    up, down = 16000 // g, rate // g
    span = 2 * 10 * max(up, down) // up + 1
    return [1, 7, span - 1, span, span + 1, 2950 + 17 * RATES.index(rate)]


ASYMMETRIC = ((3, 7, 21, 500), (7, 3, 21, 300), (160, 441, 882, 1500), (2, 1, 5, 64), (1, 6, 60, 700))    # up, down, half, n


def draw(rng, n, channels, width):
    if width == 1:
        return rng.integers(0, 256, (n, channels), dtype=np.uint8)
    if width == 2:
        return rng.integers(-32768, 32768, (n, channels), dtype=np.int16)
    lim = 1 << (8 * width - 1)
    return rng.integers(-lim, lim, (n, channels), dtype=np.int64).astype(np.int32)


def main():
    rng = np.random.default_rng(20240917)
    meta, arrays = [], {}
    i = 0
    for rate in RATES:
        g = math.gcd(rate, 16000)
        up, down = 16000 // g, rate // g
        for n in lengths(rate):
            width = 1 + i % 4
            channels = 1 + (i // 2) % 3
            mono = (i // 12) % 2
            if n > 2500:                       # the long cases: 3 x 3 rates go through every channel count, 9 through the widths
                r = RATES.index(rate)
                width, channels, mono = 1 + r % 4, 1 + r % 3, (r // 3) % 2
            pcm = draw(rng, n, channels, width)
            x = pcm.astype(np.float64)
            if width == 1:
                x -= 128.0
            x /= float(1 << (8 * width - 1))
            x = x[:, 0] if mono else x.sum(axis=1) / channels
            y = signal.resample_poly(x, up, down)
            assert y.dtype == np.float64 and len(y) == -((-n * up) // down)
            arrays[f"pcm_{i}"] = pcm
            arrays[f"y_{i}"] = y
            meta.append((rate, n, width, channels, mono))
            i += 1
    meta = np.asarray(meta, dtype=np.int64)
    for col, name in ((2, "width"), (3, "channels"), (4, "mono")):      # each value at several rates
        for v in np.unique(meta[:, col]):
            assert len(np.unique(meta[meta[:, col] == v, 0])) >= 4, (name, v)
    for j, (up, down, half, n) in enumerate(ASYMMETRIC):
        assert half % down == 0
        taps, x = rng.standard_normal(2 * half + 1), rng.uniform(-1.0, 1.0, n)
        n_out = -((-n * up) // down)
        full = signal.upfirdn(taps, x, up, down)
        full = np.concatenate([full, np.zeros(max(0, half // down + n_out - len(full)))])     # past the last tap: zeros
        arrays[f"asym_taps_{j}"], arrays[f"asym_x_{j}"], arrays[f"asym_y_{j}"] = taps, x, full[half // down:half // down + n_out]
    arrays["asym_meta"] = np.asarray([(up, down, n) for up, down, _, n in ASYMMETRIC], dtype=np.int64)
    path = os.path.join(HERE, "audio_resample_cases.npz")
    np.savez_compressed(path, meta=meta, **arrays)
    print(path, len(meta), "cases", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 400_000


if __name__ == "__main__":
    main()
