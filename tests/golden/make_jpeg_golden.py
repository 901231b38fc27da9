"""Writes tests/golden/jpeg_cases.npz: for every case of the JPEG encoder's tests the seeded BGR input, the quality and the bytes
Pillow (libjpeg-turbo) writes for ``quality=q, subsampling=0, restart_marker_rows=1`` after the BGR -> RGB flip.  The one
full-size case stores its generator's seed, the SHA-256 and the length instead.  Needs a Pillow that knows
``restart_marker_rows`` (>= 10.2); run from the repository root:  python tests/golden/make_jpeg_golden.py

The cases are the smallest at which the encoder can still go wrong; over the set the host twin's symbol statistics must show
every DC category 0..11, every AC category 1..10, a ZRL, a block without an EOB, a stuffed byte and an RST7 -> RST0 wrap."""
import hashlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "jpeg_cases.npz")


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def constant(h, w):
    return np.full((h, w, 3), (31, 130, 222), dtype=np.uint8)


def stripes(h, w):
    """4-pixel columns of 0 / 255, inverted every 8 rows"""
    on = ((np.arange(w)[None, :] // 4) + (np.arange(h)[:, None] // 8)) % 2
    return np.repeat((on * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def smooth(seed, h, w):
    """a slow gradient with a little seeded tilt per channel: long zero runs"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = [40 + 170 * (a * x / max(w - 1, 1) + (1 - a) * y / max(h - 1, 1)) + 12 * np.sin(x / 9.0 + p) for a, p in rng.random((3, 2))]
    return np.clip(np.stack(chans, axis=2), 0, 255).astype(np.uint8)


def steps(h, w):
    """whole 8 x 8 blocks of one grey each, the levels chosen so that the DC differences of a row walk through every category"""
    levels = [128, 128, 129, 127, 130, 126, 134, 120, 140, 110, 150, 90, 170, 60, 200, 0, 255, 0]
    row = np.repeat(np.asarray(levels[:w // 8], dtype=np.uint8), 8)
    return np.repeat(np.repeat(row[None, :], h, axis=0)[:, :, None], 3, axis=2)


def full_size(seed):
    f = smooth(seed, 1080, 1920)
    f[500:570, 900:1100] = noise(seed + 1, 70, 200)
    return f


# name -> (input, quality)
def small_cases():
    return {
        "constant_8x8_q95": (constant(8, 8), 95),
        "noise_19x37_q95": (noise(1, 19, 37), 95),
        "noise_24x40_q1": (noise(2, 24, 40), 1),
        "noise_24x40_q10": (noise(2, 24, 40), 10),
        "noise_16x16_q100": (noise(3, 16, 16), 100),
        "stripes_16x64_q95": (stripes(16, 64), 95),
        "stripes_16x64_q100": (stripes(16, 64), 100),
        "stripes_83x24_q95": (stripes(83, 24), 95),
        "stripes_83x24_q100": (stripes(83, 24), 100),
        "noise_8x1032_q95": (noise(4, 8, 1032), 95),
        "smooth_64x48_q75": (smooth(5, 64, 48), 75),
        "steps_8x144_q100": (steps(8, 144), 100),       # added for the DC categories the others do not reach
    }


FULL = ("full_1080x1920_q95", 6, 95)


def pillow(frame_bgr, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame_bgr[:, :, ::-1])).save(buf, format="JPEG", quality=quality, subsampling=0,
                                                                      restart_marker_rows=1)
    return buf.getvalue()


def main():
    from calipsync_amd import jpeg
    cases = small_cases()
    arrays = {"names": np.asarray(sorted(cases))}
    dc, ac, zrl, no_eob, stuffed, wrap = set(), set(), 0, 0, 0, False
    for name, (frame, q) in cases.items():
        data = pillow(frame, q)
        assert jpeg.encode_jpeg_host(frame, q) == data, name
        arrays[name + ".input"] = frame
        arrays[name + ".quality"] = np.int32(q)
        arrays[name + ".jpeg"] = np.frombuffer(data, dtype=np.uint8)
        s = jpeg.symbol_statistics(frame, q)
        dc |= s["dc"]
        ac |= s["ac"]
        zrl += s["zrl"]
        no_eob += s["no_eob"]
        stuffed += s["stuffed"]
        wrap |= s["rows"] > 9                             # RST0..RST7, then RST0 again after the ninth row
        print(f"{name}: {len(data)} bytes, dc {sorted(s['dc'])}, ac {sorted(s['ac'])}, zrl {s['zrl']}, no eob {s['no_eob']}, "
              f"stuffed {s['stuffed']}, rows {s['rows']}")
    assert dc == set(range(12)), sorted(dc)
    assert ac >= set(range(1, 11)), sorted(ac)
    assert zrl and no_eob and stuffed and wrap, (zrl, no_eob, stuffed, wrap)
    name, seed, q = FULL
    data = pillow(full_size(seed), q)
    arrays[name + ".seed"] = np.int32(seed)
    arrays[name + ".quality"] = np.int32(q)
    arrays[name + ".sha256"] = np.frombuffer(hashlib.sha256(data).digest(), dtype=np.uint8)
    arrays[name + ".length"] = np.int64(len(data))
    np.savez_compressed(OUT, **arrays)
    print(f"{name}: {len(data)} bytes; {OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 300 * 1024


if __name__ == "__main__":
    main()
