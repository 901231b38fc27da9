"""Writes tests/golden/jpeg420_cases.npz: for every case of the 4:2:0 JPEG encoder's tests the seeded BGR input, the quality and
the bytes Pillow (libjpeg-turbo) writes for ``quality=q, subsampling=2, restart_marker_rows=1`` after the BGR -> RGB flip.  The
inputs come from the seeded generators of make_jpeg_golden.py.  The one full-size case stores its generator's seed, the SHA-256
and the length instead.  Needs a Pillow that knows ``restart_marker_rows`` (>= 10.2); run from the repository root:
python tests/golden/make_jpeg420_golden.py

The cases are the smallest at which the encoder can still go wrong.  Over the set the host twin's symbol statistics must show
every DC category 0..11, every AC category 1..10, a ZRL, a block without an EOB, a stuffed byte and an RST7 -> RST0 wrap, and the
sizes must include right-edge dummy Y blocks, a bottom row of dummy Y blocks, both at once, an odd width, an odd height, and a
row of more than 64 MCUs whose last MCU has dummy Y blocks."""
import hashlib
import importlib.util
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "jpeg420_cases.npz")

_spec = importlib.util.spec_from_file_location("make_jpeg_golden", os.path.join(HERE, "make_jpeg_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
noise, constant, stripes, smooth, steps, full_size = gen.noise, gen.constant, gen.stripes, gen.smooth, gen.steps, gen.full_size


def wide_steps(h, w):
    """16-pixel columns of one grey each: the DC differences between neighbouring MCUs walk through every category, and within
    an MCU they are 0"""
    return np.repeat(steps(h, w // 2), 2, axis=1)[:, :w]


# name -> (input, quality)
def small_cases():
    return {
        "constant_1x1_q95": (constant(1, 1), 95),
        "constant_16x16_q95": (constant(16, 16), 95),
        "noise_8x24_q95": (noise(1, 8, 24), 95),              # a right dummy, then a bottom row of dummies, in both MCUs
        "noise_17x17_q95": (noise(2, 17, 17), 95),            # odd both ways; the last MCU row and column hold one real Y block
        "noise_15x17_q50": (noise(3, 15, 17), 50),
        "noise_24x40_q1": (noise(4, 24, 40), 1),
        "noise_24x40_q10": (noise(4, 24, 40), 10),
        "noise_32x32_q100": (noise(5, 32, 32), 100),          # stuffed bytes, blocks without an EOB; the outgrown-slot case
        "noise_19x37_q95": (noise(6, 19, 37), 95),
        "stripes_16x64_q100": (stripes(16, 64), 100),
        "stripes_147x24_q95": (stripes(147, 24), 95),         # ten MCU rows: RST7 -> RST0, and an odd height
        "noise_16x1032_q95": (noise(7, 16, 1032), 95),        # 65 MCUs: a third pass of 32 whose only MCU has right dummies
        "smooth_56x48_q75": (smooth(8, 56, 48), 75),          # a bottom row of dummies under whole MCU columns
        "smooth_31x18_q95": (smooth(9, 31, 18), 95),
        "steps_16x288_q100": (wide_steps(16, 288), 100),      # added for the DC categories the others do not reach
    }


FULL = ("full_1080x1920_q95", 6, 95)


def pillow(frame_bgr, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame_bgr[:, :, ::-1])).save(buf, format="JPEG", quality=quality, subsampling=2,
                                                                      restart_marker_rows=1)
    return buf.getvalue()


def main():
    from calipsync_amd import jpeg
    cases = small_cases()
    arrays = {"names": np.asarray(sorted(cases))}
    dc, ac, zrl, no_eob, stuffed, wrap = set(), set(), 0, 0, 0, False
    sizes = []
    for name, (frame, q) in cases.items():
        data = pillow(frame, q)
        assert jpeg.encode_jpeg_host(frame, q, "4:2:0") == data, name
        arrays[name + ".input"] = frame
        arrays[name + ".quality"] = np.int32(q)
        arrays[name + ".jpeg"] = np.frombuffer(data, dtype=np.uint8)
        s = jpeg.symbol_statistics(frame, q, "4:2:0")
        dc |= s["dc"]
        ac |= s["ac"]
        zrl += s["zrl"]
        no_eob += s["no_eob"]
        stuffed += s["stuffed"]
        wrap |= s["rows"] > 9                             # RST0..RST7, then RST0 again after the ninth MCU row
        sizes.append(frame.shape[:2])
        print(f"{name}: {len(data)} bytes, dc {sorted(s['dc'])}, ac {sorted(s['ac'])}, zrl {s['zrl']}, no eob {s['no_eob']}, "
              f"stuffed {s['stuffed']}, rows {s['rows']}")
    assert dc == set(range(12)), sorted(dc)
    assert ac >= set(range(1, 11)), sorted(ac)
    assert zrl and no_eob and stuffed and wrap, (zrl, no_eob, stuffed, wrap)
    right = lambda w: 1 <= w % 16 <= 8
    bottom = lambda h: 1 <= h % 16 <= 8
    assert any(right(w) and not bottom(h) for h, w in sizes) and any(bottom(h) and not right(w) for h, w in sizes)
    assert any(right(w) and bottom(h) for h, w in sizes)
    assert any(w % 2 for _, w in sizes) and any(h % 2 for h, _ in sizes)
    assert any(w > 64 * 16 and right(w) for _, w in sizes)
    name, seed, q = FULL
    frame = full_size(seed)
    data = pillow(frame, q)
    assert jpeg.encode_jpeg_host(frame, q, "4:2:0") == data, name
    arrays[name + ".seed"] = np.int32(seed)
    arrays[name + ".quality"] = np.int32(q)
    arrays[name + ".sha256"] = np.frombuffer(hashlib.sha256(data).digest(), dtype=np.uint8)
    arrays[name + ".length"] = np.int64(len(data))
    np.savez_compressed(OUT, **arrays)
    print(f"{name}: {len(data)} bytes; {OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 300 * 1024


if __name__ == "__main__":
    main()
