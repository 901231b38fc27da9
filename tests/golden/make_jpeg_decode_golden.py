"""Writes tests/golden/jpeg_decode_cases.npz: JPEG files Pillow (libjpeg-turbo) wrote, as uint8 arrays, with the pixels Pillow
decodes from them (``Image.open(...).convert("RGB")``, reversed to BGR), or the SHA-256 of those pixels for the larger frames.
The inputs come from the seeded generators of make_jpeg_golden.py.  Every size meets every setting on a noise and on a smooth
frame.  The full-size case stores only the SHA-256 of Pillow's decode of the host twin's 4:2:0 file of jpeg420_cases' seeded
1080 x 1920 frame.  Needs a Pillow that knows ``restart_marker_rows`` (>= 10.2); run from the repository root:
python tests/golden/make_jpeg_decode_golden.py

The sizes are the smallest at which the decoder can still go wrong: one pixel, less than a block, one block, odd sizes with
dummy Y blocks on the right and at the bottom, a bottom chroma row that comes from the real plane (17, 33), whole MCUs (48 x 64)
and a scan long enough for thousands of subsequences (256 x 256).  The settings: Pillow's defaults (4:2:0, Annex K tables, no
restart markers: what the reference's step 3 writes), 4:4:4, per-file Huffman tables, one restart interval per MCU row, one per
three MCUs, and qualities 30 and 100 (the latter dense in stuffed bytes)."""
import hashlib
import importlib.util
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "jpeg_decode_cases.npz")

_spec = importlib.util.spec_from_file_location("make_jpeg_golden", os.path.join(HERE, "make_jpeg_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

SIZES = ((1, 1), (7, 5), (8, 8), (17, 33), (33, 18), (48, 64), (256, 256))          # h x w
SETTINGS = {
    "default": {},
    "sub0": {"subsampling": 0},
    "optimize": {"optimize": True},
    "rstrows": {"restart_marker_rows": 1},
    "rstblocks": {"restart_marker_blocks": 3},
    "q30": {"quality": 30},
    "q100": {"quality": 100},
}
KINDS = ("noise", "smooth")
PIXELS_UP_TO = 64 * 64          # larger frames store the SHA-256 of their pixels
FULL = "full_1080x1920_q95"


def frame(kind, h, w):
    seed = 1000 * h + w
    return gen.noise(seed, h, w) if kind == "noise" else gen.smooth(seed, h, w)


def pillow_write(frame_bgr, **settings):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame_bgr[:, :, ::-1])).save(buf, format="JPEG", **settings)
    return buf.getvalue()


def pillow_read(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def case_name(kind, h, w, setting):
    return f"{kind}_{h}x{w}_{setting}"


def main():
    from calipsync_amd import jpeg
    out, names = {}, []
    for h, w in SIZES:
        for setting, kw in SETTINGS.items():
            for kind in KINDS:
                name = case_name(kind, h, w, setting)
                data = pillow_write(frame(kind, h, w), **kw)
                px = pillow_read(data)
                assert px.shape == (h, w, 3)
                names.append(name)
                out[name + ".jpeg"] = np.frombuffer(data, dtype=np.uint8)
                if h * w <= PIXELS_UP_TO:
                    out[name + ".pixels"] = px
                else:
                    out[name + ".sha256"] = np.frombuffer(hashlib.sha256(px.tobytes()).digest(), dtype=np.uint8)
    spec = importlib.util.spec_from_file_location("make_jpeg420_golden", os.path.join(HERE, "make_jpeg420_golden.py"))
    g420 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g420)
    _, seed, quality = g420.FULL
    data = jpeg.encode_jpeg_host(g420.full_size(seed), quality, "4:2:0")
    out[FULL + ".sha256"] = np.frombuffer(hashlib.sha256(pillow_read(data).tobytes()).digest(), dtype=np.uint8)
    out[FULL + ".file_sha256"] = np.frombuffer(hashlib.sha256(data).digest(), dtype=np.uint8)
    out["names"] = np.asarray(names)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(names)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
