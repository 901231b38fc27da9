"""Writes tests/golden/mjpeg_decode_cases.npz: the JPEG files of the wider decoder subset (``subset="mjpeg"``: 4:2:2, grayscale,
files without their Huffman tables) as Pillow (libjpeg-turbo) wrote them, with the pixels Pillow decodes from them
(``Image.open(...).convert("RGB")``, reversed to BGR), or the SHA-256 of those pixels for the larger frames, in the manner of
make_jpeg_decode_golden.py, whose seeded frames and Pillow helpers it uses.  Run from the repository root:
python tests/golden/make_mjpeg_decode_golden.py

4:2:2 sizes (h x w): one pixel and 1 x 2 (one chroma column: both output columns are copies), one MCU (8 x 16), an MCU row whose
last MCU is half used (8 x 9: its second Y block is a dummy), odd chroma widths (9 x 17, 17 x 23), whole MCUs (48 x 64) and
8 x 1031, an odd width whose rows cross a workgroup of the colour kernel (256 lanes of four pixels).  Gray sizes: one pixel, one
block, odd sizes, whole blocks.  Every size (the long row: three of them) meets every setting on a noise and on a smooth frame: Pillow's default tables and
per-file tables, no restart markers, one interval per MCU row, one per three MCUs (which ends inside an MCU row), qualities 30,
95 and 100.  Then the files without Huffman tables: every DHT segment stripped from a 48 x 64 file of each of the four
samplings, and a 4:2:2 file that lost only AC 1, and one that lost DC 1 and AC 0; Pillow reads each with the Annex K tables in
the place of the missing ones, and its pixels of those files are recorded like the others."""
import hashlib
import importlib.util
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "mjpeg_decode_cases.npz")

_spec = importlib.util.spec_from_file_location("make_jpeg_decode_golden", os.path.join(HERE, "make_jpeg_decode_golden.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

SIZES_422 = ((1, 1), (1, 2), (8, 16), (8, 9), (9, 17), (17, 23), (48, 64), (8, 1031))          # h x w
SIZES_GRAY = ((1, 1), (8, 8), (9, 9), (17, 23), (48, 64))
SETTINGS = {
    "default": {},
    "optimize": {"optimize": True},
    "rstrows": {"restart_marker_rows": 1},
    "rstblocks": {"restart_marker_blocks": 3},
    "q30": {"quality": 30},
    "q95": {"quality": 95},
    "q100": {"quality": 100},
}
KINDS = ("noise", "smooth")
PIXELS_UP_TO = 64 * 64          # larger frames store the SHA-256 of their pixels
LONG_ROW = (8, 1031)            # its files are the fixture's largest: it meets three settings, every other size all of them
LONG_ROW_SETTINGS = ("default", "rstblocks", "q100")
# name -> (sampling, the (class, id) of the DHT tables taken out; None: all of them)
NO_DHT = {
    "nodht444_48x64_all": ("444", None),
    "nodht422_48x64_all": ("422", None),
    "nodht420_48x64_all": ("420", None),
    "nodhtgray_48x64_all": ("gray", None),
    "nodht422_48x64_ac1": ("422", ((1, 1),)),
    "nodht422_48x64_dc1ac0": ("422", ((0, 1), (1, 0))),
}
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def frame(kind, h, w):
    return base.frame(kind, h, w)


def pillow_write(frame_bgr, sampling, **settings):
    """the frame as a JPEG file of the sampling: "444", "422", "420", or "gray" (its green channel as a mode "L" image)"""
    if sampling == "gray":
        import io
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(frame_bgr[:, :, 1])).save(buf, format="JPEG", **settings)
        return buf.getvalue()
    return base.pillow_write(frame_bgr, subsampling=SUBSAMPLING[sampling], **settings)


pillow_read = base.pillow_read


def strip_dht(data: bytes, which=None) -> bytes:
    """the file without the Huffman tables `which` ((class, id) pairs; None: every DHT segment goes): the other tables of a
    segment that loses some are written back as one segment"""
    out, pos = bytearray(data[:2]), 2
    while True:
        marker, length = data[pos + 1], struct.unpack(">H", data[pos + 2:pos + 4])[0]
        body = data[pos + 4:pos + 2 + length]
        if marker == 0xC4:
            kept, at = b"", 0
            while at < len(body):
                n = 17 + sum(body[at + 1:at + 17])
                if which is not None and (body[at] >> 4, body[at] & 15) not in which:
                    kept += body[at:at + n]
                at += n
            if kept:
                out += b"\xff\xc4" + struct.pack(">H", len(kept) + 2) + kept
        else:
            out += data[pos:pos + 2 + length]
        pos += 2 + length
        if marker == 0xDA:
            return bytes(out) + data[pos:]


def settings_of(h, w):
    return {k: v for k, v in SETTINGS.items() if (h, w) != LONG_ROW or k in LONG_ROW_SETTINGS}


def case_name(sampling, kind, h, w, setting):
    return f"{'c422' if sampling == '422' else 'gray'}{kind}_{h}x{w}_{setting}"


def main():
    out, names = {}, []

    def record(name, data, shape):
        px = pillow_read(data)
        assert px.shape == shape, (name, px.shape)
        names.append(name)
        out[name + ".jpeg"] = np.frombuffer(data, dtype=np.uint8)
        if shape[0] * shape[1] <= PIXELS_UP_TO:
            out[name + ".pixels"] = px
        else:
            out[name + ".sha256"] = np.frombuffer(hashlib.sha256(px.tobytes()).digest(), dtype=np.uint8)

    for sampling, sizes in (("422", SIZES_422), ("gray", SIZES_GRAY)):
        for h, w in sizes:
            for setting, kw in settings_of(h, w).items():
                for kind in KINDS:
                    record(case_name(sampling, kind, h, w, setting), pillow_write(frame(kind, h, w), sampling, **kw), (h, w, 3))
    for name, (sampling, which) in NO_DHT.items():
        whole = pillow_write(frame("noise", 48, 64), sampling)
        data = strip_dht(whole, which)
        assert len(data) < len(whole) and (which is not None or b"\xff\xc4" not in data[:data.index(b"\xff\xda")])
        assert (pillow_read(data) == pillow_read(whole)).all()           # Pillow puts the Annex K tables where none is defined
        record(name, data, (48, 64, 3))
    out["names"] = np.asarray(names)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(names)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
