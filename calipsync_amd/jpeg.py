"""Baseline JPEG of finished frames, on the device (csrc/jpeg_enc.hip) and its numpy twin.

One bitstream, two encoders: uint8 BGR frames -> JFIF 1.1, 4:4:4, the Annex K Huffman tables, one restart interval per row
of 8 x 8 blocks.  The arithmetic is libjpeg's integer baseline path end to end (16-bit fixed-point colour, the accurate
integer DCT, round-half-away quantisation), so the bytes are those of Pillow's
``save(format="JPEG", quality=q, subsampling=0, restart_marker_rows=1)`` on the RGB view of the frame (tests/test_jpeg.py).

    files = encode_jpeg_device(frames_dev, quality=95)     # [B,H,W,3] uint8 on the device -> B complete files
    data = encode_jpeg_host(frame_bgr, quality=95)         # the same bytes from numpy

``subsampling="4:2:0"`` (or 2, Pillow's number) on either entry writes libjpeg's default chroma sampling instead (csrc/jpeg_enc420.hip,
DESIGN.md section 8i): Y sampled 2 x 2, Cb and Cr averaged 2 x 2, one restart interval per row of 16 x 16 MCUs, the bytes of
Pillow's ``subsampling=2``.  4:4:4 stays the default.

The restart markers make the block rows independent: the device encodes one row per wave.  The host twin is the fallback for
a frame whose row outgrew its scratch slot, the subject of the CPU tests and the yardstick for inputs without a fixture.

The way back, baseline JPEG files -> frames (csrc/jpeg_dec.hip), is the second half of this file:

    frames_dev = decode_jpeg_device(files)                 # B files of one size -> [B,H,W,3] uint8 BGR on the device
    frame_bgr = decode_jpeg_host(data)                     # the same bytes from numpy: Pillow's, reversed to BGR

``subset="mjpeg"`` on the decoding entries (csrc/jpeg_dec_mjpeg.hip) widens what they read from 4:4:4 and
4:2:0 to what Motion-JPEG writers produce: 4:2:2, grayscale, and frames that leave out their Huffman tables.  "baseline" stays the
default."""
from __future__ import annotations

import ctypes as C
import struct
from typing import List

import numpy as np

HEADER_BYTES = 629

# ITU-T T.81 Annex K.1, in zigzag order (the order of a DQT segment)
BASE_LUMA = (16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
             56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92,
             101, 103, 99)
BASE_CHROMA = (17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99) + (99,) * 48
# zigzag position -> row-major position of an 8 x 8 block
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
          56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# Annex K.3: (codes of each length 1..16, symbols in code order)
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),
           (1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36,
            51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74,
            83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133,
            134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179,
            180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
            225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),
             (0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
              21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71,
              72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122,
              130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168,
              169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214,
              215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250))


def _check_size(H: int, W: int, quality: int) -> None:
    if not (1 <= int(H) <= 65535 and 1 <= int(W) <= 65535):
        raise ValueError(f"jpeg: a frame of {H} x {W} (h x w) is outside 1..65535")
    if not (1 <= int(quality) <= 100) or int(quality) != quality:
        raise ValueError(f"jpeg: quality {quality!r} is outside 1..100")


def quant_tables(quality: int):
    """(luma, chroma) as int32 [64] in zigzag order: libjpeg's quality scaling of the Annex K tables, 8-bit entries."""
    _check_size(1, 1, quality)
    q = int(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(base, dtype=np.int64) * scale + 50) // 100, 1, 255).astype(np.int32) for base in (BASE_LUMA, BASE_CHROMA))


def _huff(table):
    """symbol -> (code, length) arrays [256] of an Annex K table (Annex C: codes count up within a length)."""
    bits, vals = table
    code = np.zeros(256, dtype=np.int64)
    size = np.zeros(256, dtype=np.int64)
    c, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            code[vals[k]], size[vals[k]] = c, length
            c += 1
            k += 1
        c <<= 1
    return code, size


_HUFF = None


def _huff_tables():
    global _HUFF
    if _HUFF is None:
        _HUFF = tuple(_huff(t) for t in (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA))
    return _HUFF


def _subsampling(subsampling) -> int:
    """"4:4:4" / 0 -> 0, "4:2:0" / 2 -> 2 (Pillow's numbers); anything else is a ValueError"""
    if isinstance(subsampling, str):
        if subsampling in ("4:4:4", "4:2:0"):
            return 0 if subsampling == "4:4:4" else 2
    elif not isinstance(subsampling, bool) and isinstance(subsampling, (int, np.integer)) and int(subsampling) in (0, 2):
        return int(subsampling)
    raise ValueError(f"jpeg: subsampling {subsampling!r} is neither '4:4:4' / 0 nor '4:2:0' / 2")


def jpeg_header(H: int, W: int, quality: int = 95, subsampling="4:4:4") -> bytes:
    """Everything ahead of the scan, 629 bytes for any size and quality: SOI, APP0 (JFIF 1.1), the two DQT, SOF0, the four
    DHT, DRI (one restart interval per block row; per row of 16 x 16 MCUs at 4:2:0, where Y samples 2 x 2) and SOS."""
    _check_size(H, W, quality)
    H, W = int(H), int(W)
    sub = _subsampling(subsampling)
    seg = lambda marker, body: bytes((0xFF, marker)) + struct.pack(">H", len(body) + 2) + body
    luma, chroma = quant_tables(quality)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes((1, 1, 0, 0, 1, 0, 1, 0, 0)))
    out += seg(0xDB, bytes([0]) + bytes(int(v) for v in luma)) + seg(0xDB, bytes([1]) + bytes(int(v) for v in chroma))
    out += seg(0xC0, bytes([8]) + struct.pack(">HH", H, W) + bytes((3, 1, 0x22 if sub else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for ident, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += seg(0xC4, bytes([ident]) + bytes(bits) + bytes(vals))
    out += seg(0xDD, struct.pack(">H", (W + 15) // 16 if sub else (W + 7) // 8)) + seg(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))
    assert len(out) == HEADER_BYTES
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first: bool):
    """One pass of the accurate integer DCT along the last axis of d [..., 8] (int64); libjpeg's jfdctint, 13 constant bits and 2
    extra bits between the passes."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = np.empty_like(d)
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[..., 2] = _descale(z1 + t13 * 6270, n)
    out[..., 6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def _ycc(f: np.ndarray) -> np.ndarray:
    """[3, H, W] int64: libjpeg's 16-bit fixed-point Y, Cb, Cr of the unshifted 0..255 samples of a BGR frame"""
    b, g, r = (f[:, :, i].astype(np.int64) for i in range(3))
    half = 128 << 16
    return np.stack([(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                     (-11059 * r - 21709 * g + 32768 * b + half + 32767) >> 16,
                     (32768 * r - 27439 * g - 5329 * b + half + 32767) >> 16])


def _transform(planes: np.ndarray, div: np.ndarray) -> np.ndarray:
    """Level-shifted planes [..., 8 r, 8 c] -> [..., r, c, 64 (zigzag order)]: the two DCT passes and the round-half-away
    quantisation by div (8 Q, zigzag order, broadcast against the result)."""
    rows, cols = planes.shape[-2] // 8, planes.shape[-1] // 8
    lead = planes.shape[:-2]
    n = len(lead)
    blocks = planes.reshape(lead + (rows, 8, cols, 8)).transpose(tuple(range(n)) + (n, n + 2, n + 1, n + 3))
    coef = _fdct_pass(np.ascontiguousarray(blocks), True)                             # along x
    coef = _fdct_pass(np.ascontiguousarray(coef.swapaxes(-1, -2)), False).swapaxes(-1, -2)    # along y
    coef = coef.reshape(lead + (rows, cols, 64))[..., list(ZIGZAG)]
    mag = (np.abs(coef) + (div >> 1)) // div
    return np.where(coef < 0, -mag, mag)


def quantized_blocks_420(frame_bgr: np.ndarray, quality: int = 95):
    """The 4:2:0 scan of a frame, (q [MCU rows, MCUs per row, 6 (Y00, Y01, Y10, Y11, Cb, Cr), 64 (zigzag order)] int64,
    dummy [MCU rows, MCUs per row, 6] bool).  Y is padded by edge replication to whole 8 x 8 blocks only: a Y block of an MCU
    past those is a dummy, all zero but for the DC of the Y block before it in its MCU, so it codes as difference 0 and EOB.
    Chroma: the full-resolution planes are padded on the right to whole MCUs (and by one row under an odd H), averaged 2 x 2
    with libjpeg's alternating bias 1, 2, and the last *downsampled* row is repeated to whole blocks."""
    f = np.asarray(frame_bgr)
    H, W = f.shape[:2]
    luma, chroma = (8 * t.astype(np.int64) for t in quant_tables(quality))
    ycc = _ycc(f)
    mrows, mcols = (H + 15) // 16, (W + 15) // 16
    y = np.pad(ycc[0], ((0, -H % 8), (0, -W % 8)), mode="edge") - 128
    yq = _transform(y, luma)                                                          # [ceil(H/8), ceil(W/8), 64]
    q = np.zeros((2 * mrows, 2 * mcols, 64), dtype=np.int64)
    q[:yq.shape[0], :yq.shape[1]] = yq
    dummy = np.ones((2 * mrows, 2 * mcols), dtype=bool)
    dummy[:yq.shape[0], :yq.shape[1]] = False
    mcu = lambda a: a.reshape((mrows, 2, mcols, 2) + a.shape[2:]).swapaxes(1, 2).reshape((mrows, mcols, 4) + a.shape[2:])
    q, dummy = mcu(q), mcu(dummy)
    for k in range(1, 4):                                                             # block 0 of an MCU is never a dummy
        q[..., k, 0] = np.where(dummy[..., k], q[..., k - 1, 0], q[..., k, 0])
    c = np.pad(ycc[1:], ((0, 0), (0, H % 2), (0, 16 * mcols - W)), mode="edge")
    bias = np.where(np.arange(8 * mcols) % 2, 2, 1)
    c = (c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2] + bias) >> 2
    c = np.pad(c, ((0, 0), (0, 8 * mrows - c.shape[1]), (0, 0)), mode="edge") - 128
    cq = _transform(c, chroma)                                                        # [2, mrows, mcols, 64]
    q = np.concatenate([q, cq.transpose(1, 2, 0, 3)], axis=2)
    return q, np.concatenate([dummy, np.zeros((mrows, mcols, 2), dtype=bool)], axis=2)


def quantized_blocks(frame_bgr: np.ndarray, quality: int = 95) -> np.ndarray:
    """The quantised coefficients [block rows, MCUs per row, 3 (Y, Cb, Cr), 64 (zigzag order)] int64 of a frame: colour
    conversion, edge replication, DCT and quantisation, vectorised over every block."""
    f = np.asarray(frame_bgr)
    H, W = f.shape[:2]
    luma, chroma = quant_tables(quality)
    ycc = _ycc(f) - 128
    ycc = np.pad(ycc, ((0, 0), (0, -H % 8), (0, -W % 8)), mode="edge")
    rows, cols = ycc.shape[1] // 8, ycc.shape[2] // 8
    blocks = ycc.reshape(3, rows, 8, cols, 8).transpose(1, 3, 0, 2, 4)               # [rows, cols, 3, y, x]
    coef = _fdct_pass(np.ascontiguousarray(blocks), True)                             # along x
    coef = _fdct_pass(np.ascontiguousarray(coef.swapaxes(-1, -2)), False).swapaxes(-1, -2)    # along y
    coef = coef.reshape(rows, cols, 3, 64)[..., list(ZIGZAG)]
    div = 8 * np.stack([luma, chroma, chroma]).astype(np.int64)                       # [3, 64]
    mag = (np.abs(coef) + (div >> 1)) // div
    return np.where(coef < 0, -mag, mag)


def _bit_length(v: np.ndarray) -> np.ndarray:
    """bit length of non-negative int64 values < 2^15"""
    n = np.zeros(v.shape, dtype=np.int64)
    for s in range(15):
        n += (v >> s) > 0
    return n


def scan_symbols(q: np.ndarray, components=(0, 1, 2)):
    """The code words of a scan, vectorised over every block: q [rows, cols, blocks of an MCU, 64] quantised coefficients, of
    which block k belongs to components[k] (0 Y, 1 Cb, 2 Cr) -> (row [n], code [n], length [n], kind [n]) in stream order, where
    kind is 0 for a DC code (its category is length's companion in the symbol statistics), 1 for an AC code, 2 for ZRL and 3 for
    EOB, and (dc categories [n_dc], ac categories [n_ac]) for the statistics."""
    rows, cols, nb = q.shape[:3]
    components = np.asarray(components, dtype=np.int64)
    (dcl_c, dcl_s), (acl_c, acl_s), (dcc_c, dcc_s), (acc_c, acc_s) = _huff_tables()
    dc_code = np.stack([dcl_c, dcc_c, dcc_c])
    dc_size = np.stack([dcl_s, dcc_s, dcc_s])
    ac_code = np.stack([acl_c, acc_c, acc_c])
    ac_size = np.stack([acl_s, acc_s, acc_s])
    comp = np.broadcast_to(components[None, None, :], (rows, cols, nb))
    # order key of a code word: ((row, col, block), k, sub) with sub = position among the words one coefficient emits
    block_id = (np.arange(rows)[:, None, None] * cols + np.arange(cols)[None, :, None]) * nb + np.arange(nb)[None, None, :]

    def words(v, huff_code, huff_size):
        cat = _bit_length(np.abs(v))
        low = np.where(v < 0, v - 1, v) & ((1 << cat) - 1)
        return cat, (huff_code << cat) | low, huff_size + cat

    # DC: difference against the previous block of the same component in the row
    dc = q[..., 0]
    diff = np.empty_like(dc)
    for c in range(3):
        mine = np.nonzero(components == c)[0]
        seq = dc[:, :, mine].reshape(rows, -1)
        diff[:, :, mine] = (seq - np.concatenate([np.zeros((rows, 1), dtype=np.int64), seq[:, :-1]], axis=1)).reshape(rows, cols, -1)
    dc_cat = _bit_length(np.abs(diff))
    _, code, size = words(diff, dc_code[comp, dc_cat], dc_size[comp, dc_cat])
    keys = [block_id.reshape(-1) * 64 * 4]
    codes, sizes, kinds = [code.reshape(-1)], [size.reshape(-1)], [np.zeros(code.size, dtype=np.int64)]
    # AC: run = zeros since the previous non-zero coefficient of the block
    ac = q[..., 1:]
    nz = ac != 0
    pos = np.arange(1, 64)
    last = np.maximum.accumulate(np.where(nz, pos, 0), axis=-1)                        # position of the latest non-zero up to k
    prev = np.concatenate([np.zeros(last.shape[:-1] + (1,), dtype=np.int64), last[..., :-1]], axis=-1)
    run = pos - prev - 1                                                               # at a non-zero k
    bi, ki = np.nonzero(nz.reshape(-1, 63))
    v = ac.reshape(-1, 63)[bi, ki]
    r = run.reshape(-1, 63)[bi, ki]
    c = comp.reshape(-1)[bi]
    cat = _bit_length(np.abs(v))
    sym = ((r & 15) << 4) | cat
    _, code, size = words(v, ac_code[c, sym], ac_size[c, sym])
    key = (block_id.reshape(-1)[bi] * 64 + ki + 1) * 4
    keys.append(key + 3)
    codes.append(code)
    sizes.append(size)
    kinds.append(np.ones(code.size, dtype=np.int64))
    for j in range(3):                                                                 # up to three ZRL ahead of a coefficient
        m = (r >> 4) > j
        keys.append(key[m] + j)
        codes.append(ac_code[c[m], 0xF0])
        sizes.append(ac_size[c[m], 0xF0])
        kinds.append(np.full(int(m.sum()), 2, dtype=np.int64))
    eob = (last[..., -1] != 63).reshape(-1)                                            # the block ends in zeros
    ce = comp.reshape(-1)[eob]
    keys.append((block_id.reshape(-1)[eob] * 64 + 63) * 4 + 3)
    codes.append(ac_code[ce, 0])
    sizes.append(ac_size[ce, 0])
    kinds.append(np.full(int(eob.sum()), 3, dtype=np.int64))
    key = np.concatenate(keys)
    order = np.argsort(key, kind="stable")
    key = key[order]
    return (key // (cols * nb * 64 * 4), np.concatenate(codes)[order], np.concatenate(sizes)[order], np.concatenate(kinds)[order],
            (dc_cat.reshape(-1), cat))


def _pack_rows(row, code, size, rows: int) -> List[bytes]:
    """Code words -> per block row its bytes, MSB first, padded to a byte with 1-bits (not yet stuffed)."""
    total = np.zeros(rows, dtype=np.int64)
    np.add.at(total, row, size)
    pad = -total % 8
    start = np.concatenate([[0], np.cumsum(total + pad)])                              # bit offset of each row
    nbits = int(start[-1])
    bits = np.zeros(nbits, dtype=np.uint8)
    csum = np.cumsum(size) - size                                                      # exclusive, over the whole stream
    row_first = np.concatenate([[0], np.cumsum(total)])[:-1]
    at = csum - row_first[row] + start[row]                                            # bit position of each code word
    for j in range(int(size.max()) if size.size else 0):                               # bit j of every word at once (at most 26)
        m = size > j
        bits[at[m] + j] = (code[m] >> (size[m] - 1 - j)) & 1
    for r in range(rows):
        if pad[r]:
            bits[start[r + 1] - pad[r]:start[r + 1]] = 1
    packed = np.packbits(bits).tobytes()
    return [packed[start[r] // 8:start[r + 1] // 8] for r in range(rows)]


def _check_frame(frame_bgr) -> np.ndarray:
    f = np.asarray(frame_bgr)
    if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
        raise ValueError(f"jpeg: frames must be uint8 HxWx3 (BGR), got {f.dtype} {f.shape}")
    return f


Y420 = (0, 0, 0, 0, 1, 2)         # the component of each block of a 4:2:0 MCU


def _scan_blocks(f: np.ndarray, quality: int, sub: int):
    """(q [restart rows, MCUs per row, blocks of an MCU, 64], the component of each block of an MCU)"""
    if sub:
        return quantized_blocks_420(f, quality)[0], Y420
    return quantized_blocks(f, quality), (0, 1, 2)


def encode_jpeg_host(frame_bgr: np.ndarray, quality: int = 95, subsampling="4:4:4") -> bytes:
    """One BGR uint8 [H,W,3] frame as a complete baseline JPEG file: the numpy twin of the device encoder, 4:4:4 or 4:2:0."""
    f = _check_frame(frame_bgr)
    sub = _subsampling(subsampling)
    H, W = f.shape[:2]
    out = [jpeg_header(H, W, quality, sub)]
    q, components = _scan_blocks(f, quality, sub)
    rows = q.shape[0]
    row, code, size, _, _ = scan_symbols(q, components)
    for r, data in enumerate(_pack_rows(row, code, size, rows)):
        out.append(data.replace(b"\xff", b"\xff\x00"))
        out.append(bytes((0xFF, 0xD0 + (r & 7))) if r + 1 < rows else b"\xff\xd9")
    return b"".join(out)


def symbol_statistics(frame_bgr: np.ndarray, quality: int = 95, subsampling="4:4:4") -> dict:
    """What the scan of a frame exercises (tests/golden/make_jpeg_golden.py and make_jpeg420_golden.py assert coverage over their
    cases): the DC and AC categories seen, the number of ZRL codes, of blocks without an EOB, of stuffed bytes, and the restart
    rows (block rows at 4:4:4, MCU rows at 4:2:0)."""
    f = _check_frame(frame_bgr)
    q, components = _scan_blocks(f, quality, _subsampling(subsampling))
    rows = q.shape[0]
    row, code, size, kind, (dc_cat, ac_cat) = scan_symbols(q, components)
    stuffed = sum(d.count(b"\xff") for d in _pack_rows(row, code, size, rows))
    return {"dc": set(int(v) for v in np.unique(dc_cat)), "ac": set(int(v) for v in np.unique(ac_cat)),
            "zrl": int((kind == 2).sum()), "no_eob": int(q.shape[0] * q.shape[1] * q.shape[2] - (kind == 3).sum()),
            "stuffed": int(stuffed), "rows": int(rows)}


# ---------------------------------------------------------------------------------------------------------------- device
def default_slot_bytes(W: int, subsampling="4:4:4") -> int:
    """The scratch slot of one restart row when slot_bytes = 0: twice the raw bytes of the samples it codes (a block row of
    three planes at 4:4:4; at 4:2:0 an MCU row, 384 samples per 16 x 16 MCU)."""
    if _subsampling(subsampling):
        return 2 * 384 * ((int(W) + 15) // 16)
    return 2 * 8 * 3 * 8 * ((int(W) + 7) // 8)


def restart_rows(H: int, subsampling="4:4:4") -> int:
    """Restart intervals of a frame: rows of 8 x 8 blocks at 4:4:4, of 16 x 16 MCUs at 4:2:0"""
    return (int(H) + 15) // 16 if _subsampling(subsampling) else (int(H) + 7) // 8


def _entry(name: str, sub: int) -> str:
    """casync_op_jpeg_<name> or its 4:2:0 sibling casync_op_jpeg420_<name>"""
    return f"casync_op_jpeg420_{name}" if sub else f"casync_op_jpeg_{name}"


def _header_from_lib(H: int, W: int, quality: int, subsampling="4:4:4") -> bytes:
    from . import _lib
    entry = _entry("header", _subsampling(subsampling))
    buf = (C.c_uint8 * HEADER_BYTES)()
    n = _lib.check(getattr(_lib.load(), entry)(H, W, quality, buf, HEADER_BYTES), entry)
    return bytes(buf[:n])


def encode_jpeg_op(frames, quality: int, slot_bytes: int, scratch, out, offsets, status, subsampling="4:4:4") -> None:
    """casync_op_jpeg_encode (casync_op_jpeg420_encode for 4:2:0) on torch's current stream, every buffer the caller's (uint8
    scratch and out, int64 offsets [B+1], int32 status [B]); nothing is waited for."""
    import torch
    from . import _lib
    entry = _entry("encode", _subsampling(subsampling))
    B, H, W = (int(v) for v in frames.shape[:3])
    _lib.check(getattr(_lib.load(), entry)(frames.data_ptr(), B, H, W, int(quality), int(slot_bytes), scratch.data_ptr(),
                                           scratch.numel(), out.data_ptr(), out.numel(), offsets.data_ptr(), status.data_ptr(),
                                           torch.cuda.current_stream(frames.device).cuda_stream), entry)


def encode_jpeg_device(frames, quality: int = 95, *, subsampling="4:4:4", slot_bytes: int = 0) -> List[bytes]:
    """uint8 [B,H,W,3] BGR frames on the device -> B complete JPEG files, encoded where they lie (torch's current stream).
    Two copies cross to the host: offsets and status, then exactly the bytes produced (through ``frame_loop``'s pinned pool).
    A frame whose row outgrew its ``slot_bytes`` scratch slot (0: twice the row's raw bytes) is downloaded alone and encoded
    by ``encode_jpeg_host``, so the caller always gets B valid files.  ``subsampling`` "4:2:0" writes what libjpeg writes by
    default: chroma at half resolution both ways, six blocks per 16 x 16 pixels in place of twelve."""
    import torch
    sub = _subsampling(subsampling)
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        what = f"{tuple(frames.shape)} {frames.dtype}" if isinstance(frames, torch.Tensor) else type(frames).__name__
        raise ValueError(f"encode_jpeg_device: needs a uint8 [B,H,W,3] tensor, got {what}")
    B, H, W = (int(v) for v in frames.shape[:3])
    if B:
        _check_size(H, W, quality)
    else:
        _check_size(1, 1, quality)
    if int(slot_bytes) < 0:
        raise ValueError(f"encode_jpeg_device: slot_bytes {slot_bytes}")
    if frames.device.type != "cuda":
        raise RuntimeError("encode_jpeg_device needs the frames on a ROCm device (encode_jpeg_host is the host encoder)")
    if B == 0:
        return []
    from . import _lib, frame_loop
    lib = _lib.load()
    frames = frames.contiguous()
    dev = frames.device
    slot = int(slot_bytes) or default_slot_bytes(W, sub)
    rows = restart_rows(H, sub)
    need = getattr(lib, _entry("workspace_bytes", sub))(B, H, W, slot)
    if need < 0:
        _lib.check(int(need), _entry("workspace_bytes", sub))
    cap = B * (HEADER_BYTES + rows * slot)                     # a frame that passed its slots fits here
    with torch.cuda.device(dev):
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        meta = torch.empty(B + 1 + (B + 1) // 2, dtype=torch.int64, device=dev)        # offsets [B+1] | status [B] int32
        offsets, status = meta[:B + 1], meta[B + 1:].view(torch.int32)[:B]
        encode_jpeg_op(frames, quality, slot, scratch, out, offsets, status, sub)
        meta_host = frame_loop._acquire_pinned(meta.numel() * 8)
        data_host = None
        try:
            meta_host[:meta.numel() * 8].copy_(meta.view(torch.uint8), non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            words = meta_host[:meta.numel() * 8].numpy().view(np.int64)
            off = words[:B + 1].copy()
            st = words[B + 1:].view(np.int32)[:B].copy()
            total = int(off[B])
            if total:
                data_host = frame_loop._acquire_pinned(total)
                data_host[:total].copy_(out[:total], non_blocking=True)
                torch.cuda.current_stream(dev).synchronize()
                data = data_host[:total].numpy()
            files = []
            for i in range(B):
                if st[i] == 0:
                    files.append(data[off[i]:off[i + 1]].tobytes())
                else:                                          # a row outgrew its slot: this frame alone, on the host
                    files.append(encode_jpeg_host(frames[i].cpu().numpy(), quality, sub))
            return files
        finally:
            frame_loop._release_pinned(meta_host)
            if data_host is not None:
                frame_loop._release_pinned(data_host)


# ================================================================================================================ decoding
# Baseline JPEG -> pixels, byte for byte libjpeg's default path (islow IDCT, fancy upsampling, 16-bit fixed-point colour):
# csrc/jpeg_dec.hip on the device, the numpy twin here.  The entropy stage of the device cuts each restart
# segment into subsequences of chunk_bits bits and finds every subsequence's entry state by a fixed-point iteration;
# sync_states() below is the host model of exactly that rule.
DEFAULT_CHUNK_BITS = 2048           # the fastest of 256 / 512 / 1024 / 2048 on 1080p files (tools/jpeg_decode_bench.py)
TAB_BYTES = 384 + 8 + 4 * 832     # the per-frame table block of the device (see _device_tables)
MAX_SUBSEQUENCES = 1 << 17        # per frame: what casync_op_jpegdec_decode admits (the plan's rounds are bounded by this number)
REC_WORDS = 16


class JpegUnsupported(ValueError):
    """The file is outside the subset the decoder reads (parse_jpeg names the reason)"""


class JpegUnreadable(ValueError):
    """decode_jpeg_device: file .index is outside the subset and the host decoder cannot read it either"""

    def __init__(self, index: int, what: str):
        super().__init__(what)
        self.index = int(index)


class JpegCorrupt(ValueError):
    """The scan of a file inside the subset broke a rule; .status is the device's code: 1 invalid code or coefficient overrun,
    2 the scan ended before the last MCU, 3 more data than MCUs in a segment"""

    def __init__(self, status: int, what: str):
        super().__init__(what)
        self.status = int(status)


SUBSETS = ("baseline", "mjpeg")
GRAY = 3                          # JpegInfo.subsampling of a one-component file; 0, 1 and 2 are Pillow's numbers for 4:4:4, 4:2:2 and 4:2:0
# per sampling: the component of each block of an MCU (the slot map), and the MCU's height and width in pixels
SLOT_MAPS = {0: (0, 1, 2), 1: (0, 0, 1, 2), 2: (0, 0, 0, 0, 1, 2), GRAY: (0,)}
MCU_SIZES = {0: (8, 8), 1: (8, 16), 2: (16, 16), GRAY: (8, 8)}


def _subset(subset) -> str:
    if subset not in SUBSETS:
        raise ValueError(f"jpeg: subset {subset!r} is neither 'baseline' nor 'mjpeg'")
    return subset


class JpegInfo:
    """What parse_jpeg reads from the headers.  H, W; subsampling 0 (4:4:4) or 2 (4:2:0), under subset="mjpeg" also 1 (4:2:2) and
    3 (GRAY, one component); qtables: per component int32 [64] in zigzag order; dc_tables / ac_tables: per component (bits[16],
    vals) as the scan selects them; dc_sel / ac_sel: the table ids (0 / 1); restart_interval in MCUs (0: none); scan_offset,
    scan_length: the entropy-coded bytes, markers included; restart_offsets: byte offsets in the file of every RSTn marker."""
    __slots__ = ("H", "W", "subsampling", "qtables", "dc_tables", "ac_tables", "dc_sel", "ac_sel", "restart_interval", "scan_offset",
                 "scan_length", "restart_offsets")

    @property
    def slot_components(self):
        """the component of each block of an MCU, in stream order"""
        return SLOT_MAPS[self.subsampling]

    @property
    def blocks_per_mcu(self) -> int:
        return len(SLOT_MAPS[self.subsampling])

    @property
    def mcu_grid(self):
        """(MCU rows, MCUs per row)"""
        sh, sw = MCU_SIZES[self.subsampling]
        return (self.H + sh - 1) // sh, (self.W + sw - 1) // sw

    def segments(self):
        """[(start, end)] of the restart segments, byte offsets relative to the scan's first byte, markers excluded"""
        cuts = [int(o) - self.scan_offset for o in self.restart_offsets]
        starts = [0] + [c + 2 for c in cuts]
        return list(zip(starts, cuts + [self.scan_length]))

    def expected_segments(self) -> int:
        rows, cols = self.mcu_grid
        n = rows * cols
        return (n + self.restart_interval - 1) // self.restart_interval if self.restart_interval else 1


def _huff_ok(bits, vals) -> bool:
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > (1 << length):
            return False
        code <<= 1
    return sum(bits) == len(vals) and len(vals) <= 256


def parse_jpeg(data, subset: str = "baseline") -> JpegInfo:
    """The headers of a baseline file of the supported subset (SOF0, 8 bits, three components sampled 1x1 or 2x2 / 1x1 / 1x1, one
    interleaved scan, 8-bit quantisation tables, Huffman tables 0 and 1, any restart interval); JpegUnsupported otherwise.
    ``subset="mjpeg"`` admits what Motion-JPEG writers add to that: 2x1 / 1x1 / 1x1 sampling (4:2:2), one component (grayscale:
    a scan of single blocks), and a scan that names a Huffman table no DHT segment defines, which is then the Annex K table of
    its class and id (the ``MJPG`` convention: libjpeg-turbo supplies the same tables)."""
    wide = _subset(subset) == "mjpeg"
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise JpegUnsupported("jpeg: not a JPEG file (no SOI)")
    ended = JpegUnsupported("jpeg: the file ends inside its headers")
    qt, huff, frame, ri, pos, adobe = {}, {}, None, 0, 2, 1
    while True:
        if pos + 4 > n:
            raise ended
        if data[pos] != 0xFF:
            raise JpegUnsupported(f"jpeg: no marker at byte {pos}")
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            pos += 2
            continue
        if m == 0xD9:
            raise ended
        length = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        if length < 2 or pos + 2 + length > n:
            raise ended
        body = data[pos + 4:pos + 2 + length]
        pos += 2 + length
        if m == 0xC0:
            if frame is not None:
                raise JpegUnsupported("jpeg: several frames")
            if len(body) < 6 or len(body) < 6 + 3 * body[5]:
                raise JpegUnsupported("jpeg: a short SOF segment")
            if body[0] != 8:
                raise JpegUnsupported(f"jpeg: {body[0]}-bit samples")
            H, W = struct.unpack(">HH", body[1:5])
            nf = body[5]
            if nf == 1 and not wide:
                raise JpegUnsupported("jpeg: a grayscale file")
            if nf == 4:
                raise JpegUnsupported("jpeg: a four-component (CMYK) file")
            if nf not in (1, 3):
                raise JpegUnsupported(f"jpeg: {nf} components")
            if H < 1 or W < 1:
                raise JpegUnsupported("jpeg: a frame without a size (DNL)")
            comps = [(body[6 + 3 * i], body[7 + 3 * i], body[8 + 3 * i]) for i in range(nf)]
            samp = tuple(c[1] for c in comps)
            if samp == (0x11, 0x11, 0x11):
                sub = 0
            elif samp == (0x22, 0x11, 0x11):
                sub = 2
            elif wide and samp == (0x21, 0x11, 0x11):
                sub = 1
            elif nf == 1 and samp == (0x11,):
                sub = GRAY
            else:
                known = "4:4:4, 4:2:2 and 4:2:0" if wide else "4:4:4 and 4:2:0"
                raise JpegUnsupported(f"jpeg: chroma sampling other than {known} (" + ", ".join(f"{s >> 4}x{s & 15}" for s in samp) + ")")
            frame = (H, W, sub, comps)
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF, 0xCC):
            what = {0xC2: "a progressive file", 0xC1: "an extended sequential file", 0xC3: "a lossless file"}.get(
                m, "arithmetic coding" if m >= 0xC9 else f"frame type SOF{m - 0xC0}")
            raise JpegUnsupported(f"jpeg: {what}")
        elif m == 0xC4:
            at = 0
            while at < len(body):
                if at + 17 > len(body):
                    raise JpegUnsupported("jpeg: a short DHT segment")
                tc, th = body[at] >> 4, body[at] & 15
                bits = tuple(body[at + 1:at + 17])
                vals = bytes(body[at + 17:at + 17 + sum(bits)])
                if tc > 1 or not _huff_ok(bits, vals):
                    raise JpegUnsupported("jpeg: a Huffman table that is no prefix code")
                huff[(tc, th)] = (bits, vals)
                at += 17 + sum(bits)
        elif m == 0xDB:
            at = 0
            while at < len(body):
                pq, tq = body[at] >> 4, body[at] & 15
                if pq:
                    raise JpegUnsupported("jpeg: a 16-bit quantisation table")
                if at + 65 > len(body):
                    raise JpegUnsupported("jpeg: a short DQT segment")
                qt[tq] = np.frombuffer(body[at + 1:at + 65], dtype=np.uint8).astype(np.int32)
                at += 65
        elif m == 0xDD:
            if len(body) < 2:
                raise JpegUnsupported("jpeg: a short DRI segment")
            ri = struct.unpack(">H", body[:2])[0]
        elif m == 0xEE:
            if body[:5] == b"Adobe" and len(body) >= 12:
                adobe = body[11]                                 # judged at the scan: a CMYK file is named as that
        elif m == 0xDA:
            if frame is None:
                raise JpegUnsupported("jpeg: a scan ahead of the frame header")
            H, W, sub, comps = frame
            nf = len(comps)
            if adobe != 1 and nf == 3:
                raise JpegUnsupported(f"jpeg: Adobe colour transform {adobe}, not YCbCr")
            if len(body) < 1 or body[0] != nf or len(body) < 4 + 2 * nf:
                raise JpegUnsupported("jpeg: a scan that does not interleave the three components (several scans)" if nf == 3 else
                                      "jpeg: a scan that does not hold the file's one component")
            sel = [(body[1 + 2 * i], body[2 + 2 * i]) for i in range(nf)]
            if [s[0] for s in sel] != [c[0] for c in comps]:
                raise JpegUnsupported("jpeg: scan components out of frame order")
            if tuple(body[1 + 2 * nf:4 + 2 * nf]) != (0, 63, 0):
                raise JpegUnsupported("jpeg: a scan with spectral selection or successive approximation")
            break
        # every other segment (APPn, COM, ...) is skipped
    info = JpegInfo()
    info.H, info.W, info.subsampling = H, W, sub
    info.dc_sel, info.ac_sel = tuple(s[1] >> 4 for s in sel), tuple(s[1] & 15 for s in sel)
    if max(info.dc_sel + info.ac_sel) > 1:
        raise JpegUnsupported("jpeg: a Huffman table id above 1")
    if wide:                                                     # a table the scan names and no DHT defines is Annex K's of that class and id
        for key, table in (((0, 0), DC_LUMA), ((1, 0), AC_LUMA), ((0, 1), DC_CHROMA), ((1, 1), AC_CHROMA)):
            huff.setdefault(key, (tuple(table[0]), bytes(table[1])))
    try:
        info.qtables = [qt[c[2]] for c in comps]
        info.dc_tables = [huff[(0, t)] for t in info.dc_sel]
        info.ac_tables = [huff[(1, t)] for t in info.ac_sel]
    except KeyError as exc:
        raise JpegUnsupported(f"jpeg: the scan names a table the file does not define ({exc.args[0]})") from None
    info.restart_interval = int(ri)
    info.scan_offset = pos
    scan = np.frombuffer(data, dtype=np.uint8, offset=pos)
    ff = np.nonzero(scan[:-1] == 0xFF)[0] if scan.size > 1 else np.zeros(0, dtype=np.int64)
    nxt = scan[ff + 1]
    rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    other = ff[(nxt != 0) & ~rst]
    end = int(other[0]) if other.size else int(scan.size)          # no marker behind the scan: it runs to the end of the file
    if other.size and b"\xff\xda" in data[pos + end:]:
        raise JpegUnsupported("jpeg: several scans")
    info.scan_length = end
    marks = ff[rst]
    info.restart_offsets = (marks[marks < end] + pos).astype(np.int64)
    return info


def _lut16(bits, vals) -> np.ndarray:
    """the next 16 bits -> length << 8 | symbol (0: no code)"""
    lut = np.zeros(65536, dtype=np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lo = code << (16 - length)
            lut[lo:lo + (1 << (16 - length))] = (length << 8) | vals[k]
            code += 1
            k += 1
        code <<= 1
    return lut


class _Segment:
    """One restart segment, unstuffed, with the maps between bit positions of the stuffed stream (relative to the scan's first
    byte; byte k of a segment is stuffing iff it is 0x00 behind 0xFF, a position never lies in one; bytes past the segment's end
    read as zero) and of the unstuffed one."""

    def __init__(self, scan: bytes, start: int, end: int):
        sb = scan[start:end]
        a = np.frombuffer(sb, dtype=np.uint8)
        stuff = np.zeros(a.size, dtype=bool)
        if a.size > 1:
            stuff[1:] = (a[1:] == 0) & (a[:-1] == 0xFF)
        self.start, self.n_s = start, a.size
        self.stuff = stuff
        self.didx = np.nonzero(~stuff)[0]
        self.cum = np.cumsum(~stuff) - 1
        self.n_u = int(self.didx.size)
        self.u = a[~stuff].tobytes() + b"\0" * 16
        self.end_bits = end * 8

    def to_u(self, p: int) -> int:
        p -= self.start * 8
        k, o = p >> 3, p & 7
        if k < self.n_s and self.stuff[k]:
            k, o = k + 1, 0
        if k >= self.n_s:
            return (self.n_u + k - self.n_s) * 8 + o
        return int(self.cum[k]) * 8 + o

    def to_s(self, q: int) -> int:
        k, o = q >> 3, q & 7
        k = self.n_s + k - self.n_u if k >= self.n_u else int(self.didx[k])
        return (self.start + k) * 8 + o


class _Scan:
    """The tables of a file's scan in the form the symbol loop wants"""

    def __init__(self, info: JpegInfo, data: bytes):
        self.info = info
        self.scan = bytes(data[info.scan_offset:info.scan_offset + info.scan_length])
        self.bpm = info.blocks_per_mcu
        self.comp = info.slot_components
        self.dc = [_lut16(*t).tolist() for t in info.dc_tables]
        self.ac = [_lut16(*t).tolist() for t in info.ac_tables]
        rows, cols = info.mcu_grid
        self.n_mcu = rows * cols
        self.ri = info.restart_interval or self.n_mcu
        self.segs = info.segments()

    def seg_blocks(self, j: int) -> int:
        """blocks the geometry gives segment j"""
        return max(0, min(self.ri, self.n_mcu - j * self.ri)) * self.bpm

    def run(self, seg: _Segment, q: int, s: int, z: int, end_q: int, out=None, block0: int = 0, cap: int = 0, pred=None):
        """Decode the symbols that start at unstuffed bit positions q <= .. < end_q from state (slot s, zigzag index z).
        -> (q, s, z, blocks finished, blocks finished ahead of an invalid code or -1, DC difference sums [3]).  out
        [blocks, 64] (zigzag order) takes the coefficients of blocks block0 + 0 .. below block0 + cap, DC as values from pred."""
        u, bpm, comp = seg.u, self.bpm, self.comp
        n, dcs = 0, [0, 0, 0]
        while q < end_q:
            k, o = q >> 3, q & 7
            w = (int.from_bytes(u[k:k + 5], "big") >> (8 - o)) & 0xFFFFFFFF
            c = comp[s]
            done = False
            if z == 0:
                e = self.dc[c][w >> 16]
                ln, cat = e >> 8, e & 0xFF
                if ln == 0 or cat > 11:
                    return -1, 0, 0, n, n, dcs
                v = 0
                if cat:
                    v = (w >> (32 - ln - cat)) & ((1 << cat) - 1)
                    if v < (1 << (cat - 1)):
                        v -= (1 << cat) - 1
                dcs[c] += v
                if out is not None and n < cap:
                    pred[c] += v
                    out[block0 + n, 0] = pred[c]
                z = 1
                q += ln + cat
            else:
                e = self.ac[c][w >> 16]
                ln, sym = e >> 8, e & 0xFF
                if ln == 0:
                    return -1, 0, 0, n, n, dcs
                r, cat = sym >> 4, sym & 15
                if cat == 0:
                    if r == 15:
                        z += 16
                        if z > 64:
                            return -1, 0, 0, n, n, dcs
                        done = z == 64
                    else:
                        done = True
                else:
                    z += r
                    if z > 63:
                        return -1, 0, 0, n, n, dcs
                    v = (w >> (32 - ln - cat)) & ((1 << cat) - 1)
                    if v < (1 << (cat - 1)):
                        v -= (1 << cat) - 1
                    if out is not None and n < cap:
                        out[block0 + n, z] = v
                    z += 1
                    done = z == 64
                q += ln + cat
            if done:
                z, s, n = 0, (s + 1) % bpm, n + 1
        return q, s, z, n, -1, dcs


def _segment_status(n: int, err_n: int, want: int) -> int:
    if 0 <= err_n < want:
        return 1
    return 2 if n < want else 3 if n > want else 0


def _decode_scan(info: JpegInfo, data: bytes):
    """(coefficients [blocks, 64] int32 in zigzag order, stream order, DC as values; status)"""
    sc = _Scan(info, data)
    coef = np.zeros((sc.n_mcu * sc.bpm, 64), dtype=np.int32)
    if len(sc.segs) != info.expected_segments():
        return coef, 2 if len(sc.segs) < info.expected_segments() else 3
    status = 0
    for j, (a, b) in enumerate(sc.segs):
        seg = _Segment(sc.scan, a, b)
        want = sc.seg_blocks(j)
        _, _, _, n, err_n, _ = sc.run(seg, 0, 0, 0, seg.n_u * 8, coef, j * sc.ri * sc.bpm, want, [0, 0, 0])
        if status == 0:
            status = _segment_status(n, err_n, want)
    return coef, status


def scan_status(data, subset: str = "baseline") -> int:
    """The status the device gives a file of the subset: 0, or the code of the first restart segment that breaks a rule"""
    return _decode_scan(parse_jpeg(data, subset), bytes(data))[1]


def _idct_pass(c, shift: int):
    """One pass of libjpeg's accurate integer inverse DCT (jidctint) along the last axis of c [..., 8] (int64)"""
    z1 = (c[..., 2] + c[..., 6]) * 4433
    t2, t3 = z1 - c[..., 6] * 15137, z1 + c[..., 2] * 6270
    t0, t1 = (c[..., 0] + c[..., 4]) << 13, (c[..., 0] - c[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c[..., 7], c[..., 5], c[..., 3], c[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.empty_like(c)
    for i, v in enumerate((t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3)):
        out[..., i] = _descale(v, shift)
    return out


def _idct_blocks(coef_zz: np.ndarray, q_zz: np.ndarray) -> np.ndarray:
    """[n, 64] coefficients and [64] table, both in zigzag order -> [n, 8, 8] samples 0..255"""
    nat = np.zeros(coef_zz.shape, dtype=np.int64)
    nat[:, list(ZIGZAG)] = coef_zz.astype(np.int64) * q_zz.astype(np.int64)
    b = nat.reshape(-1, 8, 8)
    b = _idct_pass(np.ascontiguousarray(b.swapaxes(-1, -2)), 11).swapaxes(-1, -2)      # columns first
    b = _idct_pass(np.ascontiguousarray(b), 18)                                          # then rows
    return np.clip(b + 128, 0, 255)


def _upsample_h2v2(c: np.ndarray, H: int, W: int) -> np.ndarray:
    """libjpeg's h2v2_fancy_upsample of the real downsampled plane c [ceil(H/2), ceil(W/2)] -> [H, W]"""
    ch, cw = c.shape
    near = np.repeat(np.arange(ch), 2)
    far = np.clip(near + np.where(np.arange(2 * ch) % 2, 1, -1), 0, ch - 1)
    s = 3 * c[near] + c[far]                                                             # [2 ch, cw]
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out[:H, :W]


def _upsample_h2v1(c: np.ndarray, W: int) -> np.ndarray:
    """libjpeg's h2v1_fancy_upsample of the real downsampled plane c [H, ceil(W/2)] -> [H, W]: the triangle filter along the row,
    the first and the last column copied (what repeating the edge column gives under this rounding), no vertical filter"""
    left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out = np.empty((c.shape[0], 2 * c.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    return out[:, :W]


def _pixels(info: JpegInfo, coef: np.ndarray) -> np.ndarray:
    """coefficients [blocks, 64] (zigzag order, stream order) -> BGR uint8 [H, W, 3]"""
    H, W = info.H, info.W
    rows, cols = info.mcu_grid
    bpm = info.blocks_per_mcu
    coef = coef.reshape(rows, cols, bpm, 64)
    if info.subsampling == GRAY:                                 # the Y plane is B, G and R
        y = _idct_blocks(coef[:, :, 0].reshape(-1, 64), info.qtables[0]).reshape(rows, cols, 8, 8)
        y = y.transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)[:H, :W]
        return np.ascontiguousarray(np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8))
    if info.subsampling == 1:                                    # 4:2:2: an MCU of 16 x 8 pixels, slots (Y, Y, Cb, Cr)
        y = _idct_blocks(coef[:, :, :2].reshape(-1, 64), info.qtables[0]).reshape(rows, cols, 2, 8, 8)
        planes = [y.transpose(0, 3, 1, 2, 4).reshape(rows * 8, cols * 16)[:H, :W]]
        for c in (1, 2):
            p = _idct_blocks(coef[:, :, 1 + c].reshape(-1, 64), info.qtables[c]).reshape(rows, cols, 8, 8)
            planes.append(_upsample_h2v1(p.transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)[:H, :(W + 1) // 2], W))
    elif info.subsampling:
        y = _idct_blocks(coef[:, :, :4].reshape(-1, 64), info.qtables[0]).reshape(rows, cols, 2, 2, 8, 8)
        y = y.transpose(0, 2, 4, 1, 3, 5).reshape(rows * 16, cols * 16)[:H, :W]
        planes = [y]
        for c in (1, 2):
            p = _idct_blocks(coef[:, :, 3 + c].reshape(-1, 64), info.qtables[c]).reshape(rows, cols, 8, 8)
            p = p.transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)[:(H + 1) // 2, :(W + 1) // 2]
            planes.append(_upsample_h2v2(p, H, W))
    else:
        planes = []
        for c in range(3):
            p = _idct_blocks(coef[:, :, c].reshape(-1, 64), info.qtables[c]).reshape(rows, cols, 8, 8)
            planes.append(p.transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)[:H, :W])
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def decode_jpeg_host(data, subset: str = "baseline") -> np.ndarray:
    """A baseline JPEG file of the subset -> BGR uint8 [H, W, 3], the numpy twin of the device decoder: the bytes of Pillow's
    ``Image.open(...).convert("RGB")``, reversed to BGR.  JpegUnsupported for a file outside the subset (``subset="mjpeg"``: the
    wider one of parse_jpeg), JpegCorrupt (with the device's status code) for a scan that breaks a rule."""
    data = bytes(data)
    info = parse_jpeg(data, subset)
    coef, status = _decode_scan(info, data)
    if status:
        raise JpegCorrupt(status, f"jpeg: the scan is damaged (status {status})")
    return _pixels(info, coef)


def _chunk_bits(chunk_bits: int) -> int:
    c = int(chunk_bits) or DEFAULT_CHUNK_BITS
    if c < 32 or c % 32 or c > (1 << 30):
        raise ValueError(f"jpeg: chunk_bits {chunk_bits} is not a multiple of 32 in 32..2^30")
    return c


def _subsequences(segs, chunk: int):
    """subsequences of each segment [(start, end)] (bytes): max(1, ceil(bits / chunk))"""
    return [max(1, -(-(b - a) * 8 // chunk)) for a, b in segs]


class SyncResult:
    """states [S, 3] int64: the entry state (bit position in the stuffed scan, block slot of the MCU, zigzag index) of every
    subsequence, segment after segment; segment [S]; rounds [S]: the round after which the state last changed (0: it was known or
    guessed right); total_rounds: decoding rounds run"""
    __slots__ = ("states", "segment", "rounds", "total_rounds")


def _boundaries(sc: _Scan, chunk: int):
    """(segment objects, [(segment index, k, end bit)] per subsequence)"""
    segs = [_Segment(sc.scan, a, b) for a, b in sc.segs]
    subs = []
    for j, (n, seg) in enumerate(zip(_subsequences(sc.segs, chunk), segs)):
        for k in range(n):
            end = seg.end_bits if k == n - 1 else min(seg.start * 8 + (k + 1) * chunk, seg.end_bits)
            subs.append((j, k, end))
    return segs, subs


def sync_states(info: JpegInfo, data, chunk_bits: int = 0) -> SyncResult:
    """The host model of the device's entropy plan.  Every restart segment is cut into subsequences of chunk_bits bits of the
    stuffed stream.  The first of a segment starts in the known state, every other from the guess (its first bit, slot 0, zigzag
    0).  A round decodes every subsequence whose entry state changed; the exit state of one is the entry state of the next.  The
    rounds end when no entry state changes: subsequence k of a segment is right after at most k rounds.  A subsequence that meets
    an invalid code hands the guess to the next one, so a wrong guess that runs into one does not spoil what follows it (the
    frame's status comes from the first invalid code of a segment, which no later state changes)."""
    chunk = _chunk_bits(chunk_bits)
    sc = _Scan(info, bytes(data))
    segs, subs = _boundaries(sc, chunk)
    S = len(subs)
    entry = []
    for j, k, _ in subs:
        seg = segs[j]
        entry.append((seg.to_s(seg.to_u(min(seg.start * 8 + k * chunk, seg.end_bits))), 0, 0))     # to_s(to_u()) steps over a stuffed byte
    exits = [None] * S
    rounds = [0] * S
    changed = list(range(S))
    total = 0
    while changed:
        total += 1
        for g in changed:
            j, k, end = subs[g]
            p, s, z = entry[g]
            seg = segs[j]
            q, s, z, _, _, _ = sc.run(seg, seg.to_u(p), s, z, seg.to_u(end))
            exits[g] = (seg.to_s(seg.to_u(end)), 0, 0) if q < 0 else (seg.to_s(q), s, z)
        nxt = []
        for g in changed:
            if g + 1 < S and subs[g + 1][0] == subs[g][0] and entry[g + 1] != exits[g]:
                entry[g + 1] = exits[g]
                rounds[g + 1] = total
                nxt.append(g + 1)
        changed = nxt
    res = SyncResult()
    res.states = np.asarray(entry, dtype=np.int64).reshape(S, 3)
    res.segment = np.asarray([j for j, _, _ in subs], dtype=np.int64)
    res.rounds = np.asarray(rounds, dtype=np.int64)
    res.total_rounds = total
    return res


def serial_states(info: JpegInfo, data, chunk_bits: int = 0) -> np.ndarray:
    """[S, 3]: the state of a plain serial decoder where it crosses into each subsequence of sync_states' cut (behind an invalid
    code it goes on from the next boundary's guess)"""
    chunk = _chunk_bits(chunk_bits)
    sc = _Scan(info, bytes(data))
    segs, subs = _boundaries(sc, chunk)
    out, state = [], None
    for j, k, end in subs:
        seg = segs[j]
        if k == 0:
            state = (seg.start * 8, 0, 0)
        out.append(state)
        q, s, z, _, _, _ = sc.run(seg, seg.to_u(state[0]), state[1], state[2], seg.to_u(end))
        state = (seg.to_s(seg.to_u(end)), 0, 0) if q < 0 else (seg.to_s(q), s, z)
    return np.asarray(out, dtype=np.int64).reshape(len(subs), 3)


# ---------------------------------------------------------------------------------------------------------------- device
def _device_huffman(bits, vals) -> bytes:
    """832 bytes: lut [256] u16 (length << 8 | symbol for codes of up to 8 bits) | maxcode [8] int32 of lengths 9..16 (-1: none) |
    valoff [8] int32 (index of the length's first symbol minus its first code) | the symbols, padded to 256"""
    lut = np.zeros(256, dtype=np.uint16)
    maxcode = np.full(8, -1, dtype=np.int32)
    valoff = np.zeros(8, dtype=np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        n = bits[length - 1]
        if n and length <= 8:
            for i in range(n):
                lo = (code + i) << (8 - length)
                lut[lo:lo + (1 << (8 - length))] = (length << 8) | vals[k + i]
        elif n:
            maxcode[length - 9] = code + n - 1
            valoff[length - 9] = k - code
        code = (code + n) << 1
        k += n
    return lut.tobytes() + maxcode.tobytes() + valoff.tobytes() + bytes(vals) + b"\0" * (256 - len(vals))


def _device_tables(info: JpegInfo) -> bytes:
    """The table block of one frame, TAB_BYTES: quantisation [3][64] u16 in natural order | the DC table (0 / 1) of each component,
    0 | the AC table of each, 0 | the Huffman tables DC 0, DC 1, AC 0, AC 1 (zeros where the file has none)"""
    q = np.zeros((3, 64), dtype=np.uint16)
    for c in range(len(info.qtables)):                           # a grayscale file fills component 0 alone
        q[c, list(ZIGZAG)] = info.qtables[c]
    out = q.tobytes() + bytes(info.dc_sel).ljust(4, b"\0") + bytes(info.ac_sel).ljust(4, b"\0")
    for cls, sel, tables in ((0, info.dc_sel, info.dc_tables), (1, info.ac_sel, info.ac_tables)):
        for t in (0, 1):
            out += _device_huffman(*tables[sel.index(t)]) if t in sel else b"\0" * 832
    assert len(out) == TAB_BYTES
    return out


class DecodePlan:
    """What casync_op_jpegdec_decode wants for a batch of files: blob (uint8: each file's scan, segment list and table block,
    4-byte aligned), rec (int32 [B, 16], see include/casync_hip.h), infos (JpegInfo, or the JpegUnsupported of a file outside the
    subset, whose record carries status 1 and nothing else), total_sub, subsampling (2: every file is 4:2:0, else 0), subset
    ("mjpeg": the records are casync_op_mjpegdec_decode's, whose sampling word also takes 1, 4:2:2, and 3, grayscale)"""
    __slots__ = ("blob", "rec", "infos", "total_sub", "subsampling", "H", "W", "chunk_bits", "subset")


def plan_decode(files, chunk_bits: int = 0, subset: str = "baseline") -> DecodePlan:
    chunk = _chunk_bits(chunk_bits)
    plan = DecodePlan()
    plan.subset = _subset(subset)
    plan.chunk_bits = chunk
    plan.infos = []
    parts, at, total = [], 0, 0
    rec = np.zeros((len(files), REC_WORDS), dtype=np.int32)

    def put(b: bytes) -> int:
        nonlocal at
        off = at
        b += b"\0" * (-len(b) % 4)
        parts.append(b)
        at += len(b)
        return off

    for i, data in enumerate(files):
        data = bytes(data)
        rec[i, 8] = total
        try:
            info = parse_jpeg(data, subset)
            if info.scan_length >= 1 << 27:
                raise JpegUnsupported("jpeg: a scan of 128 MiB or more")
        except JpegUnsupported as exc:
            plan.infos.append(exc)
            rec[i, 9] = 1
            continue
        plan.infos.append(info)
        segs = info.segments()
        want = info.expected_segments()
        rec[i, 2], rec[i, 3] = info.subsampling, info.restart_interval
        if len(segs) != want:                                    # the host's call: the device gets no work for this frame
            rec[i, 9] = 2 if len(segs) < want else 3
            continue
        nsub = _subsequences(segs, chunk)
        if sum(nsub) > MAX_SUBSEQUENCES:                         # the host path: the device bounds its rounds by this count
            plan.infos[-1] = JpegUnsupported(f"jpeg: {sum(nsub)} subsequences of {chunk} bits, the device takes {MAX_SUBSEQUENCES} a frame")
            rec[i, 2], rec[i, 3], rec[i, 9] = 0, 0, 1
            continue
        first = np.concatenate([[0], np.cumsum(nsub)]).astype(np.int32)
        rec[i, 0] = put(data[info.scan_offset:info.scan_offset + info.scan_length])
        rec[i, 1] = info.scan_length
        rec[i, 4] = len(segs)
        rec[i, 5] = put(np.asarray([a for a, _ in segs] + [b for _, b in segs], dtype=np.int32).tobytes() + first.tobytes())
        rec[i, 6] = put(_device_tables(info))
        rec[i, 7] = int(first[-1])
        total += int(first[-1])
    plan.blob = np.frombuffer(b"".join(parts) or b"\0\0\0\0", dtype=np.uint8)
    plan.rec, plan.total_sub = rec, total
    good = [x for x in plan.infos if isinstance(x, JpegInfo)]
    plan.subsampling = 2 if good and all(x.subsampling == 2 for x in good) else 0
    sizes = {(x.H, x.W) for x in good}
    plan.H, plan.W = next(iter(sizes)) if len(sizes) == 1 else (0, 0)
    return plan


def decode_jpeg_op(plan: DecodePlan, data, scratch, out, status, H: int = 0, W: int = 0) -> None:
    """casync_op_jpegdec_decode (casync_op_mjpegdec_decode for a plan of subset "mjpeg") on torch's current stream, every buffer
    the caller's (uint8 data holding plan.blob, uint8 scratch, uint8 out [B,H,W,3], int32 status [B]); nothing is waited for."""
    import torch
    from . import _lib
    if plan.subset == "mjpeg":
        _lib.check(_lib.load().casync_op_mjpegdec_decode(data.data_ptr(), data.numel(), plan.rec.ctypes.data, plan.rec.shape[0], H or plan.H,
                                                         W or plan.W, plan.chunk_bits, scratch.data_ptr(), scratch.numel(), out.data_ptr(),
                                                         status.data_ptr(), torch.cuda.current_stream(out.device).cuda_stream),
                   "casync_op_mjpegdec_decode")
        return
    _lib.check(_lib.load().casync_op_jpegdec_decode(data.data_ptr(), data.numel(), plan.rec.ctypes.data, plan.rec.shape[0], H or plan.H, W or plan.W,
                                                    plan.subsampling, plan.chunk_bits, scratch.data_ptr(), scratch.numel(), out.data_ptr(),
                                                    status.data_ptr(), torch.cuda.current_stream(out.device).cuda_stream), "casync_op_jpegdec_decode")


def _decode_pillow(data) -> np.ndarray:
    """BGR uint8 [H,W,3] of any file Pillow reads: the host path of a file outside the subset, as frame_synth._imread decodes"""
    import io
    from PIL import Image
    with Image.open(io.BytesIO(bytes(data))) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def workspace_bytes(plan: DecodePlan, B: int, H: int, W: int) -> int:
    """the scratch the plan's entry wants for B frames of H x W (the entry's own error where it refuses the arguments)"""
    from . import _lib
    lib = _lib.load()
    if plan.subset == "mjpeg":
        entry, need = "casync_op_mjpegdec_workspace_bytes", lib.casync_op_mjpegdec_workspace_bytes(B, H, W, plan.total_sub)
    else:
        entry, need = "casync_op_jpegdec_workspace_bytes", lib.casync_op_jpegdec_workspace_bytes(B, H, W, plan.subsampling, plan.total_sub)
    if need < 0:
        _lib.check(int(need), entry)
    return int(need)


def decode_jpeg_device(files, *, device="cuda:0", chunk_bits: int = 0, fallback: str = "host", out=None, subset: str = "baseline"):
    """A sequence of JPEG files (bytes) of one size -> uint8 [B,H,W,3] BGR on the device, decoded there (csrc/jpeg_dec.hip): the
    compressed bytes go up in one pinned copy, and what comes back is the B status words.  A file outside the subset
    (parse_jpeg), or one whose device status is non-zero, is decoded on the host with Pillow and uploaded into its slot; with
    ``fallback="raise"`` it raises instead, naming the file's index.  ``chunk_bits`` (0: the default, 2048) is the length of the
    subsequences the entropy stage cuts a scan into.  ``out``: a contiguous uint8 [B,H,W,3] device tensor to decode into.
    ``subset="mjpeg"`` sends the whole batch through the wider decoder (csrc/jpeg_dec_mjpeg.hip): 4:2:2 and grayscale files and
    files without their Huffman tables are decoded on the device as well, and one batch may mix all four samplings."""
    import torch
    _subset(subset)
    if fallback not in ("host", "raise"):
        raise ValueError(f"decode_jpeg_device: fallback {fallback!r} is neither 'host' nor 'raise'")
    files = [bytes(f) for f in files]
    dev = torch.device(device) if out is None else out.device
    if dev.type != "cuda":
        raise RuntimeError("decode_jpeg_device needs a ROCm device (decode_jpeg_host is the host decoder)")
    plan = plan_decode(files, chunk_bits, subset)
    B = len(files)
    if B == 0:
        return torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=dev) if out is None else out
    host = {}                                                    # index -> pixels decoded on the host
    for i, info in enumerate(plan.infos):
        if not isinstance(info, JpegInfo):
            if fallback == "raise":
                raise JpegUnsupported(f"decode_jpeg_device: file {i}: {info}")
            try:
                host[i] = _decode_pillow(files[i])
            except Exception as exc:
                raise JpegUnreadable(i, f"decode_jpeg_device: cannot read file {i}: {info}; Pillow: {exc}") from exc
    sizes = {(x.H, x.W) for x in plan.infos if isinstance(x, JpegInfo)} | {v.shape[:2] for v in host.values()}
    if len(sizes) != 1:
        raise ValueError(f"decode_jpeg_device: the files must have one size, got {sorted(sizes)} (h x w)")
    H, W = (int(v) for v in next(iter(sizes)))
    if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != (B, H, W, 3) or not out.is_contiguous()):
        raise ValueError(f"decode_jpeg_device: out must be a contiguous uint8 {(B, H, W, 3)} tensor, got {tuple(out.shape)} {out.dtype}")
    from . import frame_loop
    need = workspace_bytes(plan, B, H, W)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        stage = frame_loop._acquire_pinned(plan.blob.size)
        status_host = frame_loop._acquire_pinned(4 * B)
        try:
            stage[:plan.blob.size].numpy()[:] = plan.blob
            data = torch.empty(plan.blob.size, dtype=torch.uint8, device=dev)
            data.copy_(stage[:plan.blob.size], non_blocking=True)
            scratch = torch.empty(max(int(need), 16), dtype=torch.uint8, device=dev)
            status = torch.empty(B, dtype=torch.int32, device=dev)
            decode_jpeg_op(plan, data, scratch, out, status, H, W)
            status_host[:4 * B].copy_(status.view(torch.uint8), non_blocking=True)
            stream.synchronize()
            st = status_host[:4 * B].numpy().view(np.int32).copy()
        finally:
            frame_loop._release_pinned(stage)
            frame_loop._release_pinned(status_host)
        for i in range(B):
            if st[i] and i not in host:
                if fallback == "raise":
                    raise JpegCorrupt(int(st[i]), f"decode_jpeg_device: file {i}: the scan is damaged (status {int(st[i])})")
                try:
                    host[i] = _decode_pillow(files[i])
                except Exception as exc:
                    raise JpegCorrupt(int(st[i]), f"decode_jpeg_device: file {i}: status {int(st[i])} on the device, and Pillow cannot read it "
                                      f"either ({exc})") from exc
                if host[i].shape != (H, W, 3):
                    raise ValueError(f"decode_jpeg_device: file {i} decodes to {host[i].shape}, the batch is {(H, W, 3)}")
        for i, px in host.items():
            out[i].copy_(torch.from_numpy(px))
    return out
