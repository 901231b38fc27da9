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
a frame whose row outgrew its scratch slot, the subject of the CPU tests and the yardstick for inputs without a fixture."""
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
