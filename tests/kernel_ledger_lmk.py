"""The ledger of calipsync_amd/lib/obj_lmk/ (the kernels of the PFLD landmark handle, csrc/landmark.hip), under the rule of
tests/kernel_ledger.py: every compiled kernel instance has op-level cases that launch it through its C-ABI entry with the
launch log on and hold it to a float64 reference.  The channel widths are the network's (they are what is instantiated);
the spatial sizes break the tiling: not square, not a multiple of the 6 x 6 (ghost) or 8 x 8 (stem) tile, odd.

Bars, from tests/kernel_ledger.py's fp32 ops of the same kind:
  * ghost module (1x1 conv + depthwise 3x3 in one kernel) = pw_dw: max|d| <= 3e-6 max|ref|;
  * stride-2 depthwise = dw3x3: 2e-6 max|ref|;
  * stem (dense 3x3 conv, then depthwise) = conv3x3: 3e-6 max|ref|;
  * kinds without a bar there -- the per-tile channel sums and the head (means, conv7, conv8, conv_out) -- take 4 x the
    error of the same op in float32 torch against float64 on the case's own data (_bar4).
Every output goes into a sentinel-filled buffer: with a wider leading dimension where the entry has one, between sentinel
rows otherwise.  Nothing here touches a GPU at import.
"""
from __future__ import annotations

from kernel_ledger import (C, _abs, _dev, _done, _gen, _lib, _ok, _p, _rel, _Run, _s, _sentinel, _t)


def _bar4(f32, f64):
    """4 x max|float32 torch - float64| of the same op on the case's data"""
    return 4.0 * float((f32.double() - f64).abs().max())


def _scaled(err, bar, main_bar):
    """an error held to `bar`, expressed against the case's main bar"""
    return err / bar * main_bar if bar > 0 else (0.0 if err == 0 else float("inf"))


def _padded(a, rows, cols):
    z = _t().zeros(rows, cols)
    z[:a.shape[0], :a.shape[1]] = a
    return z


def _ceil(v, m):
    return (v + m - 1) // m * m


def _tile_sums(x, tile):
    """[B,C,H,W] -> [B, tiles, C] sums over tile x tile blocks (row-major tiles, partial ones at the edges)"""
    torch = _t()
    b, c, h, w = x.shape
    xp = torch.nn.functional.pad(x, (0, _ceil(w, tile) - w, 0, _ceil(h, tile) - h))
    t = xp.reshape(b, c, xp.shape[2] // tile, tile, xp.shape[3] // tile, tile).sum((3, 5))
    return t.permute(0, 2, 3, 1).reshape(b, -1, c)


# ------------------------------------------------------------------ ghost module
def ghost(act, b, h, w, cin, half, sums):
    """casync_op_pfld_ghost vs float64: in a column slice of wider rows with NaN beside it (the padded weight rows are
    zero, and 0 x NaN is NaN), out a column slice of a sentinel-filled buffer;
    sums: the per-tile channel sums too."""
    torch = _t()
    F = torch.nn.functional
    g = _gen("ghost", act, b, h, w, cin, half, sums)
    d = _dev()
    x = torch.randn(b, cin, h, w, generator=g)
    wp = torch.randn(half, cin, generator=g) / cin ** 0.5
    bp = torch.randn(half, generator=g) * 0.3
    wd = torch.randn(half, 1, 3, 3, generator=g) / 3
    bd = torch.randn(half, generator=g) * 0.3

    def op(dt):
        a = (lambda v: F.relu(v)) if act else (lambda v: v)
        x1 = a(F.conv2d(x.to(dt), wp.to(dt)[:, :, None, None], bp.to(dt)))
        return torch.cat([x1, a(F.conv2d(x1, wd.to(dt), bd.to(dt), 1, 1, 1, half))], 1)

    ref = op(torch.float64)
    npad = _ceil(half, 16)
    wpp = _padded(wp.T, _ceil(cin, 16), npad).to(d)
    bpp, bdp = _padded(bp[None], 1, npad).to(d), _padded(bd[None], 1, npad).to(d)
    wdp = _padded(wd.reshape(half, 9).T, 9, npad).to(d)
    ld_in, ld_out = cin + 8, 2 * half + 12
    xin = torch.full((b, h, w, ld_in), float("nan"), device=d)   # a read past cin (widths that are no multiple of 16) shows
    xin[..., 8:] = x.permute(0, 2, 3, 1)
    out = torch.full((b, h, w, ld_out), -7.0, device=d)
    tiles = -(-h // 6) * -(-w // 6)
    sm = torch.full((b * tiles + 2, 2 * half), -7.0, device=d) if sums else None
    with _Run(0) as r:
        _ok(_lib().casync_op_pfld_ghost(xin.data_ptr() + 32, ld_in, _p(wpp), _p(bpp), _p(wdp), _p(bdp), out.data_ptr() + 16, ld_out,
                                        sm.data_ptr() + 2 * half * 4 if sums else 0, b, h, w, cin, half, act, _s()), "pfld_ghost")
    err = max(_rel(out[..., 4:4 + 2 * half], ref.permute(0, 2, 3, 1)), _sentinel(out, 4, 4 + 2 * half, -7.0))
    if sums:
        want = _tile_sums(ref, 6).reshape(b * tiles, 2 * half)
        bar = _bar4(_tile_sums(op(torch.float32), 6).reshape(b * tiles, 2 * half), want)
        err = max(err, _scaled(_abs(sm[1:-1], want), bar, 3e-6))
        if not bool((sm[0] == -7.0).all() and (sm[-1] == -7.0).all()):
            err = float("inf")
    return _done(r, err, 3e-6, f"pfld ghost act={act} {b}x{h}x{w} {cin}->2x{half} sums={sums}")


# ------------------------------------------------------------------ stride-2 depthwise
def dw_s2(b, h, w, c):
    """casync_op_pfld_dw_s2 (linear, pad 1, odd sizes allowed) vs float64, out a column slice of a sentinel-filled buffer"""
    torch = _t()
    F = torch.nn.functional
    g = _gen("dw_s2", b, h, w, c)
    d = _dev()
    x = torch.randn(b, c, h, w, generator=g)
    wd = torch.randn(c, 1, 3, 3, generator=g) / 3
    bd = torch.randn(c, generator=g) * 0.3
    ref = F.conv2d(x.double(), wd.double(), bd.double(), 2, 1, 1, c).permute(0, 2, 3, 1)
    ho, wo = ref.shape[1], ref.shape[2]
    assert (ho, wo) == ((h - 1) // 2 + 1, (w - 1) // 2 + 1)
    xin = x.permute(0, 2, 3, 1).contiguous().to(d)
    wdp, bdd = wd.reshape(c, 9).T.contiguous().to(d), bd.to(d)
    ld = c + 8
    out = torch.full((b, ho, wo, ld), -7.0, device=d)
    with _Run(0) as r:
        _ok(_lib().casync_op_pfld_dw_s2(_p(xin), _p(wdp), _p(bdd), out.data_ptr() + 16, ld, b, h, w, c, _s()), "pfld_dw_s2")
    err = max(_rel(out[..., 4:4 + c], ref), _sentinel(out, 4, 4 + c, -7.0))
    return _done(r, err, 2e-6, f"pfld dw_s2 {b}x{h}x{w}x{c}")


# ------------------------------------------------------------------ stem
def stem(u8, b, h, w):
    """casync_op_pfld_stem on an h x w input (float NCHW, or uint8 HWC divided by 255 on the device) vs float64: conv2's
    output, conv1's output (the debug tap) and the per-tile channel sums, each between sentinel rows.  The uint8 form is
    also held bit-equal to the float form on float32(u8) / 255."""
    torch = _t()
    import numpy as np
    F = torch.nn.functional
    g = _gen("stem", b, h, w)           # (the same data for both input forms)
    d = _dev()
    raw = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.uint8)
    x = torch.from_numpy((np.asarray(raw.numpy(), dtype=np.float32) / 255.0).transpose(0, 3, 1, 2).copy())
    w1 = torch.randn(32, 3, 3, 3, generator=g) / 27 ** 0.5
    b1 = torch.randn(32, generator=g) * 0.3
    w2 = torch.randn(32, 1, 3, 3, generator=g) / 3
    b2 = torch.randn(32, generator=g) * 0.3

    def op(dt):
        c1 = F.relu(F.conv2d(x.to(dt), w1.to(dt), b1.to(dt), 2, 1))
        return c1, F.relu(F.conv2d(c1, w2.to(dt), b2.to(dt), 1, 1, 1, 32))

    c1, c2 = op(torch.float64)
    ho, wo = c2.shape[2], c2.shape[3]
    tiles = -(-ho // 8) * -(-wo // 8)
    w1p, w2p = w1.permute(2, 3, 1, 0).reshape(27, 32).contiguous().to(d), w2.reshape(32, 9).T.contiguous().to(d)
    b1d, b2d = b1.to(d), b2.to(d)
    lib = _lib()

    def launch(as_u8):
        out = torch.full((b * ho * wo + 2, 32), -7.0, device=d)
        t1 = torch.full((b * ho * wo + 2, 32), -7.0, device=d)
        sm = torch.full((b * tiles + 2, 32), -7.0, device=d)
        xin = raw.to(d) if as_u8 else x.to(d)
        _ok(lib.casync_op_pfld_stem(_p(xin), int(as_u8), _p(w1p), _p(b1d), _p(w2p), _p(b2d), out.data_ptr() + 128, sm.data_ptr() + 128,
                                    t1.data_ptr() + 128, b, h, w, _s()), "pfld_stem")
        return out, t1, sm

    with _Run(0) as r:
        out, t1, sm = launch(u8)
    err = max(_rel(out[1:-1], c2.permute(0, 2, 3, 1).reshape(-1, 32)), _rel(t1[1:-1], c1.permute(0, 2, 3, 1).reshape(-1, 32)))
    want = _tile_sums(c2, 8).reshape(b * tiles, 32)
    bar = _bar4(_tile_sums(op(torch.float32)[1], 8).reshape(b * tiles, 32), want)
    err = max(err, _scaled(_abs(sm[1:-1], want), bar, 3e-6))
    for buf in (out, t1, sm):
        if not bool((buf[0] == -7.0).all() and (buf[-1] == -7.0).all()):
            err = float("inf")
    if u8:
        other = launch(False)
        if not all(bool(torch.equal(p, q)) for p, q in zip((out, t1, sm), other)):
            err = float("inf")
    return _done(r, err, 3e-6, f"pfld stem u8={u8} {b}x{h}x{w}")


# ------------------------------------------------------------------ head
def head(b):
    """casync_op_pfld_head vs float64: the four means from per-tile sums (tile counts that divide nothing evenly), conv7,
    conv8, conv_out; out a column slice of a sentinel-filled buffer.  No bar of this kind in tests/kernel_ledger.py:
    4 x the float32 torch error of the same op."""
    torch = _t()
    import ctypes
    F = torch.nn.functional
    g = _gen("head", b)
    d = _dev()
    widths, tiles, counts = (32, 40, 48, 72), (144, 7, 16, 4), (9216, 2304, 576, 144)
    sums = [torch.randn(b, t, c, generator=g) * (n / t) ** 0.5 + 0.4 * n / t for c, t, n in zip(widths, tiles, counts)]
    x6 = torch.randn(b, 8, 12, 12, generator=g)
    w7 = torch.randn(16, 8, 3, 3, generator=g) / 72 ** 0.5
    b7 = torch.randn(16, generator=g) * 0.3
    w8 = torch.randn(64, 16, 12, 12, generator=g) / 2304 ** 0.5
    wo = torch.randn(220, 256, generator=g) / 16
    bo = torch.randn(220, generator=g) * 0.3

    def op(dt):
        means = [s.to(dt).sum(1) / n for s, n in zip(sums, counts)]
        a = F.relu(F.conv2d(x6.to(dt), w7.to(dt), b7.to(dt), 1, 1))
        x5 = F.relu(F.conv2d(a, w8.to(dt))).flatten(1)
        return torch.cat(means + [x5], 1) @ wo.to(dt).T + bo.to(dt)

    ref = op(torch.float64)
    bar = _bar4(op(torch.float32), ref)
    sd_ = [s.contiguous().to(d) for s in sums]
    ptrs = (ctypes.c_void_p * 4)(*[s.data_ptr() for s in sd_])
    nt, cnt = (ctypes.c_int * 4)(*tiles), (ctypes.c_int * 4)(*counts)
    x6d = x6.permute(0, 2, 3, 1).contiguous().to(d)
    w7p = w7.permute(2, 3, 1, 0).reshape(72, 16).contiguous().to(d)
    w8p = w8.permute(2, 3, 1, 0).reshape(2304, 64).contiguous().to(d)
    wop, b7d, bod = wo.T.contiguous().to(d), b7.to(d), bo.to(d)
    ld = 220 + 36
    out = torch.full((b, ld), -7.0, device=d)
    with _Run(0) as r:
        _ok(_lib().casync_op_pfld_head(ptrs, nt, cnt, _p(x6d), _p(w7p), _p(b7d), _p(w8p), _p(wop), _p(bod), out.data_ptr() + 64, ld, b,
                                       _s()), "pfld_head")
    err = max(_abs(out[:, 16:236], ref), _sentinel(out, 16, 236, -7.0))
    return _done(r, err, bar, f"pfld head B={b}")


# ------------------------------------------------------------------ the ledger of lib/obj_lmk/
LEDGER = {
    "lmk_ghost_kernel<true>": [C(ghost, 1, 3, 12, 12, 72, 126, 0), C(ghost, 1, 3, 20, 28, 32, 24, 0), C(ghost, 1, 2, 7, 5, 40, 30, 0),
                               C(ghost, 1, 3, 20, 28, 48, 84, 0), C(ghost, 1, 1, 13, 12, 48, 60, 1)],
    "lmk_ghost_kernel<false>": [C(ghost, 0, 3, 12, 12, 252, 36, 1), C(ghost, 0, 3, 20, 28, 60, 20, 1), C(ghost, 0, 1, 12, 12, 108, 4, 0),
                                C(ghost, 0, 3, 20, 28, 120, 24, 1), C(ghost, 0, 2, 11, 7, 100, 24, 0)],
    "lmk_dw_s2_kernel": [C(dw_s2, 3, 24, 24, 100), C(dw_s2, 2, 13, 9, 48), C(dw_s2, 1, 96, 96, 48), C(dw_s2, 3, 7, 12, 168)],
    "lmk_stem_kernel<false>": [C(stem, 0, 3, 24, 40), C(stem, 0, 2, 23, 37), C(stem, 0, 1, 192, 192)],
    "lmk_stem_kernel<true>": [C(stem, 1, 3, 24, 40), C(stem, 1, 2, 23, 37), C(stem, 1, 1, 192, 192)],
    "lmk_head_kernel": [C(head, 1), C(head, 3)],
}


def cases():
    """[(kernel, index, case)] in ledger order: one GPU test each"""
    return [(name, i, c) for name, cs in LEDGER.items() for i, c in enumerate(cs)]
