"""The ledger of calipsync_amd/lib/obj_sync/ (the kernels of the SyncNet_color handle, csrc/syncnet.hip), under the rule of
tests/kernel_ledger.py: every compiled kernel has op-level cases that launch it through its C-ABI entry with the launch log on
and hold it to a float64 reference.  The channel widths are the network's (they are compiled in); the spatial sizes break the
tiling: smaller than a tile, more than one tile, rows and frames that end inside a tile, outputs whose taps are mostly padding.

Bars:
  * stem7, conv5 and conv3 (dense convs) = tests/kernel_ledger.py's conv3x3: max|d| <= 3e-6 max|ref|;
  * embed and curve -- kinds without a bar there -- take 4 x the error of the same op in float32 torch against float64 on the
    case's own data (kernel_ledger_lmk._bar4);
  * relu and to_nchw move values: exact.
Every output goes into a buffer between sentinel rows (relu: in place inside a sentinel-filled buffer).  Nothing here touches a
GPU at import.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

from kernel_ledger import (C, _abs, _dev, _done, _gen, _lib, _ok, _p, _rel, _Run, _s, _t)
from kernel_ledger_lmk import _bar4


def _rows(n_rows, width, d, dtype="float32"):
    """a sentinel-filled [n_rows + 2, width] buffer and the pointer of its row 1"""
    torch = _t()
    buf = torch.full((n_rows + 2, width), -7.0, device=d, dtype=getattr(torch, dtype))
    return buf, buf.data_ptr() + width * buf.element_size()


def _guards(buf):
    """inf when the first or the last row is no longer the sentinel"""
    return 0.0 if bool((buf[0] == -7.0).all() and (buf[-1] == -7.0).all()) else float("inf")


class Precision(NamedTuple):
    """what differs between the fp32 and the bf16 instance of a kernel body both objects compile (csrc/syncnet_common.h)"""
    tag: str              # "sync" | "sync16": the entry casync_op_<tag>_*, the seed's name and the printed line
    dtype: str            # torch's name of the type the stem stores and to_nchw reads
    stem_bar: Callable    # (the stem's output rows, the float64 reference) -> (err, bar)


F32 = Precision("sync", "float32", lambda out, ref: (_rel(out, ref), 3e-6))


# ------------------------------------------------------------------ stem (7x7, pad 3, 3 -> 32, ReLU)
def stem7_of(P, b, h, w):
    """casync_op_<tag>_stem7 on an h x w float NCHW input vs float64"""
    torch = _t()
    F = torch.nn.functional
    g = _gen(f"{P.tag}_stem7", b, h, w)
    d = _dev()
    x = torch.rand(b, 3, h, w, generator=g)
    wt = torch.randn(32, 3, 7, 7, generator=g) / 147 ** 0.5
    bias = torch.randn(32, generator=g) * 0.3
    ref = F.relu(F.conv2d(x.double(), wt.double(), bias.double(), 1, 3)).permute(0, 2, 3, 1).reshape(-1, 32)
    wp = wt.permute(2, 3, 1, 0).reshape(147, 32).contiguous().to(d)
    xd, bd = x.to(d), bias.to(d)
    out, ptr = _rows(b * h * w, 32, d, P.dtype)
    with _Run(0) as r:
        _ok(getattr(_lib(), f"casync_op_{P.tag}_stem7")(_p(xd), _p(wp), _p(bd), ptr, b, h, w, _s()), f"{P.tag}_stem7")
    err, bar = P.stem_bar(out[1:-1], ref)
    return _done(r, max(err, _guards(out)), bar, f"{P.tag} stem7 {b}x{h}x{w}")


def stem7(b, h, w):
    return stem7_of(F32, b, h, w)


# ------------------------------------------------------------------ 5x5, stride 2, pad 1, 32 -> 64, ReLU
def conv5(b, h, w):
    """casync_op_sync_conv5 on an h x w NHWC input vs float64"""
    torch = _t()
    F = torch.nn.functional
    g = _gen("sync_conv5", b, h, w)
    d = _dev()
    x = torch.randn(b, 32, h, w, generator=g)
    wt = torch.randn(64, 32, 5, 5, generator=g) / 800 ** 0.5
    bias = torch.randn(64, generator=g) * 0.3
    ref = F.relu(F.conv2d(x.double(), wt.double(), bias.double(), 2, 1)).permute(0, 2, 3, 1)
    assert tuple(ref.shape[1:3]) == ((h - 3) // 2 + 1, (w - 3) // 2 + 1)
    ref = ref.reshape(-1, 64)
    xd = x.permute(0, 2, 3, 1).contiguous().to(d)
    wp = wt.permute(0, 2, 3, 1).reshape(64, 800).contiguous().to(d)
    bd = bias.to(d)
    out, ptr = _rows(ref.shape[0], 64, d)
    with _Run(0) as r:
        _ok(_lib().casync_op_sync_conv5(_p(xd), _p(wp), _p(bd), ptr, b, h, w, _s()), "sync_conv5")
    return _done(r, max(_rel(out[1:-1], ref), _guards(out)), 3e-6, f"sync conv5 {b}x{h}x{w}")


# ------------------------------------------------------------------ 3x3, any stride and pad, (+ x), ReLU
def conv3(b, h, w, cin, cout, sh, sw, pad, res):
    """casync_op_sync_conv3 vs float64; res: a residual [B,ho,wo,cout] added before the ReLU"""
    torch = _t()
    F = torch.nn.functional
    g = _gen("sync_conv3", b, h, w, cin, cout, sh, sw, pad, res)
    d = _dev()
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.3
    y = F.conv2d(x.double(), wt.double(), bias.double(), (sh, sw), pad).permute(0, 2, 3, 1)
    assert tuple(y.shape[1:3]) == ((h + 2 * pad - 3) // sh + 1, (w + 2 * pad - 3) // sw + 1)
    r_ = torch.randn(y.shape, generator=g) if res else None
    ref = F.relu(y + r_.double() if res else y).reshape(-1, cout)
    xd = x.permute(0, 2, 3, 1).contiguous().to(d)
    wp = wt.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous().to(d)
    bd, rd = bias.to(d), (r_.contiguous().to(d) if res else None)
    out, ptr = _rows(ref.shape[0], cout, d)
    with _Run(0) as r:
        _ok(_lib().casync_op_sync_conv3(_p(xd), _p(wp), _p(bd), _p(rd), ptr, b, h, w, cin, cout, sh, sw, pad, _s()), "sync_conv3")
    return _done(r, max(_rel(out[1:-1], ref), _guards(out)), 3e-6, f"sync conv3 {b}x{h}x{w} {cin}->{cout} s({sh},{sw}) p{pad} res={res}")


# ------------------------------------------------------------------ ReLU in place
def relu(n):
    torch = _t()
    g = _gen("sync_relu", n)
    d = _dev()
    x = torch.randn(n, generator=g)
    buf = torch.full((n + 8,), -7.0, device=d)
    buf[4:4 + n] = x.to(d)
    with _Run(0) as r:
        _ok(_lib().casync_op_sync_relu(buf.data_ptr() + 16, n, _s()), "sync_relu")
    ok = bool(torch.equal(buf[4:4 + n].cpu(), torch.relu(x)) and (buf[:4] == -7.0).all() and (buf[4 + n:] == -7.0).all())
    return _done(r, 0.0 if ok else float("inf"), 0.0, f"sync relu n={n}")


# ------------------------------------------------------------------ NHWC -> NCHW (fp32 out)
def to_nchw_of(P, b, hw, c):
    torch = _t()
    g = _gen(f"{P.tag}_to_nchw", b, hw, c)
    d = _dev()
    x = torch.randn(b, hw, c, generator=g).to(getattr(torch, P.dtype))
    xd = x.to(d)
    out, ptr = _rows(b * c, hw, d)
    with _Run(0) as r:
        _ok(getattr(_lib(), f"casync_op_{P.tag}_to_nchw")(_p(xd), ptr, b, hw, c, _s()), f"{P.tag}_to_nchw")
    ok = bool(torch.equal(out[1:-1].cpu(), x.float().permute(0, 2, 1).reshape(b * c, hw))) and _guards(out) == 0.0
    return _done(r, 0.0 if ok else float("inf"), 0.0, f"{P.tag} to_nchw {b}x{hw}x{c}")


def to_nchw(b, hw, c):
    return to_nchw_of(F32, b, hw, c)


# ------------------------------------------------------------------ embedding
def embed():
    """casync_op_sync_embed, B = 3: a frame of order 1, an all-zero frame (the 1e-12 clamp: zeros, not NaN) and a frame of order
    1e-3; negative entries everywhere (the 0.01 slope).  4 x the float32 torch error of the same op."""
    torch = _t()
    import syncnet_ref
    g = _gen("sync_embed")
    d = _dev()
    x = torch.randn(3, 512, 3, 3, generator=g)
    x[1] = 0.0
    x[2] *= 1e-3
    ref = syncnet_ref.embed(x.double())
    assert bool((ref < 0).any()) and bool((ref[1] == 0).all())
    bar = _bar4(syncnet_ref.embed(x), ref)
    xd = x.permute(0, 2, 3, 1).contiguous().to(d)
    out, ptr = _rows(3, 4608, d)
    with _Run(0) as r:
        _ok(_lib().casync_op_sync_embed(_p(xd), ptr, 3, _s()), "sync_embed")
    return _done(r, max(_abs(out[1:-1], ref), _guards(out)), bar, "sync embed B=3")


# ------------------------------------------------------------------ shift curve
def curve(n, s, dim, roll):
    """casync_op_sync_curve vs float64; roll = k: audio = roll(face, k), and the curve must peak at shift k with value 1 (within
    the bar) on every valid pair of that shift.  4 x the float32 torch error of the same op."""
    torch = _t()
    import syncnet_ref
    g = _gen("sync_curve", n, s, dim, roll)
    d = _dev()
    face = torch.randn(n, dim, generator=g)
    audio = torch.roll(face, roll, 0) if roll is not None else torch.randn(n, dim, generator=g)
    ref = syncnet_ref.shift_curve(face.double(), audio.double(), s)
    bar = _bar4(syncnet_ref.shift_curve(face, audio, s), ref)
    fd, ad = face.to(d), audio.to(d)
    out, ptr = _rows(2 * s + 1, n, d)
    with _Run(0) as r:
        _ok(_lib().casync_op_sync_curve(_p(fd), _p(ad), n, dim, s, ptr, _s()), "sync_curve")
    sim = out[1:-1]
    err = max(_abs(sim, ref), _guards(out))
    if roll is not None:
        row = sim[roll + s, max(0, -roll):min(n, n - roll)].double().cpu()
        means = sim.double().sum(1).cpu() / (n - (torch.arange(-s, s + 1)).abs()).clamp_min(1)
        if int(means.argmax()) != roll + s or float((row - 1.0).abs().max()) > bar:
            err = float("inf")
    return _done(r, err, bar, f"sync curve N={n} S={s} D={dim} roll={roll}")


# ------------------------------------------------------------------ the ledger of lib/obj_sync/
LEDGER = {
    "sync_stem7_kernel": [C(stem7, 2, 9, 11), C(stem7, 2, 17, 8), C(stem7, 1, 20, 37)],
    "sync_conv_kernel<5>": [C(conv5, 1, 33, 21), C(conv5, 2, 3, 3), C(conv5, 3, 9, 8)],
    "sync_conv_kernel<3>": [C(conv3, 2, 9, 11, 64, 64, 1, 1, 1, 1), C(conv3, 2, 7, 6, 64, 128, 2, 2, 2, 0), C(conv3, 3, 5, 8, 256, 64, 1, 2, 1, 0),
                            C(conv3, 2, 3, 3, 512, 512, 1, 1, 0, 0), C(conv3, 1, 9, 9, 32, 256, 2, 2, 1, 0), C(conv3, 2, 5, 5, 512, 64, 1, 1, 1, 1)],
    "sync_relu_kernel": [C(relu, 4), C(relu, 1028)],
    "sync_to_nchw_kernel": [C(to_nchw, 2, 25, 12), C(to_nchw, 1, 81, 256)],
    "sync_embed_kernel": [C(embed)],
    "sync_curve_kernel": [C(curve, 1, 0, 4608, None), C(curve, 7, 3, 4608, 2), C(curve, 3, 5, 260, None), C(curve, 7, 3, 4608, None)],
}


def cases():
    """[(kernel, index, case)] in ledger order: one GPU test each"""
    return [(name, i, c) for name, cs in LEDGER.items() for i, c in enumerate(cs)]
