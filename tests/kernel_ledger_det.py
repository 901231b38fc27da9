"""The ledger of calipsync_amd/lib/obj_det/ (the kernels of the S3FD face-detector handle, csrc/facedet.hip), under the rule
of tests/kernel_ledger.py: every compiled kernel instance has op-level cases that launch it through its C-ABI entry with the
launch log on and hold it to a float64 (or exact) reference.  The channel widths are the network's; the spatial sizes are the
smallest that break something: odd, not a multiple of the four pixels a head wave takes, one row, more than one block.

Bars, from tests/kernel_ledger.py's fp32 ops of the same kind:
  * stem and heads (dense 3x3 convs) = conv3x3: max|d| <= 3e-6 max|ref|;
  * max pooling, the dilated im2col and the ReLU pass move or select values: exact (bar 0);
  * kinds without a bar there -- L2Norm and priors + decode + softmax -- take 4 x the error of the same op in float32 torch
    against float64 on the case's own data (_bar4).
Every output goes into a sentinel-filled buffer, between sentinel rows.  Nothing here touches a GPU at import.

The six cases the bf16 precision has too (stem, maxpool, im2col, relu, l2norm, head) are written once, as bodies that take a
precision record (Prec): tests/kernel_ledger_det16.py binds the same bodies to its record, its entries and its bars.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

from kernel_ledger import (C, _abs, _dev, _done, _gen, _lib, _ok, _p, _rel, _Run, _s, _t)
from kernel_ledger_lmk import _bar4

FENCE = -7.0        # exact in bf16


class Prec(NamedTuple):
    """One precision of the handle, as the six case bodies the two ledgers share see it"""
    dtype: str          # torch dtype of the activations
    entry: str          # the C-ABI entries are entry + "stem", ...
    size: int           # bytes per value: a payload starts one sentinel row into its buffer
    tag: str            # prefix of the _gen tags (they seed the data)
    label: str          # opens every case's description
    half_ulp: Callable  # magnitude -> what one rounding of the output to the activation type may add to the bar


F32 = Prec("float32", "casync_op_s3fd_", 4, "det_", "s3fd", lambda top: 0.0)


def family(p):
    """(stem, maxpool, im2col, relu, l2norm, head) of precision p: the shared bodies with p bound, each a function of its own
    (a ledger case is cached by its function and parameters)"""
    def bind(body):
        def fn(*params):
            return body(p, *params)
        fn.__name__, fn.__doc__ = body.__name__[1:], body.__doc__
        return fn
    return tuple(bind(body) for body in (_stem, _maxpool, _im2col, _relu, _l2norm, _head))


def _fenced(rows, cols, dtype=None):
    """a sentinel-filled [rows + 2, cols] buffer (fp32 unless told otherwise); the payload is rows 1 .. rows"""
    return _t().full((rows + 2, cols), FENCE, device=_dev(), dtype=dtype or _t().float32)


def _fence_ok(*bufs):
    return all(bool((b[0].float() == FENCE).all() and (b[-1].float() == FENCE).all()) for b in bufs)


def _entry(p, name):
    return getattr(_lib(), p.entry + name)


# ------------------------------------------------------------------ stem
def _stem(p, u8, b, h, w):
    """the stem entry (float NCHW with the mean subtracted, or uint8 HWC) vs float64 (rounded once to bf16 in bf16); the uint8
    form also bit-equal to the float form on float32(u8) - mean"""
    torch = _t()
    import numpy as np
    from calipsync_amd import facedet
    F = torch.nn.functional
    g = _gen(p.tag + "stem", b, h, w)          # (the same data for both input forms)
    d = _dev()
    raw = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.uint8)
    x = torch.from_numpy((np.asarray(raw.numpy(), dtype=np.float32) - facedet.IMG_MEAN).transpose(0, 3, 1, 2).copy())
    w1 = torch.randn(64, 3, 3, 3, generator=g) / (27 ** 0.5 * 50.0)
    b1 = torch.randn(64, generator=g) * 0.3
    ref = F.relu(F.conv2d(x.double(), w1.double(), b1.double(), 1, 1)).permute(0, 2, 3, 1).reshape(-1, 64)
    w1p, b1d = w1.permute(2, 3, 1, 0).reshape(27, 64).contiguous().to(d), b1.to(d)

    def launch(as_u8):
        out = _fenced(b * h * w, 64, getattr(torch, p.dtype))
        xin = raw.to(d) if as_u8 else x.to(d)
        _ok(_entry(p, "stem")(_p(xin), int(as_u8), _p(w1p), _p(b1d), out.data_ptr() + 64 * p.size, b, h, w, _s()), p.label + "_stem")
        return out

    with _Run(0) as r:
        out = launch(u8)
    if p is F32:       # the fp32 conv bar, of max|ref|
        err, bar = _rel(out[1:-1], ref), 3e-6
    else:              # the same bar as an absolute error, and the rounding of the output
        top = float(ref.abs().max())
        err, bar = _abs(out[1:-1], ref), p.half_ulp(top) + 3e-6 * top
    if not _fence_ok(out) or (u8 and not bool(torch.equal(out, launch(False)))):
        err = float("inf")
    return _done(r, err, bar, f"{p.label} stem u8={u8} {b}x{h}x{w}")


# ------------------------------------------------------------------ max pooling
def _maxpool(p, ceil, b, h, w, c):
    """the maxpool entry vs F.max_pool2d(2, 2, ceil_mode) on the values of the activation type: exact"""
    torch = _t()
    g = _gen(p.tag + "maxpool", ceil, b, h, w, c)
    d = _dev()
    x = torch.randn(b, c, h, w, generator=g).to(getattr(torch, p.dtype))
    ref = torch.nn.functional.max_pool2d(x.float(), 2, 2, ceil_mode=bool(ceil)).permute(0, 2, 3, 1)
    out = _fenced(ref.shape[0] * ref.shape[1] * ref.shape[2], c, x.dtype)
    xin = x.permute(0, 2, 3, 1).contiguous().to(d)
    with _Run(0) as r:
        _ok(_entry(p, "maxpool")(_p(xin), out.data_ptr() + p.size * c, b, h, w, c, ceil, _s()), p.label + "_maxpool")
    err = _abs(out[1:-1], ref.reshape(-1, c)) if _fence_ok(out) else float("inf")
    return _done(r, err, 0.0, f"{p.label} maxpool ceil={ceil} {b}x{h}x{w}x{c} -> {tuple(ref.shape[1:3])}")


# ------------------------------------------------------------------ dilated im2col
def _im2col(p, b, h, w, c, dil):
    """the im2col_dil entry vs F.unfold(3, dilation, padding = dilation) reordered to (ky, kx, c): exact"""
    torch = _t()
    g = _gen(p.tag + "im2col", b, h, w, c, dil)
    d = _dev()
    x = torch.randn(b, c, h, w, generator=g).to(getattr(torch, p.dtype))
    cols = torch.nn.functional.unfold(x.float(), 3, dilation=dil, padding=dil)                 # [b, (c, ky, kx), h w]
    ref = cols.reshape(b, c, 9, h * w).permute(0, 3, 2, 1).reshape(b * h * w, 9 * c)
    out = _fenced(b * h * w, 9 * c, x.dtype)
    xin = x.permute(0, 2, 3, 1).contiguous().to(d)
    with _Run(0) as r:
        _ok(_entry(p, "im2col_dil")(_p(xin), out.data_ptr() + 9 * p.size * c, b, h, w, c, dil, _s()), p.label + "_im2col_dil")
    err = _abs(out[1:-1], ref) if _fence_ok(out) else float("inf")
    return _done(r, err, 0.0, f"{p.label} im2col {b}x{h}x{w}x{c} dilation {dil}")


# ------------------------------------------------------------------ ReLU
def _relu(p, n):
    torch = _t()
    g = _gen(p.tag + "relu", n)
    x = torch.randn(n, generator=g).to(getattr(torch, p.dtype))
    buf = _fenced(1, n, x.dtype)
    buf[1] = x.to(_dev())
    with _Run(0) as r:
        _ok(_entry(p, "relu")(buf.data_ptr() + p.size * n, n, _s()), p.label + "_relu")
    err = _abs(buf[1], torch.relu(x.float())) if _fence_ok(buf) else float("inf")
    return _done(r, err, 0.0, f"{p.label} relu n={n}")


# ------------------------------------------------------------------ L2Norm
def _l2norm(p, rows, c):
    """the l2norm entry vs x / (sqrt(sum x^2) + 1e-10) in float64 on the rows as the kernel reads them; row 1 is all zeros (the
    1e-10 keeps it finite: 0)"""
    torch = _t()
    g = _gen(p.tag + "l2norm", rows, c)
    x = (torch.randn(rows, c, generator=g) * 3.0).to(getattr(torch, p.dtype))
    x[1 % rows] = 0.0

    def op(dt):
        v = x.to(dt)
        return torch.div(v, v.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)

    ref = op(torch.float64)
    out = _fenced(rows, c, x.dtype)
    xin = x.to(_dev())
    with _Run(0) as r:
        _ok(_entry(p, "l2norm")(_p(xin), out.data_ptr() + p.size * c, rows, c, _s()), p.label + "_l2norm")
    err = _abs(out[1:-1], ref) if _fence_ok(out) else float("inf")
    return _done(r, err, p.half_ulp(float(ref.abs().max())) + _bar4(op(torch.float32), ref), f"{p.label} l2norm {rows}x{c}")


# ------------------------------------------------------------------ heads
def _head(p, b, h, w, c, maxout):
    """the head entry vs F.conv2d in float64 on the activations as the kernel reads them (fp32 weights, fp32 outputs): the 4 loc
    and 4 conf rows of one source at priors first .. first + h w of P, conf after the max-out (rows 4-6 -> one) or rows 4, 5; the
    priors before and after stay untouched"""
    torch = _t()
    F = torch.nn.functional
    g = _gen(p.tag + "head", b, h, w, c, maxout)
    d = _dev()
    x = torch.randn(b, c, h, w, generator=g).to(getattr(torch, p.dtype))
    wt = torch.randn(8, c, 3, 3, generator=g) / (9 * c) ** 0.5
    bias = torch.randn(8, generator=g) * 0.3
    y = F.conv2d(x.double(), wt.double(), bias.double(), 1, 1).permute(0, 2, 3, 1).reshape(b, h * w, 8)
    ref_conf = torch.stack((y[..., 4:7].max(dim=-1)[0], y[..., 7]), -1) if maxout else y[..., 4:6]
    first, P = 3, h * w + 7
    loc = torch.full((b, P, 4), FENCE, device=d)
    conf = torch.full((b, P, 2), FENCE, device=d)
    xin = x.permute(0, 2, 3, 1).contiguous().to(d)
    wp, bd = wt.permute(0, 2, 3, 1).reshape(8, 9 * c).contiguous().to(d), bias.to(d)
    with _Run(0) as r:
        _ok(_entry(p, "head")(_p(xin), _p(wp), _p(bd), _p(loc), _p(conf), b, h, w, c, P, first, maxout, _s()), p.label + "_head")
    top = max(1e-6, float(y.abs().max()))
    err = max(_abs(loc[:, first:first + h * w], y[..., :4]), _abs(conf[:, first:first + h * w], ref_conf)) / top
    for buf in (loc, conf):
        if not bool((buf[:, :first] == FENCE).all() and (buf[:, first + h * w:] == FENCE).all()):
            err = float("inf")
    return _done(r, err, 3e-6, f"{p.label} head {b}x{h}x{w}x{c} maxout={maxout}")


stem, maxpool, im2col, relu, l2norm, head = family(F32)


# ------------------------------------------------------------------ priors + decode + score
def decode(b, H, W):
    """casync_op_s3fd_decode vs PriorBox + decode + softmax restated in float64 (tests/s3fd_ref.py) on the float32 priors"""
    torch = _t()
    import s3fd_ref
    from calipsync_amd import facedet
    g = _gen("det_decode", b, H, W)
    maps = facedet.map_sizes(H, W)
    P = facedet.n_priors(H, W)
    taps = {"loc": torch.randn(b, P, 4, generator=g), "conf": torch.randn(b, P, 2, generator=g) * 3.0, "maps": maps}
    ref = s3fd_ref.dense(taps, H, W, torch.float64)
    bar = _bar4(s3fd_ref.dense(taps, H, W, torch.float32), ref)
    out = _fenced(b * P, 5)
    loc, conf = taps["loc"].to(_dev()), taps["conf"].to(_dev())
    with _Run(0) as r:
        _ok(_lib().casync_op_s3fd_decode(_p(loc), _p(conf), out.data_ptr() + 20, b, H, W, _s()), "s3fd_decode")
    err = _abs(out[1:-1], ref.reshape(-1, 5)) if _fence_ok(out) else float("inf")
    return _done(r, err, bar, f"s3fd decode {b}x{H}x{W} P={P}")


# ------------------------------------------------------------------ the ledger of lib/obj_det/
LEDGER = {
    "det_stem_kernel<false>": [C(stem, 0, 2, 13, 19), C(stem, 0, 1, 16, 16)],
    "det_stem_kernel<true>": [C(stem, 1, 2, 13, 19), C(stem, 1, 1, 16, 16)],
    "det_maxpool_kernel": [C(maxpool, 0, 2, 7, 10, 64), C(maxpool, 0, 1, 3, 2, 128), C(maxpool, 1, 2, 7, 10, 256), C(maxpool, 1, 1, 1, 6, 256),
                           C(maxpool, 1, 2, 19, 23, 256)],
    "det_im2col_dil_kernel": [C(im2col, 2, 2, 3, 512, 6), C(im2col, 1, 8, 15, 64, 6)],
    "det_relu_kernel": [C(relu, 4), C(relu, 6 * 1024 + 4)],
    "det_l2norm_kernel": [C(l2norm, 37, 256), C(l2norm, 10, 512), C(l2norm, 5, 1024)],
    "det_head_kernel": [C(head, b, h, w, c, int(c == 256)) for c in (256, 512, 1024) for b, h, w in ((2, 1, 1), (2, 1, 2), (1, 10, 12))],
    "det_decode_kernel": [C(decode, 2, 77, 93), C(decode, 1, 64, 64)],
}


def cases():
    """[(kernel, index, case)] in ledger order: one GPU test each"""
    return [(name, i, c) for name, cs in LEDGER.items() for i, c in enumerate(cs)]
