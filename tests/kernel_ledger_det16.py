"""The ledger of calipsync_amd/lib/obj_det16/ (the kernels of the bf16 precision of the S3FD handle, csrc/facedet_bf16.hip),
under the rule of tests/kernel_ledger.py: every compiled kernel instance has op-level cases that launch it through its
casync_op_s3fd16_* entry with the launch log on and hold it to a float64 (or exact) reference computed from the SAME
bf16-rounded inputs.  The channel widths are the network's; the spatial sizes are those of tests/kernel_ledger_det.py, the
smallest that break something (odd, one row, not a multiple of the four pixels a head wave or a stem lane takes, more than
one block or tile), and L2Norm has an all-zero row.

Bars:
  * max pooling, the dilated im2col, the ReLU pass and the widening move or select bf16 values: exact (bar 0);
  * stem and L2Norm compute in fp32 and round once to bf16: half a bf16 ulp of the largest magnitude of the reference, plus
    the fp32 bar of the same op in tests/kernel_ledger_det.py (3e-6 max|ref| for the stem; 4 x the error of the op in
    float32 torch against float64 for L2Norm), as an absolute error;
  * the heads write fp32: the fp32 bar of det_head_kernel, max|d| <= 3e-6 max|ref|, on bf16-exact activations.
Every output goes into a sentinel-filled buffer, between sentinel rows.  Nothing here touches a GPU at import.
"""
from __future__ import annotations

import math

from kernel_ledger import (C, _abs, _dev, _done, _gen, _lib, _ok, _p, _Run, _s, _t)
from kernel_ledger_lmk import _bar4

FENCE = -7.0        # exact in bf16


def _fenced(rows, cols, dtype=None):
    """a sentinel-filled [rows + 2, cols] buffer (bf16 unless told otherwise); the payload is rows 1 .. rows"""
    torch = _t()
    return torch.full((rows + 2, cols), FENCE, device=_dev(), dtype=dtype or torch.bfloat16)


def _fence_ok(*bufs):
    return all(bool((b[0].float() == FENCE).all() and (b[-1].float() == FENCE).all()) for b in bufs)


def _half_ulp(top: float) -> float:
    """half a bf16 ulp (8 significant bits) at magnitude `top`"""
    return 2.0 ** (math.floor(math.log2(max(top, 1e-30))) - 8)


# ------------------------------------------------------------------ stem
def stem(u8, b, h, w):
    """casync_op_s3fd16_stem (float NCHW with the mean subtracted, or uint8 HWC) vs float64 rounded once to bf16; the uint8
    form also bit-equal to the float form on float32(u8) - mean"""
    torch = _t()
    import numpy as np
    from calipsync_amd import facedet
    F = torch.nn.functional
    g = _gen("det16_stem", b, h, w)          # (the same data for both input forms)
    d = _dev()
    raw = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.uint8)
    x = torch.from_numpy((np.asarray(raw.numpy(), dtype=np.float32) - facedet.IMG_MEAN).transpose(0, 3, 1, 2).copy())
    w1 = torch.randn(64, 3, 3, 3, generator=g) / (27 ** 0.5 * 50.0)
    b1 = torch.randn(64, generator=g) * 0.3
    ref = F.relu(F.conv2d(x.double(), w1.double(), b1.double(), 1, 1)).permute(0, 2, 3, 1).reshape(-1, 64)
    w1p, b1d = w1.permute(2, 3, 1, 0).reshape(27, 64).contiguous().to(d), b1.to(d)

    def launch(as_u8):
        out = _fenced(b * h * w, 64)
        xin = raw.to(d) if as_u8 else x.to(d)
        _ok(_lib().casync_op_s3fd16_stem(_p(xin), int(as_u8), _p(w1p), _p(b1d), out.data_ptr() + 128, b, h, w, _s()), "s3fd16_stem")
        return out

    with _Run(0) as r:
        out = launch(u8)
    top = float(ref.abs().max())
    err = _abs(out[1:-1], ref)
    if not _fence_ok(out) or (u8 and not bool(torch.equal(out, launch(False)))):
        err = float("inf")
    return _done(r, err, _half_ulp(top) + 3e-6 * top, f"s3fd16 stem u8={u8} {b}x{h}x{w}")


# ------------------------------------------------------------------ max pooling
def maxpool(ceil, b, h, w, c):
    """casync_op_s3fd16_maxpool vs F.max_pool2d(2, 2, ceil_mode) on bf16 values: exact"""
    torch = _t()
    g = _gen("det16_maxpool", ceil, b, h, w, c)
    d = _dev()
    x = torch.randn(b, c, h, w, generator=g).bfloat16()
    ref = torch.nn.functional.max_pool2d(x.float(), 2, 2, ceil_mode=bool(ceil)).permute(0, 2, 3, 1)
    out = _fenced(ref.shape[0] * ref.shape[1] * ref.shape[2], c)
    xin = x.permute(0, 2, 3, 1).contiguous().to(d)
    with _Run(0) as r:
        _ok(_lib().casync_op_s3fd16_maxpool(_p(xin), out.data_ptr() + 2 * c, b, h, w, c, ceil, _s()), "s3fd16_maxpool")
    err = _abs(out[1:-1], ref.reshape(-1, c)) if _fence_ok(out) else float("inf")
    return _done(r, err, 0.0, f"s3fd16 maxpool ceil={ceil} {b}x{h}x{w}x{c} -> {tuple(ref.shape[1:3])}")


# ------------------------------------------------------------------ dilated im2col
def im2col(b, h, w, c, dil):
    """casync_op_s3fd16_im2col_dil vs F.unfold(3, dilation, padding = dilation) reordered to (ky, kx, c): exact"""
    torch = _t()
    g = _gen("det16_im2col", b, h, w, c, dil)
    d = _dev()
    x = torch.randn(b, c, h, w, generator=g).bfloat16()
    cols = torch.nn.functional.unfold(x.float(), 3, dilation=dil, padding=dil)                 # [b, (c, ky, kx), h w]
    ref = cols.reshape(b, c, 9, h * w).permute(0, 3, 2, 1).reshape(b * h * w, 9 * c)
    out = _fenced(b * h * w, 9 * c)
    xin = x.permute(0, 2, 3, 1).contiguous().to(d)
    with _Run(0) as r:
        _ok(_lib().casync_op_s3fd16_im2col_dil(_p(xin), out.data_ptr() + 18 * c, b, h, w, c, dil, _s()), "s3fd16_im2col_dil")
    err = _abs(out[1:-1], ref) if _fence_ok(out) else float("inf")
    return _done(r, err, 0.0, f"s3fd16 im2col {b}x{h}x{w}x{c} dilation {dil}")


# ------------------------------------------------------------------ ReLU, widening
def relu(n):
    torch = _t()
    g = _gen("det16_relu", n)
    x = torch.randn(n, generator=g).bfloat16()
    buf = _fenced(1, n)
    buf[1] = x.to(_dev())
    with _Run(0) as r:
        _ok(_lib().casync_op_s3fd16_relu(buf.data_ptr() + 2 * n, n, _s()), "s3fd16_relu")
    err = _abs(buf[1], torch.relu(x.float())) if _fence_ok(buf) else float("inf")
    return _done(r, err, 0.0, f"s3fd16 relu n={n}")


def widen(n):
    """casync_op_s3fd16_widen: bf16 -> fp32, exact"""
    torch = _t()
    g = _gen("det16_widen", n)
    x = (torch.randn(n, generator=g) * 2.5).bfloat16()
    out = _fenced(1, n, torch.float32)
    with _Run(0) as r:
        _ok(_lib().casync_op_s3fd16_widen(_p(x.to(_dev())), out.data_ptr() + 4 * n, n, _s()), "s3fd16_widen")
    err = _abs(out[1], x.float()) if _fence_ok(out) else float("inf")
    return _done(r, err, 0.0, f"s3fd16 widen n={n}")


# ------------------------------------------------------------------ L2Norm
def l2norm(rows, c):
    """casync_op_s3fd16_l2norm vs x / (sqrt(sum x^2) + 1e-10) in float64 on the bf16 rows; row 1 is all zeros"""
    torch = _t()
    g = _gen("det16_l2norm", rows, c)
    x = (torch.randn(rows, c, generator=g) * 3.0).bfloat16()
    x[1 % rows] = 0.0

    def op(dt):
        v = x.to(dt)
        return torch.div(v, v.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)

    ref = op(torch.float64)
    out = _fenced(rows, c)
    xin = x.to(_dev())
    with _Run(0) as r:
        _ok(_lib().casync_op_s3fd16_l2norm(_p(xin), out.data_ptr() + 2 * c, rows, c, _s()), "s3fd16_l2norm")
    err = _abs(out[1:-1], ref) if _fence_ok(out) else float("inf")
    return _done(r, err, _half_ulp(float(ref.abs().max())) + _bar4(op(torch.float32), ref), f"s3fd16 l2norm {rows}x{c}")


# ------------------------------------------------------------------ heads
def head(b, h, w, c, maxout):
    """casync_op_s3fd16_head vs F.conv2d in float64 on the bf16 activations (fp32 weights): as kernel_ledger_det.head"""
    torch = _t()
    F = torch.nn.functional
    g = _gen("det16_head", b, h, w, c, maxout)
    d = _dev()
    x = torch.randn(b, c, h, w, generator=g).bfloat16()
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
        _ok(_lib().casync_op_s3fd16_head(_p(xin), _p(wp), _p(bd), _p(loc), _p(conf), b, h, w, c, P, first, maxout, _s()), "s3fd16_head")
    top = max(1e-6, float(y.abs().max()))
    err = max(_abs(loc[:, first:first + h * w], y[..., :4]), _abs(conf[:, first:first + h * w], ref_conf)) / top
    for buf in (loc, conf):
        if not bool((buf[:, :first] == FENCE).all() and (buf[:, first + h * w:] == FENCE).all()):
            err = float("inf")
    return _done(r, err, 3e-6, f"s3fd16 head {b}x{h}x{w}x{c} maxout={maxout}")


# ------------------------------------------------------------------ the ledger of lib/obj_det16/
LEDGER = {
    "det16_stem_kernel<false>": [C(stem, 0, 2, 13, 19), C(stem, 0, 1, 16, 16), C(stem, 0, 1, 5, 67)],
    "det16_stem_kernel<true>": [C(stem, 1, 2, 13, 19), C(stem, 1, 1, 16, 16), C(stem, 1, 1, 5, 67)],
    "det16_maxpool_kernel": [C(maxpool, 0, 2, 7, 10, 64), C(maxpool, 0, 1, 3, 2, 128), C(maxpool, 1, 2, 7, 10, 256), C(maxpool, 1, 1, 1, 6, 256),
                             C(maxpool, 1, 2, 19, 23, 256)],
    "det16_im2col_dil_kernel": [C(im2col, 2, 2, 3, 512, 6), C(im2col, 1, 8, 15, 64, 6)],
    "det16_relu_kernel": [C(relu, 8), C(relu, 6 * 1024 + 8)],
    "det16_widen_kernel": [C(widen, 8), C(widen, 6 * 1024 + 8)],
    "det16_l2norm_kernel": [C(l2norm, 37, 256), C(l2norm, 1, 256), C(l2norm, 10, 512), C(l2norm, 5, 1024)],
    "det16_head_kernel": [C(head, b, h, w, c, int(c == 256)) for c in (256, 512, 1024) for b, h, w in ((2, 1, 1), (2, 1, 2), (1, 10, 13))],
}


def cases():
    """[(kernel, index, case)] in ledger order: one GPU test each"""
    return [(name, i, c) for name, cs in LEDGER.items() for i, c in enumerate(cs)]
