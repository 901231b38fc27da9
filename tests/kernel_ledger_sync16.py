"""The ledger of calipsync_amd/lib/obj_sync16/ (the kernels of the bf16 precision of the SyncNet_color handle,
csrc/syncnet_bf16.hip), under the rule of tests/kernel_ledger.py: every compiled kernel instance has op-level cases that launch
it through its casync_op_sync16_* entry with the launch log on and hold it to a float64 reference computed from the SAME
bf16-representable inputs.  The conv cases are the smallest shapes that reach each branch: a tail of M with frames that
straddle a tile (M = 70), stride (1, 2), stride 2 with pad 2, pad 0, the 16-channel tile, cin = 32 (two taps in one chunk of
64 k, and K = 288 ends inside a chunk), K = 4608, the 5x5 kernel (K = 800 ends inside a chunk), the 1x1 kernel's fp32 store.

Bars, per element (the error is reported as max |d| / tolerance, the bar is 1):
  * a conv with a bf16 store: 2^-8 |y| + K 2^-23 sum|a||w| -- the rounding of the store (half a bf16 ulp is at most 2^-8 |y|) and
    the bound of an fp32 sum of K products in any order;
  * the 1x1 conv's fp32 store: K 2^-23 sum|a||w|;
  * the stem computes in fp32 as sync_stem7_kernel does and rounds once: 2^-8 |y| + 3e-6 max|ref| (that kernel's bar in
    tests/kernel_ledger_sync.py);
  * to_nchw widens bf16 values: exact.
Every output goes into a buffer between sentinel rows.  Nothing here touches a GPU at import.
"""
from __future__ import annotations

from kernel_ledger import (C, _dev, _done, _gen, _lib, _ok, _p, _Run, _s, _t)
from kernel_ledger_sync import Precision, _guards, _rows, stem7_of, to_nchw_of


def _ratio(got, ref, tol):
    """max |got - ref| / tol; inf where a value is not finite"""
    torch = _t()
    got = got.double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / (tol + 1e-300)).max())


# ------------------------------------------------------------------ stem and to_nchw: kernel_ledger_sync's bodies in bf16
def _stem_bar(out, ref):
    return _ratio(out, ref, ref.abs() * 2.0 ** -8 + 3e-6 * float(ref.abs().max())), 1.0


BF16 = Precision("sync16", "bfloat16", _stem_bar)


def stem7(b, h, w):
    return stem7_of(BF16, b, h, w)


def to_nchw(b, hw, c):
    return to_nchw_of(BF16, b, hw, c)


# ------------------------------------------------------------------ KS x KS conv, any stride and pad, (+ x), ReLU
def conv(ks, tile, b, h, w, cin, cout, sh, sw, pad, res):
    """casync_op_sync16_conv{1,3,5} vs float64 on bf16-representable inputs; tile: the 3x3 entry's channel tile (else 0);
    res: a bf16 residual [B,ho,wo,cout] added before the ReLU.  The 1x1 entry stores fp32."""
    torch = _t()
    F = torch.nn.functional
    g = _gen("sync16_conv", ks, tile, b, h, w, cin, cout, sh, sw, pad, res)
    d = _dev()
    K = ks * ks * cin
    x = torch.randn(b, cin, h, w, generator=g).bfloat16()
    wt = (torch.randn(cout, cin, ks, ks, generator=g) / K ** 0.5).bfloat16()
    bias = torch.randn(cout, generator=g) * 0.3
    y = F.conv2d(x.double(), wt.double(), bias.double(), (sh, sw), pad).permute(0, 2, 3, 1)
    assert tuple(y.shape[1:3]) == ((h + 2 * pad - ks) // sh + 1, (w + 2 * pad - ks) // sw + 1)
    sum_abs = F.conv2d(x.double().abs(), wt.double().abs(), None, (sh, sw), pad).permute(0, 2, 3, 1).reshape(-1, cout)
    r_ = torch.randn(y.shape, generator=g).bfloat16() if res else None
    ref = F.relu(y + r_.double() if res else y).reshape(-1, cout)
    f32_out = ks == 1
    tol = K * 2.0 ** -23 * sum_abs + (0.0 if f32_out else 2.0 ** -8 * ref.abs())
    xd = x.permute(0, 2, 3, 1).contiguous().to(d)
    wp = wt.permute(0, 2, 3, 1).reshape(cout, K).contiguous().to(d)
    bd, rd = bias.to(d), (r_.contiguous().to(d) if res else None)
    out, ptr = _rows(ref.shape[0], cout, d, "float32" if f32_out else "bfloat16")
    lib = _lib()
    with _Run(0) as r:
        if ks == 1:
            assert (sh, sw, pad, res) == (1, 1, 0, 0)
            _ok(lib.casync_op_sync16_conv1(_p(xd), _p(wp), _p(bd), ptr, b, h, w, cin, cout, _s()), "sync16_conv1")
        elif ks == 5:
            assert (cin, cout, sh, sw, pad, res) == (32, 64, 2, 2, 1, 0)
            _ok(lib.casync_op_sync16_conv5(_p(xd), _p(wp), _p(bd), ptr, b, h, w, _s()), "sync16_conv5")
        else:
            _ok(lib.casync_op_sync16_conv3(_p(xd), _p(wp), _p(bd), _p(rd), ptr, b, h, w, cin, cout, sh, sw, pad, tile, _s()), "sync16_conv3")
    what = f"sync16 conv{ks} tile {tile} {b}x{h}x{w} {cin}->{cout} s({sh},{sw}) p{pad} res={res} M={ref.shape[0]} K={K}"
    return _done(r, max(_ratio(out[1:-1], ref, tol), _guards(out)), 1.0, what)


# ------------------------------------------------------------------ the ledger of lib/obj_sync16/
LEDGER = {
    "sync16_stem7_kernel": [C(stem7, 2, 9, 11), C(stem7, 2, 17, 8), C(stem7, 1, 20, 37)],
    "sync16_conv_kernel<3, 64>": [C(conv, 3, 64, 2, 5, 7, 64, 64, 1, 1, 1, 1), C(conv, 3, 64, 1, 4, 10, 64, 128, 1, 2, 1, 0),
                                  C(conv, 3, 64, 2, 8, 8, 64, 64, 2, 2, 2, 0), C(conv, 3, 64, 1, 6, 6, 32, 64, 1, 1, 1, 0),
                                  C(conv, 3, 64, 1, 3, 3, 512, 64, 1, 1, 1, 0)],
    "sync16_conv_kernel<3, 16>": [C(conv, 3, 16, 3, 5, 5, 64, 64, 1, 1, 0, 0), C(conv, 3, 16, 2, 5, 7, 64, 64, 1, 1, 1, 1),
                                  C(conv, 3, 16, 1, 6, 6, 32, 64, 1, 1, 1, 0), C(conv, 3, 16, 1, 3, 3, 512, 128, 1, 1, 1, 0)],
    "sync16_conv_kernel<5, 64>": [C(conv, 5, 0, 1, 9, 11, 32, 64, 2, 2, 1, 0), C(conv, 5, 0, 2, 3, 3, 32, 64, 2, 2, 1, 0)],
    "sync16_conv_kernel<1, 16>": [C(conv, 1, 0, 3, 3, 3, 64, 64, 1, 1, 0, 0), C(conv, 1, 0, 2, 9, 8, 512, 128, 1, 1, 0, 0)],
    "sync16_to_nchw_kernel": [C(to_nchw, 2, 25, 12), C(to_nchw, 1, 81, 256)],
}


def cases():
    """[(kernel, index, case)] in ledger order: one GPU test each"""
    return [(name, i, c) for name, cs in LEDGER.items() for i, c in enumerate(cs)]
