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
from kernel_ledger_det import Prec, _fence_ok, _fenced, family


def _half_ulp(top: float) -> float:
    """half a bf16 ulp (8 significant bits) at magnitude `top`"""
    return 2.0 ** (math.floor(math.log2(max(top, 1e-30))) - 8)


# the six cases this precision shares with tests/kernel_ledger_det.py: its bodies on bf16 activations, with the bars above
BF16 = Prec("bfloat16", "casync_op_s3fd16_", 2, "det16_", "s3fd16", _half_ulp)
stem, maxpool, im2col, relu, l2norm, head = family(BF16)


# ------------------------------------------------------------------ widening
def widen(n):
    """casync_op_s3fd16_widen: bf16 -> fp32, exact"""
    torch = _t()
    g = _gen("det16_widen", n)
    x = (torch.randn(n, generator=g) * 2.5).bfloat16()
    out = _fenced(1, n)
    with _Run(0) as r:
        _ok(_lib().casync_op_s3fd16_widen(_p(x.to(_dev())), out.data_ptr() + 4 * n, n, _s()), "s3fd16_widen")
    err = _abs(out[1], x.float()) if _fence_ok(out) else float("inf")
    return _done(r, err, 0.0, f"s3fd16 widen n={n}")


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
