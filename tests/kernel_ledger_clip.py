"""The ledger of calipsync_amd/lib/obj_clip/ (the two byte-move kernels of a clip resident on the device, csrc/clip_ops.hip),
under the rule of tests/kernel_ledger.py: every compiled kernel instance has op-level cases that launch it through its
casync_op_* entry with the launch log on.  These are byte moves: every bar is exact equality with numpy slicing, the error is
the number of differing bytes of the whole output buffer, gaps between regions included (inf where a fence around it changed).
Inputs and expected values come from tests/clip_cases.py.  Nothing here touches a GPU at import."""
from __future__ import annotations

import clip_cases as cc
from kernel_ledger import C, _done, _Run


def gather(h, w, repeat=1):
    """casync_op_clip_gather on the batch of one size: every kind of box, region offsets of any alignment"""
    with _Run(0) as r:
        err = cc.run_gather(h, w, repeat)
    return _done(r, err, 0.0, f"gather {cc.case(h, w, repeat).batch} boxes of {h} x {w} frames")


def compose(h, w, repeat=1, plain=False):
    """casync_op_clip_compose on the same batch; plain: no valid record, out_regions NULL"""
    with _Run(0) as r:
        err = cc.run_compose(h, w, repeat, plain)
    return _done(r, err, 0.0, f"compose {cc.case(h, w, repeat).batch} frames of {h} x {w}{' (plain fetch)' if plain else ''}")


# every size of clip_cases.SIZES, the real size, and 80 records (two launches of 64 and 16)
LEDGER = {
    "clip_gather_kernel": [C(gather, h, w) for h, w in cc.SIZES] + [C(gather, *cc.REAL), C(gather, 5, 7, 10)],
    "clip_compose_kernel": [C(compose, h, w) for h, w in cc.SIZES] + [C(compose, h, w, 1, True) for h, w in cc.SIZES] +
                           [C(compose, *cc.REAL), C(compose, 33, 31, 10), C(compose, 5, 7, 10, True)],
}


def cases():
    """[(kernel, index, case)] in ledger order: one GPU test each"""
    return [(name, i, c) for name, cs in LEDGER.items() for i, c in enumerate(cs)]
