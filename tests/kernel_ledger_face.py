"""The ledger of calipsync_amd/lib/obj_face/ (the face pipeline's kernels between S3FD and PFLD, csrc/face_ops.hip), under the
rule of tests/kernel_ledger.py: every compiled kernel instance has op-level cases that launch it through its casync_op_* entry
with the launch log on.  These are integer kernels (bytes, row selection, a float32 expression with a prescribed rounding per
operation): every bar is exact equality, the error is the number of differing elements (inf where a sentinel around the output
changed).  Inputs and expected values come from tests/face_cases.py: the unchanged oracle's resize_linear_u8, numpy's
mask-select, LandmarkDetector.landmarks_from_crops' loop.  Nothing here touches a GPU at import."""
from __future__ import annotations

import face_cases as fc
from kernel_ledger import C, _done, _Run


def _count(got, want, fence):
    import numpy as np
    if got.shape != want.shape or not fence:
        return float("inf")
    return float(np.count_nonzero(got != want))


def resize(name, batch):
    """casync_op_resize_linear_u8: copy, 2x area and bilinear branches, both scale forms"""
    with _Run(0) as r:
        got, want, fence = fc.run_resize(name, batch)
    return _done(r, _count(got, want, fence), 0.0, f"resize {name} x{batch} -> {want.shape}")


def crops(which):
    """casync_op_face_crops192: one record, one of every kind, more records than a launch carries"""
    with _Run(0) as r:
        got, want, fence = fc.run_crops(which)
    return _done(r, _count(got, want, fence), 0.0, f"crops192 {which}: {len(want)} crops")


def candidates(batch, p, thresh, cap):
    """casync_op_s3fd_candidates on seeded scores: P below, at and above the 256 priors of a step"""
    det = fc.synthetic_det(batch, p, thresh)
    if p > 3:
        det[0, 1, 0] = float("nan")
        det[batch - 1, :, 0] *= 0.5 * thresh          # an all-below frame
    with _Run(0) as r:
        ok, counts = fc.candidates_match(det, thresh, cap)
    return _done(r, 0.0 if ok else float("inf"), 0.0, f"candidates {batch}x{p} > {thresh}, cap {cap}: counts {counts.tolist()}")


def finalize(n):
    with _Run(0) as r:
        got, want, fence = fc.run_finalize(n)
    return _done(r, _count(got, want, fence), 0.0, f"finalize {n} rows")


LEDGER = {
    "face_resize_kernel": [C(resize, "quarter-308x372", 3), C(resize, "fx-42x54", 1), C(resize, "upscale-7x5", 3), C(resize, "identity-12x17", 3),
                           C(resize, "area-20x14", 3), C(resize, "one-column-9x1", 1), C(resize, "to-one-pixel-6x9", 3)],
    "face_crops192_kernel": [C(crops, "one"), C(crops, "kinds"), C(crops, "many")],
    "face_candidates_kernel": [C(candidates, 3, 596, 0.5, 596), C(candidates, 2, 256, 0.25, 40), C(candidates, 1, 1, 0.0, 1),
                               C(candidates, 2, 1031, 0.9, 64)],
    "face_finalize_kernel": [C(finalize, 1), C(finalize, 70)],
}


def cases():
    """[(kernel, index, case)] in ledger order: one GPU test each"""
    return [(name, i, c) for name, cs in LEDGER.items() for i, c in enumerate(cs)]
