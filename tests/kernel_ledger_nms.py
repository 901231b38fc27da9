"""The ledger of calipsync_amd/lib/obj_nms/ (S3FD's two NMS passes, csrc/face_nms.hip), under the rule of tests/kernel_ledger.py:
every compiled kernel instance has op-level cases that launch it through its casync_op_* entry with the launch log on.  Every
operation of the kernel is an IEEE one in a stated type, so every bar is exact equality with the host code (facedet.detect_output,
facedet.detect_faces_rows): the error is the number of differing elements, status and stage-1 rows included (inf where a sentinel
around an output changed).  Inputs and expected values come from tests/nms_cases.py.  Nothing here touches a GPU at import."""
from __future__ import annotations

import nms_cases as nc
from kernel_ledger import C, _done, _Run


def nms(*case):
    """casync_op_s3fd_nms on one row of nms_cases.TABLE, alone (B = 1, cap = its count)"""
    rows, want = nc.table_case(*case)
    with _Run(0) as r:
        got = nc.run_nms([rows], len(rows))
    err = nc.frame_differences(got, 0, want) if got["fence"] else float("inf")
    return _done(r, err, 0.0, f"nms of {len(rows)} rows: {want.detect_n} kept, {want.status} faces")


def nms_batch():
    """one call of four frames (0, 65, 1024 and 2 rows) with cap 1024"""
    cases = [None] + [nc.table_case(*nc.TABLE[i]) for i in (3, 6, 1)]
    frames = [c[0] if c else nc.candidate_rows(0, 1) for c in cases]
    with _Run(0) as r:
        got = nc.run_nms(frames, 1024)
    err = sum(nc.frame_differences(got, b, c[1] if c else nc.Expected(frames[b])) for b, c in enumerate(cases)) if got["fence"] else float("inf")
    return _done(r, err, 0.0, f"nms of 4 frames: status {got['status'].tolist()}")


LEDGER = {
    "face_nms_kernel": [C(nms, *nc.TABLE[0]), C(nms, *nc.TABLE[4]), C(nms, *nc.TABLE[7]), C(nms_batch)],
}


def cases():
    """[(kernel, index, case)] in ledger order: one GPU test each"""
    return [(name, i, c) for name, cs in LEDGER.items() for i, c in enumerate(cs)]
