#!/usr/bin/env python3
"""Per-kernel and per-family table of the bf16 HuBERT forward from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats -d DIR -o hb16 -- python tools/hubert_bench.py --precision bf16 --shapes clip60s --no-baseline
    python tools/hubert_trace_table.py DIR/hb16_results.db [--csv profiles/hubert_bf16_kernel_stats.csv] [--batch 3] [--layers 24]

The trace holds the fp32 engine's forwards too (the bench times both in one process).  A bf16 forward is the run of
dispatches from hb16_conv0_kernel to hb16_layernorm1024_kernel<true> (the final LayerNorm); inside it the GEMMs before the
feature projection's LayerNorm are the conv stack, the fp32 GEMM and the positional conv after it are the fp32 front end,
the rest are the encoder layers.  Times are means per forward over all traced bf16 forwards but the first two (warm-up);
TFLOP/s are on FLOPs counted from shapes (tools/hubert_bench.py flops())."""
from __future__ import annotations

import argparse
import collections
import csv
import os
import sqlite3
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_names import short  # noqa: E402

FIRST, LAST, FP_LN = "hb16_conv0_kernel", "hb16_layernorm1024_kernel<true>", "hb16_layernorm512_kernel<true, false>"


def forwards(db_path: str):
    """[[(short name, microseconds)] per bf16 forward]"""
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, duration from kernels order by start").fetchall()
    out, cur = [], None
    for name, dur in rows:
        k = short(name)
        if k == FIRST:
            cur = []
        if cur is not None:
            cur.append((k, dur / 1e3))
            if k == LAST:
                out.append(cur)
                cur = None
    return out


def family(k: str, seen_fp_ln: bool) -> str:
    if k.startswith("pw_gemm_glds_kernel<__bf16"):
        return "layer GEMMs (bf16)" if seen_fp_ln else "conv1..6 GEMMs (bf16)"
    if k.startswith("pw_gemm_glds_kernel<float") or k == "hb_posconv_kernel":
        return "fp32 front end (projection + positional conv)"
    if k == "hb16_attention_kernel":
        return "attention (bf16)"
    if k.startswith("hb16_layernorm") or k in ("hb16_gelu_kernel", "hb16_conv0_kernel", "hb16_widen_kernel"):
        return "conv0, LayerNorm, GELU passes"
    return "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--csv")
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    a = ap.parse_args()
    fw = forwards(a.db)
    if len(fw) > 2:
        fw = fw[2:]
    n = len(fw)
    per_kernel, per_family = collections.OrderedDict(), collections.OrderedDict()
    for f in fw:
        seen = False
        for k, us in f:
            c = per_kernel.setdefault(k, [0, 0.0])
            c[0] += 1
            c[1] += us
            per_family[family(k, seen)] = per_family.get(family(k, seen), 0.0) + us
            seen = seen or k == FP_LN
    total = sum(v[1] for v in per_kernel.values()) / n
    # FLOPs per forward and family, counted from shapes
    T, t, conv = 1000, 320080, 0.0
    for i, (k, s) in enumerate(zip((10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2))):
        t = (t - k) // s + 1
        conv += 2.0 * t * 512 * 512 * k if i else 0.0
    fl = {"conv1..6 GEMMs (bf16)": conv, "fp32 front end (projection + positional conv)": 2.0 * T * 512 * 1024 + 2.0 * T * 1024 * 64 * 128,
          "layer GEMMs (bf16)": a.layers * 2.0 * T * 1024 * 12288, "attention (bf16)": a.layers * 4.0 * T * T * 1024}
    print(f"{n} bf16 forwards, {total / 1e3:.3f} ms of kernel time per forward")
    print(f"{'family':52s} {'us/forward':>11s} {'share':>7s} {'TFLOP/s':>9s}")
    for fam, us in sorted(per_family.items(), key=lambda kv: -kv[1]):
        tf = f"{a.batch * fl[fam] / (us / n) / 1e6:9.1f}" if fam in fl else f"{'-':>9s}"
        print(f"{fam:52s} {us / n:11.1f} {us / n / total:7.3f} {tf}")
    rows = sorted(per_kernel.items(), key=lambda kv: -kv[1][1])
    if a.csv:
        with open(a.csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["kernel", "calls_per_forward", "us_per_forward", "mean_us", "share"])
            for k, (c, us) in rows:
                w.writerow([k, round(c / n, 2), round(us / n, 1), round(us / c, 2), round(us / n / total, 4)])
    for k, (c, us) in rows:
        print(f"{k:60s} {c / n:7.1f} calls {us / n:9.1f} us {us / n / total:6.3f}")


if __name__ == "__main__":
    main()
