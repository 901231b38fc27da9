"""SyncNet_color throughput on one MI355X: the HIP engine (calipsync_amd/syncnet.py) beside the same folded graph in eager
torch (tests/syncnet_ref.py) on the same GPU, in one process, the two alternating round by round.

    python tools/syncnet_bench.py [--modes hubert,wenet] [--batches 1,8,64] [--rounds 5] [--steps 10] [--warmup 3]
                                  [--curve 1500,15] [--no-baseline] [--json profiles/syncnet.json] [--precisions fp32,bf16]

One JSON line per (mode, batch): the median and the range over the rounds of ms per forward (both encoders, both embeddings),
pairs per second, and the same for torch; then one line for offset_curve's kernel at N x S (embeddings in, sim out) beside the
same cosines in torch.  5.04 GMAC of convolution a pair (hubert; wenet 5.34): the TFLOP/s of the engine's median is quoted.

--precisions fp32,bf16 adds the bf16 handle (precision="bf16") and, with the baseline, eager torch under bf16 autocast to the
functions that alternate: bf16_* and torch_autocast_* figures on the same line, and the bf16 handle's median against the fp32
handle, torch and torch under autocast.  The default, fp32 alone, prints what it always printed.

The profiler run is a run of its own (never timed):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/syncnet_bench.py --modes hubert --batches 8 --no-baseline --curve 0,0
and  --stats-from DIR --forwards N  (the forwards of the profiled process: rounds x steps + warmup) turns what it wrote into the
per-kernel table: launches and microseconds per forward, share of the forward.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def macs_per_pair(mode: str) -> int:
    from calipsync_amd import syncnet
    return sum(cout * h * w * cin * k * k for (_, k, cin, cout, _, _, _), (_, h, w) in zip(syncnet.blocks(mode), syncnet.stage_shapes(mode)))


def timeit(fn, steps: int, warmup: int) -> float:
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def alternate(fns: dict, rounds: int, steps: int, warmup: int) -> dict:
    """{name: [seconds per call, one per round]}: every round times each function once, in turn"""
    out = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            out[k].append(timeit(fn, steps, warmup if r == 0 else 1))
    return out


def spread(name: str, ts, per: float) -> dict:
    med = statistics.median(ts)
    return {f"{name}_ms": med * 1e3, f"{name}_ms_min": min(ts) * 1e3, f"{name}_ms_max": max(ts) * 1e3, f"{name}_per_s": per / med}


def stats_table(directory: str, forwards: int):
    paths = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not paths:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    with open(paths[-1], newline="") as f:
        rows = list(csv.DictReader(f))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    table = [{"kernel": r["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", ""),
              "calls_per_forward": round(float(r["Calls"]) / forwards, 2), "us_per_forward": round(float(r["TotalDurationNs"]) / forwards / 1e3, 2),
              "share": round(float(r["TotalDurationNs"]) / total, 4)} for r in rows]
    return sorted(table, key=lambda r: -r["us_per_forward"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="hubert,wenet")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--curve", default="1500,15", help="N,S of the offset_curve line (0,0: none)")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--precisions", default="fp32", help="fp32, bf16 or fp32,bf16: the handles that alternate")
    ap.add_argument("--stats-from", help="directory of a rocprofv3 --kernel-trace --stats run")
    ap.add_argument("--forwards", type=int, default=0, help="forwards of the profiled process")
    a = ap.parse_args()
    from calipsync_amd import build
    if a.stats_from:
        if a.forwards <= 0:
            raise SystemExit("--forwards N is needed")
        print(json.dumps({"source_hash": build.source_hash(), "kernels": stats_table(a.stats_from, a.forwards)}, indent=1))
        return

    import torch
    import syncnet_ref
    from calipsync_amd import recipe, syncnet
    lines = []
    precisions = a.precisions.split(",")
    for p in precisions:
        syncnet.check_precision(p)
    for mode in a.modes.split(","):
        sd = recipe.make_syncnet_state_dict(mode)
        net = syncnet.SyncNetColor(mode, "cuda:0", sd)
        net16 = syncnet.SyncNetColor(mode, "cuda:0", sd, precision="bf16") if "bf16" in precisions else None
        folded = {k: torch.from_numpy(v).cuda() for k, v in syncnet.fold(sd, mode).items()}
        for b in (int(v) for v in a.batches.split(",")):
            x, au = (torch.from_numpy(v).cuda() for v in recipe.make_syncnet_inputs(min(b, 8), mode))
            x = x.repeat((b + x.shape[0] - 1) // x.shape[0], 1, 1, 1)[:b].contiguous()
            au = au.repeat((b + au.shape[0] - 1) // au.shape[0], 1, 1, 1)[:b].contiguous()
            fns = {}
            if "fp32" in precisions:
                fns["engine"] = lambda: net(x, au)
            if net16 is not None:
                fns["bf16"] = lambda: net16(x, au)

            def torch_forward():
                with torch.no_grad():
                    return syncnet_ref.forward(folded, x, au, mode)[:2]

            def torch_autocast():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                    return syncnet_ref.forward(folded, x, au, mode)[:2]
            if not a.no_baseline:
                fns["torch"] = torch_forward
                if net16 is not None:
                    fns["torch_autocast"] = torch_autocast
            ts = alternate(fns, a.rounds, a.steps, a.warmup)
            med = {k: statistics.median(v) for k, v in ts.items()}
            res = {"mode": mode, "batch": b}
            if "engine" in ts:
                res.update(spread("engine", ts["engine"], b))
                res["engine_tflops"] = 2.0 * macs_per_pair(mode) * b / med["engine"] / 1e12
            if "bf16" in ts:
                res.update(spread("bf16", ts["bf16"], b))
                res["bf16_tflops"] = 2.0 * macs_per_pair(mode) * b / med["bf16"] / 1e12
                if "engine" in ts:
                    res["bf16_vs_fp32_engine"] = med["engine"] / med["bf16"]
            if not a.no_baseline:
                res.update(spread("torch", ts["torch"], b))
                if "engine" in ts:
                    d = max(float((p - q).abs().max()) for p, q in zip(torch_forward(), net(x, au)))
                    res.update(speedup_vs_torch=med["torch"] / med["engine"], max_abs_diff_vs_torch=d)
                if "bf16" in ts:
                    res.update(spread("torch_autocast", ts["torch_autocast"], b))
                    res.update(bf16_vs_torch=med["torch"] / med["bf16"], bf16_vs_torch_autocast=med["torch_autocast"] / med["bf16"],
                               bf16_max_abs_diff_vs_torch=max(float((p - q).abs().max()) for p, q in zip(torch_forward(), net16(x, au))))
            lines.append(res)
            print(json.dumps(res), flush=True)
    n, s = (int(v) for v in a.curve.split(","))
    if n > 0:
        g = torch.Generator().manual_seed(n)
        f, au = (torch.nn.functional.normalize(torch.randn(n, syncnet.EMBED_DIM, generator=g)).cuda() for _ in range(2))
        fns = {"engine": lambda: syncnet.shift_similarity(f, au, s)}
        if not a.no_baseline:
            def torch_curve():
                sim = torch.zeros(2 * s + 1, n, device="cuda")
                for k in range(-s, s + 1):
                    lo, hi = max(0, -k), min(n, n - k)
                    sim[k + s, lo:hi] = torch.nn.functional.cosine_similarity(f[lo:hi], au[lo + k:hi + k])
                return sim
            fns["torch"] = torch_curve
        ts = alternate(fns, a.rounds, a.steps, a.warmup)
        res = {"curve_n": n, "curve_max_shift": s, **spread("engine", ts["engine"], (2 * s + 1) * n)}
        if not a.no_baseline:
            res.update(spread("torch", ts["torch"], (2 * s + 1) * n))
            res.update(speedup_vs_torch=statistics.median(ts["torch"]) / statistics.median(ts["engine"]),
                       max_abs_diff_vs_torch=float((torch_curve() - syncnet.shift_similarity(f, au, s)).abs().max()))
        lines.append(res)
        print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"what": "tools/syncnet_bench.py " + " ".join(sys.argv[1:]) + " on one MI355X, profiler off",
                       "source_hash": build.source_hash(), "lines": lines}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
