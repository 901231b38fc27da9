"""PFLD_GhostOne landmark throughput on one MI355X: the HIP engine (calipsync_amd/landmarks.py) against the same folded
graph in torch (tests/pfld_ref.py) on the same GPU, in one process.

    python tools/landmark_bench.py [--batches 1,8,64] [--steps 50] [--warmup 5] [--no-baseline] [--json profiles/landmark.json]

One JSON line per batch: ms per forward and frames/s of the engine (uint8 crops in, landmarks out) and of torch, kernel
launches per forward, and the algorithmic minimum of bytes per frame (every stage read once and written once, plus the
weights once per forward) with the bandwidth the engine's time would mean at that minimum.  The network is memory- and
launch-bound, not MFMA-bound, so no FLOP roof is quoted.

The profiler runs are runs of their own (never timed, counters never together with a trace):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/landmark_bench.py --batches 8 --no-baseline
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR2/fetch -- python tools/landmark_bench.py --batches 8 --no-baseline --steps 2 --warmup 0
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d DIR2/write -- python tools/landmark_bench.py --batches 8 --no-baseline --steps 2 --warmup 0
(the two counters do not fit one pass) and  --stats-from DIR [--csv profiles/landmark_kernel_stats.csv]  /  --counters-from DIR2
turn what they wrote into the per-kernel table (launches and microseconds per forward, share) and into measured bytes per
frame beside the minimum; both need --forwards N, the forwards of the profiled process (steps + warmup).  The counters count
kilobytes, and on gfx950 FETCH_SIZE tallies the 128-byte requests of wide (16 bytes per lane) reads at 64 bytes: the read
side lies between the counted figure and twice it, and both are given.  --json FILE merges the tables into that file.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def launches_per_forward() -> int:
    """stem + two ghost modules per bottleneck + one stride-2 depthwise per s = 2 bottleneck + head"""
    from calipsync_amd import landmarks
    return 1 + sum(2 + (s == 2) for *_, s in landmarks.BOTTLENECKS) + 1


def min_bytes(batch: int):
    """(activation bytes per frame, weight bytes per forward): the uint8 crop read once, every stage of the table in
    DESIGN section 8c written once and read once by its consumer, the landmarks written; weights = the packed buffer."""
    from calipsync_amd import _lib, landmarks
    act = 192 * 192 * 3
    for (h, w, c), name in zip(landmarks.STAGE_SHAPES, landmarks.STAGES):
        if name == "conv1":          # fused into the stem: never in memory
            continue
        act += h * w * c * 4 * (1 if name == "conv_out" else 2)
    _, total = _lib.pfld_layout()
    return act, total * 4


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


def _rows(directory: str, suffix: str):
    paths = sorted(glob.glob(os.path.join(directory, "**", f"*{suffix}"), recursive=True))
    if not paths:
        raise SystemExit(f"no *{suffix} under {directory}")
    rows = []
    for path in paths if suffix == "counter_collection.csv" else paths[-1:]:     # one file per counter pass
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    return rows


def stats_table(directory: str, forwards: int, out_csv: str | None):
    rows = [r for r in _rows(directory, "kernel_stats.csv") if "lmk_" in r["Name"]]
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    table = [{"kernel": r["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", ""),
              "calls_per_forward": round(float(r["Calls"]) / forwards, 2),
              "us_per_forward": round(float(r["TotalDurationNs"]) / forwards / 1e3, 2),
              "mean_us": round(float(r["AverageNs"]) / 1e3, 2), "share": round(float(r["TotalDurationNs"]) / total, 4)} for r in rows]
    table.sort(key=lambda r: -r["us_per_forward"])
    if out_csv:
        with open(out_csv, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(table[0]))
            w.writeheader()
            w.writerows(table)
    return table


def counter_bytes(directory: str, forwards: int, batch: int):
    fetch = write = 0.0
    for r in _rows(directory, "counter_collection.csv"):
        if "lmk_" not in r["Kernel_Name"]:
            continue
        if r["Counter_Name"] == "FETCH_SIZE":
            fetch += float(r["Counter_Value"])
        elif r["Counter_Name"] == "WRITE_SIZE":
            write += float(r["Counter_Value"])
    fetch, write = fetch * 1024 / forwards / batch, write * 1024 / forwards / batch
    return {"fetch_bytes_per_frame_counted": fetch, "fetch_bytes_per_frame_doubled": 2 * fetch, "write_bytes_per_frame": write}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--json", help="write the lines, with the source hash of the kernels, to this file")
    ap.add_argument("--stats-from", help="directory of a rocprofv3 --kernel-trace --stats run")
    ap.add_argument("--counters-from", help="directory of a rocprofv3 --pmc FETCH_SIZE WRITE_SIZE run")
    ap.add_argument("--forwards", type=int, default=0, help="forwards of the profiled process")
    ap.add_argument("--csv")
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",")]
    from calipsync_amd import build
    if a.stats_from or a.counters_from:
        if a.forwards <= 0:
            raise SystemExit("--forwards N is needed")
        doc = {"source_hash": build.source_hash()}
        if a.stats_from:
            doc["kernels"] = stats_table(a.stats_from, a.forwards, a.csv)
        if a.counters_from:
            act, wts = min_bytes(batches[0])
            doc["traffic"] = dict(counter_bytes(a.counters_from, a.forwards, batches[0]), batch=batches[0],
                                  min_bytes_per_frame=act + wts / batches[0])
        print(json.dumps(doc, indent=1))
        if a.json:
            with open(a.json) as f:
                whole = json.load(f)
            if whole.get("source_hash") != doc.pop("source_hash"):
                raise SystemExit(f"{a.json} was measured on other kernel sources")
            whole.update(doc)
            with open(a.json, "w") as f:
                json.dump(whole, f, indent=1)
                f.write("\n")
        return

    import numpy as np
    import torch
    import pfld_ref
    from calipsync_amd import landmarks, recipe
    sd = recipe.make_pfld_state_dict()
    eng = landmarks.PFLDEngine(sd)
    folded = {k: torch.from_numpy(v).cuda() for k, v in landmarks.fold(sd).items()}
    lines = []
    for b in batches:
        crops = torch.from_numpy(recipe.make_pfld_inputs(min(b, 8))).cuda()
        crops = crops.repeat((b + crops.shape[0] - 1) // crops.shape[0], 1, 1, 1)[:b].contiguous()
        t = timeit(lambda: eng.forward_u8(crops), a.steps, a.warmup)
        act, wts = min_bytes(b)
        res = {"batch": b, "engine_ms": t * 1e3, "frames_per_s": b / t, "launches_per_forward": launches_per_forward(),
               "min_bytes_per_frame": act + wts / b, "gb_per_s_at_min": (act * b + wts) / t / 1e9}
        if not a.no_baseline:
            def torch_forward():
                with torch.no_grad():
                    x = (crops.float() / 255.0).permute(0, 3, 1, 2)
                    return pfld_ref.forward(folded, x)[0]
            d = float((torch_forward() - eng.forward_u8(crops)).abs().max())
            tt = timeit(torch_forward, a.steps, a.warmup)
            res.update({"torch_ms": tt * 1e3, "torch_frames_per_s": b / tt, "speedup_vs_torch": tt / t, "max_abs_diff_vs_torch": d})
        lines.append(res)
        print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"what": "tools/landmark_bench.py " + " ".join(sys.argv[1:]) + " on one MI355X, profiler off",
                       "source_hash": build.source_hash(), "lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
