"""S3FD face-detector throughput on one MI355X: the HIP engine (calipsync_amd/facedet.py) against the same graph in eager
fp32 torch (tests/s3fd_ref.py) on the same GPU, in one process, the two alternating round by round, profiler off.

    python tools/facedet_bench.py [--batches 1,8,16] [--hw 270,480] [--steps 10] [--rounds 3] [--warmup 2] [--no-baseline]
                                  [--precision fp32|bf16|both] [--json profiles/facedet.json]

One JSON line per batch: uint8 frames in, the dense det [B,P,5] out; ms per forward (the median of the rounds, and their
spread) and frames/s of both, kernel launches per forward, and the TFLOP/s the engine's time means for the network's
multiply-adds (2 x MACs of every conv, counted from the layer table).  270 x 480 is a 1080p frame at the detector's scale 0.25.
--precision bf16 times the bf16 handle instead; both: the fp32 and the bf16 engine alternate in the same rounds of one process
(as tools/hubert_bench.py does it), the line carries both times and their ratio, and the torch baseline is left out.

The per-kernel table comes from a profiler run of its own, never timed:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/facedet_bench.py --batches 8 --no-baseline
and  --stats-from DIR --forwards N [--csv profiles/facedet_kernel_stats.csv] [--json FILE]  turns it into launches and
microseconds per forward and the share of each kernel (N = the forwards of the profiled process: rounds x steps + warmup).
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

LAUNCHES = 1 + 12 + 5 + 3 + 6 + (1 + 2) + 2 + 2 * 3 + 1    # stem, 12 convs, 5 pools, 3 L2Norms, 6 heads, fc6 (im2col, GEMM, ReLU), fc7, extras, decode


def flops(h: int, w: int) -> float:
    """2 x multiply-adds of one frame"""
    from calipsync_amd import facedet
    maps = facedet.map_sizes(h, w)
    res = {"conv1": (h, w), "conv2": (h // 2, w // 2), "conv3": maps[0], "conv4": maps[1], "conv5": maps[2], "fc6": maps[3], "fc7": maps[3]}
    macs = 0
    for _i, name, cin, cout, k in facedet.VGG:
        hh, ww = res[name.split("_")[0]]
        macs += hh * ww * cin * cout * k * k
    macs += maps[3][0] * maps[3][1] * 1024 * 256 + maps[4][0] * maps[4][1] * 256 * 512 * 9
    macs += maps[4][0] * maps[4][1] * 512 * 128 + maps[5][0] * maps[5][1] * 128 * 256 * 9
    macs += sum(a * b * c * 8 * 9 for (a, b), c in zip(maps, facedet.SOURCE_CHANNELS))
    return 2.0 * macs


def stats_table(directory: str, forwards: int, out_csv):
    paths = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not paths:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    with open(paths[-1], newline="") as f:
        rows = [r for r in csv.DictReader(f) if "det_" in r["Name"] or "det16_" in r["Name"] or "pw_gemm" in r["Name"]]
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    table = [{"kernel": r["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", ""),
              "calls_per_forward": round(float(r["Calls"]) / forwards, 2),
              "us_per_forward": round(float(r["TotalDurationNs"]) / forwards / 1e3, 2),
              "mean_us": round(float(r["AverageNs"]) / 1e3, 2), "share": round(float(r["TotalDurationNs"]) / total, 4)} for r in rows]
    table.sort(key=lambda r: -r["us_per_forward"])
    if out_csv:
        with open(out_csv, "w", newline="") as f:
            wr = csv.DictWriter(f, fieldnames=list(table[0]))
            wr.writeheader()
            wr.writerows(table)
    return table


def timeit(fn, steps: int) -> float:
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,16")
    ap.add_argument("--hw", default="270,480")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--precision", choices=("fp32", "bf16", "both"), default="fp32")
    ap.add_argument("--json")
    ap.add_argument("--stats-from")
    ap.add_argument("--forwards", type=int, default=0)
    ap.add_argument("--csv")
    a = ap.parse_args()
    from calipsync_amd import build
    if a.stats_from:
        if a.forwards <= 0:
            raise SystemExit("--forwards N is needed")
        doc = {"kernels": stats_table(a.stats_from, a.forwards, a.csv)}
        print(json.dumps(doc, indent=1))
        if a.json:
            with open(a.json) as f:
                whole = json.load(f)
            if whole.get("source_hash") != build.source_hash():
                raise SystemExit(f"{a.json} was measured on other kernel sources")
            whole.update(doc)
            with open(a.json, "w") as f:
                json.dump(whole, f, indent=1)
                f.write("\n")
        return

    import torch
    import s3fd_ref
    from calipsync_amd import facedet, recipe
    h, w = (int(v) for v in a.hw.split(","))
    sd = recipe.make_s3fd_state_dict()
    both = a.precision == "both"
    eng = facedet.S3FDEngine(sd, precision="fp32" if both else a.precision)
    eng16 = facedet.S3FDEngine(sd, precision="bf16") if both else None
    if both:
        a.no_baseline = True
    sd_dev = {k: torch.from_numpy(v).cuda() for k, v in sd.items()}
    pr = s3fd_ref.priors(h, w, facedet.map_sizes(h, w)).cuda()
    mean = torch.from_numpy(facedet.IMG_MEAN).cuda()
    lines = []
    for b in (int(v) for v in a.batches.split(",")):
        frames = torch.from_numpy(recipe.make_s3fd_inputs(min(b, 4), h, w)).cuda()
        frames = frames.repeat((b + frames.shape[0] - 1) // frames.shape[0], 1, 1, 1)[:b].contiguous()

        def torch_forward():
            with torch.no_grad():
                x = (frames.float() - mean).permute(0, 3, 1, 2)
                return s3fd_ref.dense(s3fd_ref.network(sd_dev, x, torch.float32), h, w, torch.float32, pr)

        def engine_forward():
            return eng.forward_u8(frames)

        fns = [("engine", engine_forward)] + ([] if a.no_baseline else [("torch", torch_forward)])
        if both:
            fns.append(("bf16", lambda: eng16.forward_u8(frames)))
        for _n, fn in fns:
            for _ in range(a.warmup):
                fn()
        times = {n: [] for n, _ in fns}
        for _ in range(a.rounds):                      # alternating: both see the same clocks and the same neighbours
            for n, fn in fns:
                times[n].append(timeit(fn, a.steps))
        t = statistics.median(times["engine"])
        res = {"batch": b, "hw": [h, w], "precision": eng.precision, "priors": facedet.n_priors(h, w), "engine_ms": t * 1e3, "engine_ms_rounds": [x * 1e3 for x in times["engine"]],
               "frames_per_s": b / t, "launches_per_forward": LAUNCHES, "gflop_per_frame": flops(h, w) / 1e9, "tflops": flops(h, w) * b / t / 1e12}
        if not a.no_baseline:
            tt = statistics.median(times["torch"])
            d = (torch_forward() - engine_forward()).abs().amax(dim=(0, 1))
            res.update({"torch_ms": tt * 1e3, "torch_ms_rounds": [x * 1e3 for x in times["torch"]], "torch_frames_per_s": b / tt,
                        "speedup_vs_torch": tt / t, "max_abs_diff_vs_torch": {"score": float(d[0]), "box": float(d[1:].max())}})
        if both:
            t16 = statistics.median(times["bf16"])
            d = (eng16.forward_u8(frames) - engine_forward()).abs().amax(dim=(0, 1))
            res.update({"bf16_ms": t16 * 1e3, "bf16_ms_rounds": [x * 1e3 for x in times["bf16"]], "bf16_frames_per_s": b / t16,
                        "bf16_tflops": flops(h, w) * b / t16 / 1e12, "speedup_bf16_vs_fp32": t / t16,
                        "max_abs_diff_bf16_vs_fp32": {"score": float(d[0]), "box": float(d[1:].max())}})
        lines.append(res)
        print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"what": "tools/facedet_bench.py " + " ".join(sys.argv[1:]) + " on one MI355X, profiler off",
                       "source_hash": build.source_hash(), "lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
