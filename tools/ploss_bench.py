"""Time the trainer's loss (calipsync_amd.losses.TrainingLoss) against the tests/vgg_ref.py restatement in eager
torch on the same GPU: forward, and forward + backward to the prediction, at B = 16 and 64 of 160 x 160.  The torch legs run in
fp32 and, for information, under bf16 autocast.  The legs alternate (one round = every leg once, ROUNDS rounds); a leg is ITERS
calls between two events behind WARMUP untimed ones; reported: median [min, max] of the rounds, in ms per call.

    python tools/ploss_bench.py [--out profiles/ploss.json] [--batches 16 64] [--rounds 5]

There is no performance bar: whatever this measures is written down as it is."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vgg_ref  # noqa: E402
from calipsync_amd import build, losses, recipe  # noqa: E402

DEV = "cuda:0"
WARMUP, ITERS = 3, 10


def timed(fn) -> float:
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(ITERS):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / ITERS


def legs(batch: int):
    sd = recipe.make_vgg19_state_dict()
    pred, label = (torch.from_numpy(a).to(DEV) for a in recipe.make_loss_inputs(batch))
    ours = losses.TrainingLoss(state_dict=sd, device=DEV)
    ref = vgg_ref.model(sd, torch.float32).to(DEV)

    def engine_fwd():
        with torch.no_grad():
            ours(pred, label)

    def engine_fwd_bwd():
        p = pred.detach().requires_grad_(True)
        ours(p, label)[0].backward()

    def torch_fwd(autocast):
        def run():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                vgg_ref.step_loss(ref, pred, label)
        return run

    def torch_fwd_bwd(autocast):
        def run():
            p = pred.detach().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                loss = vgg_ref.step_loss(ref, p, label)[0]
            loss.backward()
        return run

    return {"engine forward": engine_fwd, "torch fp32 forward": torch_fwd(False), "torch bf16-autocast forward": torch_fwd(True),
            "engine forward+backward": engine_fwd_bwd, "torch fp32 forward+backward": torch_fwd_bwd(False),
            "torch bf16-autocast forward+backward": torch_fwd_bwd(True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ploss.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    result = {"tool": "tools/ploss_bench.py", "device": torch.cuda.get_device_name(0), "source_hash": build.source_hash(), "image": [160, 160],
              "warmup": WARMUP, "iters": ITERS, "rounds": args.rounds, "unit": "ms per call: median [min, max] over the rounds", "batches": {}}
    for batch in args.batches:
        fns = legs(batch)
        times = {name: [] for name in fns}
        for _ in range(args.rounds):
            for name, fn in fns.items():          # the legs alternate
                times[name].append(timed(fn))
        row = {name: {"median": statistics.median(v), "min": min(v), "max": max(v)} for name, v in times.items()}
        for kind in ("forward", "forward+backward"):
            row[f"torch fp32 / engine, {kind}"] = row[f"torch fp32 {kind}"]["median"] / row[f"engine {kind}"]["median"]
        result["batches"][str(batch)] = row
        for name, v in row.items():
            print(f"B={batch:3d} {name:40s} " + (f"{v['median']:8.3f} [{v['min']:.3f}, {v['max']:.3f}] ms" if isinstance(v, dict) else f"{v:.2f}x"), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
