"""HuBERT-large feature extraction throughput on one MI355X: the HIP engine (fp32, bf16 or both) against the same model
restated in torch (tests/hubert_ref.py) on the same GPU, in one process.

    python tools/hubert_bench.py [--layers 24] [--steps 5] [--warmup 2] [--precision fp32|bf16|both]

Two shapes: one full chunk (B=1, 320080 samples = 1000 tokens) and a 60-s clip (its three full chunks in one batched
forward, as HubertExtractor runs them).  One JSON line per shape: audio-seconds/s, tokens/s, achieved TFLOP/s on the
FLOPs counted from shapes (flops() below) and its fraction of the 157.3 TFLOP/s fp32 matrix roof, for the engine and
the torch baseline.  --precision bf16 / both: the bf16 handle's line is measured against the 2.5 PFLOP/s bf16 matrix
roof and carries `speedup_vs_fp32`, its time against the fp32 engine's in the same process (with `both` the two engines'
timed steps alternate; with `bf16` alone the fp32 engine is timed too, only its line is not printed).  Per-kernel times: run
this under rocprofv3 --kernel-trace --stats.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

ROOF_TF = 157.3   # MI355X fp32 matrix peak, TFLOP/s
ROOF_TF_BF16 = 2500.0   # ... and the bf16 one


def flops(samples: int, layers: int) -> float:
    """2 x multiply-adds of one waveform of `samples` samples: the seven convs, the feature projection, the positional
    conv and, per layer, the q/k/v, out and FFN GEMMs plus attention (QK^T and PV)."""
    from calipsync_amd import hubert
    t, f = samples, 0.0
    for i, (k, s) in enumerate(zip((10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2))):
        t = (t - k) // s + 1
        f += 2.0 * t * 512 * (1 if i == 0 else 512) * k
    T = hubert.tokens(samples)
    f += 2.0 * T * 512 * 1024                       # feature projection
    f += 2.0 * T * 1024 * 64 * 128                  # positional conv (16 groups: 64 in -> 64 out, 128 taps)
    per_layer = 2.0 * T * 1024 * (3 * 1024 + 1024 + 2 * 4096) + 2.0 * 2 * T * T * 1024
    return f + layers * per_layer


def timeit(fn, steps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def timeit_alternating(fns, steps: int, warmup: int):
    """Per-call seconds of each of `fns`, their timed steps taken in turn (a, b, a, b, ...) so that clocks and thermals
    treat them alike; each call is timed between two device synchronisations."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    tot = [0.0] * len(fns)
    for _ in range(steps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            tot[i] += time.perf_counter() - t0
    return [t / steps for t in tot]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--shapes", default="chunk,clip60s", help="comma-separated subset of chunk,clip60s")
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16", "both"))
    a = ap.parse_args()
    import hubert_ref
    from calipsync_amd import hubert
    sd = hubert_ref.recipe_state_dict(a.layers)
    eng = hubert.HubertEngine(sd, a.layers)
    eng16 = hubert.HubertEngine(sd, a.layers, precision="bf16") if a.precision != "fp32" else None
    # the baseline: the restatement with its weights already on the GPU
    P = {k: torch.from_numpy(v).cuda() for k, v in hubert.packed_tensors(sd, a.layers).items()}
    hubert_ref._t = lambda x: x if isinstance(x, torch.Tensor) else torch.as_tensor(x)

    def torch_forward(w):
        with torch.no_grad():
            return hubert_ref.forward(P, a.layers, w)

    for name, b in (("chunk", 1), ("clip60s", 3)):
        if name not in a.shapes.split(","):
            continue
        w = torch.stack([torch.from_numpy(hubert.normalize(hubert_ref.golden_wave(hubert.CHUNK, 50 + i))) for i in range(b)]).cuda()
        f = b * flops(hubert.CHUNK, a.layers)
        audio_s = b * hubert.CLIP / 16000.0
        tok = b * hubert.tokens(hubert.CHUNK)
        if eng16 is not None:
            t_eng, t16 = timeit_alternating([lambda: eng(w), lambda: eng16(w)], a.steps, a.warmup)
            print(json.dumps({"shape": name, "precision": "bf16", "batch": b, "samples": hubert.CHUNK, "layers": a.layers,
                              "gflop": round(f / 1e9, 1), "engine_ms": t16 * 1e3, "audio_s_per_s": audio_s / t16,
                              "tokens_per_s": tok / t16, "tflops": f / t16 / 1e12, "roof_frac": f / t16 / 1e12 / ROOF_TF_BF16,
                              "fp32_engine_ms": t_eng * 1e3, "speedup_vs_fp32": t_eng / t16}), flush=True)
            if a.precision == "bf16":
                continue
        else:
            t_eng = timeit(lambda: eng(w), a.steps, a.warmup)
        res = {"shape": name, "precision": "fp32", "batch": b, "samples": hubert.CHUNK, "layers": a.layers, "gflop": round(f / 1e9, 1),
               "engine_ms": t_eng * 1e3, "audio_s_per_s": audio_s / t_eng, "tokens_per_s": tok / t_eng,
               "tflops": f / t_eng / 1e12, "roof_frac": f / t_eng / 1e12 / ROOF_TF}
        if not a.no_baseline:
            t_ref = timeit(lambda: torch_forward(w), a.steps, a.warmup)
            res.update({"torch_ms": t_ref * 1e3, "torch_audio_s_per_s": audio_s / t_ref, "torch_tflops": f / t_ref / 1e12,
                        "speedup_vs_torch": t_ref / t_eng})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
