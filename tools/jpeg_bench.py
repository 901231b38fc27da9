"""Finished frames off the device as JPEG files against today's raw download and Pillow encode, on one MI355X, in one process.

    python tools/jpeg_bench.py [--frames 64] [--batches 16,64] [--quality 95] [--contents smooth,noise] [--rounds 3] [--threads 16]
                               [--json profiles/jpeg_bench.json] [--subsampling 4:4:4,4:2:0]

Frames are synthetic 1080 x 1920, resident on the device (ResidentClip; no network runs: a batch is ``clip.fetch``, the compose
of stored frames, so the figures are those of getting finished frames off the device and nothing else).  Two contents: `smooth`,
a gradient that shifts from frame to frame with a 200 x 400 noise patch (file sizes of the order of camera footage), and `noise`,
uniform noise (the encoder's worst ordinary case: every coefficient is coded).  Per content and batch size B, per batch:

    a  kernels     casync_op_jpeg_encode alone, device ms by events (median of 10)
    b  jpeg        fetch(download=False).result_jpeg(q): compose, encode, two small downloads                      wall ms
    c  raw_pillow  fetch().result() and mjpeg_avi.encode_jpeg of every frame on --threads host threads (today)     wall ms
    d  raw         fetch().result() alone: the raw download                                                        wall ms

Every leg is warmed up once, then the legs alternate for --rounds rounds; a line carries the median, the lowest and the highest
round.  A difference between two legs counts only where it exceeds that spread.  Beside them the mean JPEG size of a frame.
Legs b, c and d produce the same files for the same frames up to Pillow's missing restart markers (b's bytes are checked against
the numpy twin in tests/test_jpeg_gpu.py, not here).

With ``--subsampling 4:4:4,4:2:0`` the tool compares the chroma samplings of the encoder instead (the
default --json becomes profiles/jpeg420_bench.json): per content and B only legs a and b, once per setting, the settings
alternating within each round on the same frames, and per setting the mean file size.

It needs a GPU and does not fall back.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 1080, 1920


def make_content(kind, n):
    import numpy as np
    rng = np.random.default_rng(11)
    if kind == "noise":
        return [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(n)]
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    frames = []
    for i in range(n):
        chans = [40 + 170 * (a * x / (W - 1) + (1 - a) * y / (H - 1)) + 12 * np.sin((x + 7 * i) / 9.0 + p) for a, p in ((0.2, 0.0), (0.5, 1.0), (0.8, 2.0))]
        f = np.clip(np.stack(chans, axis=2), 0, 255).astype(np.uint8)
        f[440:640, 760:1160] = rng.integers(0, 256, (200, 400, 3), dtype=np.uint8)
        frames.append(f)
    return frames


def kernel_ms(frames_dev, quality, repeats=10, subsampling="4:4:4"):
    """device ms of one casync_op_jpeg_encode (casync_op_jpeg420_encode) on the batch, by events: the median"""
    import torch
    from calipsync_amd import _lib, jpeg
    B = int(frames_dev.shape[0])
    rows = jpeg.restart_rows(H, subsampling)
    slot = jpeg.default_slot_bytes(W, subsampling)
    need = getattr(_lib.load(), jpeg._entry("workspace_bytes", jpeg._subsampling(subsampling)))(B, H, W, 0)
    dev = frames_dev.device
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(B * (jpeg.HEADER_BYTES + rows * slot), dtype=torch.uint8, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    ms = []
    for r in range(repeats + 2):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        jpeg.encode_jpeg_op(frames_dev, quality, 0, scratch, out, offsets, status, subsampling)
        ev[1].record()
        torch.cuda.synchronize()
        if r >= 2:
            ms.append(ev[0].elapsed_time(ev[1]))
    assert int(status.abs().sum()) == 0
    return statistics.median(ms), int(offsets[B]) / B


def spread(values):
    v = sorted(values)
    return {"ms": round(statistics.median(v), 3), "ms_min_max": [round(v[0], 3), round(v[-1], 3)]}


def compare_settings(clip, idx, kind, settings, a):
    """legs a and b of every chroma sampling in `settings` on one batch: round 0 warms up, then the settings alternate"""
    import torch
    B = len(idx)
    frames_dev = clip.fetch(idx, download=False).result_device()
    k_ms, j_ms, size = ({s: [] for s in settings} for _ in range(3))
    for r in range(a.rounds + 1):
        for s in settings:
            k, mean_bytes = kernel_ms(frames_dev, a.quality, subsampling=s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            files = clip.fetch(idx, download=False).result_jpeg(a.quality, s)
            t = (time.perf_counter() - t0) * 1e3
            assert len(files) == B and sum(len(f) for f in files) == round(mean_bytes * B)
            if r:
                k_ms[s].append(k)
                j_ms[s].append(t)
                size[s] = int(mean_bytes)
    res = {"what": "subsampling", "content": kind, "batch": B, "quality": a.quality, "frame": [H, W], "rounds": a.rounds,
           "raw_bytes": H * W * 3, "settings": {}}
    for s in settings:
        res["settings"][s] = {"mean_jpeg_bytes": size[s],
                              "a_kernels": dict(spread(k_ms[s]), frames_per_s=round(B / statistics.median(k_ms[s]) * 1e3, 1)),
                              "b_jpeg": dict(spread(j_ms[s]), frames_per_s=round(B / statistics.median(j_ms[s]) * 1e3, 1))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--contents", default="smooth,noise")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--json", default=None)
    ap.add_argument("--subsampling", default=None, help="e.g. 4:4:4,4:2:0: compare the encoder's chroma samplings (legs a and b only)")
    a = ap.parse_args()
    if a.json is None:
        a.json = os.path.join(ROOT, "profiles", "jpeg420_bench.json" if a.subsampling else "jpeg_bench.json")
    settings = a.subsampling.split(",") if a.subsampling else None
    if a.rounds < 3:
        raise SystemExit("at least three rounds per leg")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/jpeg_bench.py needs an MI355X: no GPU is visible (there is no fallback)")
    from calipsync_amd import build, mjpeg_avi
    from calipsync_amd.resident_clip import ResidentClip
    from frame_data import make_frames

    _, lms, _ = make_frames(1, H, W, seed=5)
    pool = ThreadPoolExecutor(max_workers=a.threads)
    lines = []
    for kind in a.contents.split(","):
        imgs = make_content(kind, a.frames)
        clip = ResidentClip(imgs, [lms[0]] * a.frames, None, "cuda:0")
        del imgs
        for B in [int(v) for v in a.batches.split(",")]:
            if B > a.frames:
                continue
            idx = list(range(B))
            if settings:
                lines.append(compare_settings(clip, idx, kind, settings, a))
                print(json.dumps(lines[-1]), flush=True)
                continue
            k_ms, mean_bytes = kernel_ms(clip.fetch(idx, download=False).result_device(), a.quality)

            def leg(name):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "jpeg":
                    n = len(clip.fetch(idx, download=False).result_jpeg(a.quality))
                else:
                    frames = clip.fetch(idx).result()
                    n = len(list(pool.map(lambda f: mjpeg_avi.encode_jpeg(f, a.quality), frames)) if name == "raw_pillow" else frames)
                    del frames
                assert n == B
                return (time.perf_counter() - t0) * 1e3
            ms = {name: [] for name in ("jpeg", "raw_pillow", "raw")}
            for r in range(a.rounds + 1):                      # round 0 warms every leg up
                for name in ms:
                    t = leg(name)
                    if r:
                        ms[name].append(t)
            res = {"what": "legs", "content": kind, "batch": B, "quality": a.quality, "frame": [H, W], "rounds": a.rounds,
                   "host_threads": a.threads, "mean_jpeg_bytes": int(mean_bytes), "raw_bytes": H * W * 3,
                   "a_kernels": {"ms": round(k_ms, 3), "frames_per_s": round(B / k_ms * 1e3, 1)}}
            for key, name in (("b_jpeg", "jpeg"), ("c_raw_pillow", "raw_pillow"), ("d_raw", "raw")):
                res[key] = dict(spread(ms[name]), frames_per_s=round(B / statistics.median(ms[name]) * 1e3, 1))
            lines.append(res)
            print(json.dumps(res), flush=True)
        clip.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        args = " ".join(f"--{k.replace('_', '-')} {v}" for k, v in sorted(vars(a).items()) if k != "json" and v is not None)
        json.dump({"what": f"tools/jpeg_bench.py {args} on one MI355X, profiler off", "source_hash": build.source_hash(), "lines": lines}, f,
                  indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
