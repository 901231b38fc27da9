"""A clip resident on the device against today's host-staged frame loop, on one MI355X, in one process.

    python tools/resident_clip_bench.py [--frames 256] [--batches 8,64] [--precisions fp32,bf16] [--in-flight 0,1] [--rounds 3]
                                        [--dir-frames 64] [--dir-steps 512] [--dir-batch 16] [--json profiles/resident_clip.json]

Frames are synthetic 1080 x 1920 noise with a plausible landmark set (tests/frame_data.make_frames), weights are the recipe's.
A leg walks the clip once, batch after batch (--frames / B batches), with --in-flight batches left on the GPU while the next
one is submitted (0: each batch is collected at once), and its figure is frames per second of wall time:

    host_copy        frame_loop.submit_batch_device(copy_frames=True)     today's default: new frames, copied on the host
    host_inplace     frame_loop.submit_batch_device(copy_frames=False)    pasted into the caller's own arrays
    resident_views   ResidentClip.submit(...).result()                    one download, frames are views of the pinned block
    resident_copies  the same with the pinned cap forced to 0             one download, then pageable copies
    resident_device  ResidentClip.submit(download=False).result_device()  nothing comes down

Every shape is warmed up once, then the legs alternate for --rounds rounds; a line carries the median, the lowest and the highest
round of each leg.  A difference between two legs counts only where it exceeds that spread.  Beside them: the device time of
gather + compose per batch by events (the two operators alone, 20 repeats), and the bytes a frame moves in each path, computed
from the shapes.

The data-directory pair: a temporary directory of --dir-frames 1080p .jpg frames (Pillow; noise compresses badly, so decoding
is at its slowest), --dir-steps feature steps, FrameSynthesizer(resident=False) against FrameSynthesizer(resident=True), the
first call of each (the resident one reads and uploads the directory in it) and --rounds later calls.

It needs a GPU and does not fall back.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = ("host_copy", "host_inplace", "resident_views", "resident_copies", "resident_device")


def run_leg(leg, net, clip, imgs, inplace, lms, feats_dev, B, in_flight):
    """one walk over the clip -> seconds"""
    import torch
    from calipsync_amd import frame_loop, resident_clip
    n = len(imgs)
    masks = [None] * B
    cap = resident_clip._PINNED_VIEW_CAP
    if leg == "resident_copies":
        resident_clip._PINNED_VIEW_CAP = 0
    pending = []

    def collect(p):
        if leg == "resident_device":
            p[1].synchronize()               # the consumer's kernels would be ordered behind it; here the event stands for them
        else:
            frames = p.result()
            assert len(frames) == B
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for start in range(0, n - B + 1, B):
            idx = list(range(start, start + B))
            if leg == "host_copy":
                p = frame_loop.submit_batch_device(net, imgs[start:start + B], lms[start:start + B], masks, features=feats_dev,
                                                   frame_indices=idx, copy_frames=True)
            elif leg == "host_inplace":
                p = frame_loop.submit_batch_device(net, inplace[start:start + B], lms[start:start + B], masks, features=feats_dev,
                                                   frame_indices=idx, copy_frames=False)
            elif leg == "resident_device":
                out = clip.submit(net, idx, features=feats_dev, frame_indices=idx, download=False).result_device()
                ev = torch.cuda.Event()
                ev.record()
                p = (out, ev)
            else:
                p = clip.submit(net, idx, features=feats_dev, frame_indices=idx)
            pending.append(p)
            while len(pending) > in_flight:
                collect(pending.pop(0))
        while pending:
            collect(pending.pop(0))
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    finally:
        resident_clip._PINNED_VIEW_CAP = cap


def operator_times(clip, B, repeats=20):
    """device ms of gather and of compose for one batch of B frames, by events, medians"""
    import numpy as np
    import torch
    from calipsync_amd import _lib
    lib = _lib.load()
    idx = np.arange(B, dtype=np.int64)
    _, _, rec, reg_total = clip._batch_records(idx)
    regions = torch.empty(reg_total, dtype=torch.uint8, device=clip.frames.device)
    out = torch.empty((B, clip.H, clip.W, 3), dtype=torch.uint8, device=clip.frames.device)
    stream = torch.cuda.current_stream().cuda_stream
    ms = {"gather": [], "compose": []}
    for r in range(repeats + 2):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        _lib.check(lib.casync_op_clip_gather(clip.frames.data_ptr(), len(clip), clip.H, clip.W, rec.ctypes.data, B, regions.data_ptr(),
                                             reg_total, stream), "gather")
        ev[1].record()
        _lib.check(lib.casync_op_clip_compose(clip.frames.data_ptr(), len(clip), clip.H, clip.W, rec.ctypes.data, B, regions.data_ptr(),
                                              reg_total, out.data_ptr(), stream), "compose")
        ev[2].record()
        torch.cuda.synchronize()
        if r >= 2:
            ms["gather"].append(ev[0].elapsed_time(ev[1]))
            ms["compose"].append(ev[1].elapsed_time(ev[2]))
    frame = clip.H * clip.W * 3
    g, c = statistics.median(ms["gather"]), statistics.median(ms["compose"])
    return {"gather_ms": round(g, 4), "compose_ms": round(c, 4), "gather_GBps": round(2 * reg_total / g / 1e6, 1),
            "compose_GBps": round(2 * B * frame / c / 1e6, 1), "region_bytes_per_frame": reg_total // B}


def spread(values, frames):
    fps = sorted(frames / v for v in values)
    return {"fps": round(statistics.median(fps), 1), "fps_min_max": [round(fps[0], 1), round(fps[-1], 1)]}


def data_dir_pair(net, a):
    import numpy as np
    from PIL import Image
    from calipsync_amd.frame_synth import FrameSynthesizer
    from frame_data import make_frames
    imgs, lms, _ = make_frames(a.dir_frames, 1080, 1920, seed=6)
    feats = np.random.default_rng(7).standard_normal((a.dir_steps, 2, 1024)).astype(np.float32)
    with tempfile.TemporaryDirectory() as root:
        for d in ("frames", "positions", "masks"):
            os.makedirs(os.path.join(root, d))
        for i, (img, l) in enumerate(zip(imgs, lms)):
            Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(os.path.join(root, "frames", f"{i:06d}.jpg"), quality=90)
            np.savetxt(os.path.join(root, "positions", f"{i:06d}.txt"), l)
        del imgs
        synth = {r: FrameSynthesizer(None, root, device="cuda:0", batch_size=a.dir_batch, seed=9, net=net, resident=r) for r in (False, True)}
        times = {False: [], True: []}
        for _ in range(a.rounds + 1):
            for r in (False, True):
                t0 = time.perf_counter()
                n = sum(1 for _ in synth[r].iterate_synthesized_frames(feats, 0, True))
                times[r].append(time.perf_counter() - t0)
                assert n == a.dir_steps
    res = {"what": "data_dir", "frames": a.dir_frames, "steps": a.dir_steps, "batch": a.dir_batch, "frame": [1080, 1920], "format": "jpg"}
    for r, name in ((False, "resident_off"), (True, "resident_on")):
        res[name] = dict(spread(times[r][1:], a.dir_steps), first_call_s=round(times[r][0], 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--in-flight", default="0,1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dir-frames", type=int, default=64)
    ap.add_argument("--dir-steps", type=int, default=512)
    ap.add_argument("--dir-batch", type=int, default=16)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "resident_clip.json"))
    a = ap.parse_args()
    if a.rounds < 3:
        raise SystemExit("at least three rounds per leg")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/resident_clip_bench.py needs an MI355X: no GPU is visible (there is no fallback)")
    from calipsync_amd import build, recipe
    from calipsync_amd.resident_clip import REC_WORDS, ResidentClip
    from calipsync_amd.unet import Model
    from frame_data import make_frames

    H, W = 1080, 1920
    imgs, lms, _ = make_frames(a.frames, H, W, seed=5)
    inplace = [im.copy() for im in imgs]
    feats_dev = torch.from_numpy(np.random.default_rng(2).standard_normal((a.frames, 2, 1024)).astype(np.float32)).cuda()
    t0 = time.perf_counter()
    clip = ResidentClip(imgs, lms, None, "cuda:0")
    torch.cuda.synchronize()
    upload_s = time.perf_counter() - t0
    sd = recipe.make_state_dict()
    lines = [{"what": "clip", "frames": a.frames, "frame": [H, W], "device_MB": round(a.frames * H * W * 3 / 2 ** 20, 1),
              "upload_and_geometry_s": round(upload_s, 3)}]
    print(json.dumps(lines[0]), flush=True)
    net = None
    for precision in a.precisions.split(","):
        net = Model(6, "hubert", precision=precision).to("cuda:0")
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
        net.eval()
        for B in [int(v) for v in a.batches.split(",")]:
            ops = operator_times(clip, B)
            frame = H * W * 3
            region = ops["region_bytes_per_frame"]
            moved = {"host_copy": {"up": region, "down": region, "host_copy": 2 * frame, "host_paste": 2 * region},
                     "host_inplace": {"up": region, "down": region, "host_paste": 2 * region},
                     "resident_views": {"up": (12 + 66 + REC_WORDS) * 4, "down": frame, "device_gather": 2 * region, "device_compose": 2 * frame},
                     "resident_copies": {"up": (12 + 66 + REC_WORDS) * 4, "down": frame, "host_copy": 2 * frame, "device_gather": 2 * region,
                                         "device_compose": 2 * frame},
                     "resident_device": {"up": (12 + 66 + REC_WORDS) * 4, "down": 0, "device_gather": 2 * region, "device_compose": 2 * frame}}
            for in_flight in [int(v) for v in a.in_flight.split(",")]:
                secs = {leg: [] for leg in LEGS}
                for r in range(a.rounds + 1):                    # round 0 warms every leg of this shape up
                    for leg in LEGS:
                        t = run_leg(leg, net, clip, imgs, inplace, lms, feats_dev, B, in_flight)
                        if r:
                            secs[leg].append(t)
                n = a.frames // B * B
                res = {"what": "legs", "precision": precision, "batch": B, "in_flight": in_flight, "rounds": a.rounds, "frames_per_leg": n,
                       "legs": {leg: spread(secs[leg], n) for leg in LEGS}, "gather_compose": ops, "bytes_per_frame": moved}
                lines.append(res)
                print(json.dumps(res), flush=True)
    clip.close()
    res = data_dir_pair(net, a)
    res["precision"] = a.precisions.split(",")[-1]
    lines.append(res)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        args = " ".join(f"--{k.replace('_', '-')} {v}" for k, v in sorted(vars(a).items()) if k != "json")
        json.dump({"what": f"tools/resident_clip_bench.py {args} on one MI355X, profiler off",
                   "source_hash": build.source_hash(), "lines": lines}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
