"""A Motion-JPEG AVI file into frames on the device, through the wider decoder against Pillow and upload, on one MI355X, in one
process; kin of tools/jpeg_decode_bench.py.

    python tools/video_io_bench.py [--frames 64] [--quality 95] [--contents smooth,noise] [--rounds 3] [--threads 16]
                                   [--json profiles/video_io.json]

Per content (tools/jpeg_bench.py's `smooth`, of the order of camera footage, and `noise`, uniform noise, the adverse case) the
1080 x 1920 frames are written by Pillow at the given quality as 4:2:2 and as 4:2:0, each with its Huffman tables and with
every DHT segment taken out (the MJPG convention), into an AVI file with mjpeg_avi.write_mjpeg_avi.  Per file, to a device tensor
[frames, 1080, 1920, 3]:

    1  mjpeg     mjpeg_avi.read_avi + jpeg.decode_jpeg_device(subset="mjpeg", fallback="raise")                       wall ms
    2  pillow    mjpeg_avi.read_avi + Pillow on --threads host threads + the raw upload through one reused pinned stage,
                 UPLOAD_CHUNK frames at a time (what decode="host" costs, and what such files cost before this decoder)  wall ms
    3  baseline  4:2:0 with its tables only: read_avi + decode_jpeg_device(subset="baseline"), the specialised kernels     wall ms
    4  kernels   casync_op_mjpegdec_decode (and, 4:2:0 with tables, casync_op_jpegdec_decode) alone on bytes already on
                 the device, by events, at the default chunk_bits                                                      device ms

Every leg is warmed up once, then the legs alternate for --rounds rounds; a line carries the median, the lowest and the highest
round.  A difference between two legs counts only where it exceeds that spread.

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
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W = 1080, 1920


def spread(values):
    v = sorted(values)
    return {"ms": round(statistics.median(v), 3), "ms_min_max": [round(v[0], 3), round(v[-1], 3)]}


class Kernels:
    """one decode entry on a batch whose bytes are already on the device, at the default chunk_bits"""

    def __init__(self, files, subset):
        import torch
        from calipsync_amd import jpeg
        self.plan = jpeg.plan_decode(files, 0, subset=subset)
        need = jpeg.workspace_bytes(self.plan, len(files), H, W)
        self.data = torch.from_numpy(self.plan.blob.copy()).cuda()
        self.scratch = torch.empty(need, dtype=torch.uint8, device="cuda:0")
        self.out = torch.empty((len(files), H, W, 3), dtype=torch.uint8, device="cuda:0")
        self.status = torch.empty(len(files), dtype=torch.int32, device="cuda:0")

    def ms(self, repeats=3):
        import torch
        from calipsync_amd import jpeg
        ms = []
        for _ in range(repeats):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            jpeg.decode_jpeg_op(self.plan, self.data, self.scratch, self.out, self.status)
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        assert int(self.status.abs().sum()) == 0
        return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--contents", default="smooth,noise")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "video_io.json"))
    a = ap.parse_args()
    if a.rounds < 3:
        raise SystemExit("at least three rounds per leg")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/video_io_bench.py needs an MI355X: no GPU is visible (there is no fallback)")
    import jpeg_bench
    import mjpeg_decode_cases as mj
    from calipsync_amd import build, frame_loop, jpeg, mjpeg_avi
    from calipsync_amd.resident_clip import UPLOAD_CHUNK

    gen = mj.generator()
    pool = ThreadPoolExecutor(max_workers=a.threads)
    lines = []
    with tempfile.TemporaryDirectory() as root:
        for kind in a.contents.split(","):
            content = list(jpeg_bench.make_content(kind, a.frames))
            B = len(content)
            for sampling in ("422", "420"):
                whole = list(pool.map(lambda f: gen.pillow_write(f, sampling, quality=a.quality), content))
                for dht in (True, False):
                    files = whole if dht else [gen.strip_dht(f) for f in whole]
                    path = os.path.join(root, f"{kind}_{sampling}_{int(dht)}.avi")
                    mjpeg_avi.write_mjpeg_avi(path, files, fps=25)
                    legs = ["mjpeg", "pillow"] + (["baseline"] if sampling == "420" and dht else [])

                    def leg(name):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        clip = mjpeg_avi.read_avi(path)
                        if name == "pillow":                   # as ResidentClip._upload: UPLOAD_CHUNK frames through one reused pinned stage
                            out = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda:0")
                            stage = frame_loop._acquire_pinned(min(B, UPLOAD_CHUNK) * H * W * 3)
                            for at in range(0, B, UPLOAD_CHUNK):
                                frames = list(pool.map(jpeg._decode_pillow, clip.frames[at:at + UPLOAD_CHUNK]))
                                torch.cuda.synchronize()
                                view = stage[:len(frames) * H * W * 3].view(len(frames), H, W, 3)
                                np.stack(frames, out=view.numpy())
                                out[at:at + len(frames)].copy_(view, non_blocking=True)
                            torch.cuda.synchronize()
                            frame_loop._release_pinned(stage)
                        else:
                            out = jpeg.decode_jpeg_device(clip.frames, fallback="raise", subset=name)
                        torch.cuda.synchronize()
                        assert tuple(out.shape) == (B, H, W, 3)
                        return (time.perf_counter() - t0) * 1e3

                    ms = {name: [] for name in legs}
                    for r in range(a.rounds + 1):              # round 0 warms every leg up
                        for name in legs:
                            t = leg(name)
                            if r:
                                ms[name].append(t)
                    kern = {}
                    for subset in ("mjpeg",) + (("baseline",) if "baseline" in legs else ()):
                        kern[subset] = []
                    for r in range(a.rounds + 1):
                        for subset in kern:
                            k = Kernels(files, subset)
                            k.ms(1)
                            t = k.ms(3)
                            del k
                            if r:
                                kern[subset].append(t)
                    res = {"content": kind, "sampling": sampling, "dht": dht, "files": B, "quality": a.quality, "frame": [H, W], "rounds": a.rounds,
                           "host_threads": a.threads, "mean_file_bytes": sum(len(f) for f in files) // B, "avi_bytes": os.path.getsize(path),
                           "raw_bytes": H * W * 3}
                    for name in legs:
                        res[name] = dict(spread(ms[name]), frames_per_s=round(B / statistics.median(ms[name]) * 1e3, 1))
                    for subset, v in kern.items():
                        res["kernels_" + subset] = dict(spread(v), frames_per_s=round(B / statistics.median(v) * 1e3, 1))
                    lines.append(res)
                    print(json.dumps(res), flush=True)
                    os.remove(path)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        args = " ".join(f"--{k.replace('_', '-')} {v}" for k, v in sorted(vars(a).items()) if k != "json" and v is not None)
        json.dump({"what": f"tools/video_io_bench.py {args} on one MI355X, profiler off", "source_hash": build.source_hash(), "lines": lines}, f,
                  indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
