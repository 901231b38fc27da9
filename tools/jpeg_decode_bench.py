"""JPEG files into frames on the device against today's Pillow decode and raw upload, on one MI355X, in one process.

    python tools/jpeg_decode_bench.py [--frames 64] [--quality 95] [--contents smooth,noise] [--rounds 3] [--threads 16]
                                      [--chunks 256,512,1024,2048] [--json profiles/jpeg_decode.json]

The files are synthetic 1080 x 1920 frames (tools/jpeg_bench.py's two contents: `smooth`, a shifting gradient with a noise patch,
of the order of camera footage, and `noise`, uniform noise, the adverse case) written by Pillow at the given quality with its
defaults: 4:2:0, Annex K tables, no restart markers, what the reference's step 3 writes.  Per content:

    1  device      jpeg.decode_jpeg_device(files): parse, plan, one pinned upload of the compressed bytes, the kernels   wall ms
    2  kernels     casync_op_jpegdec_decode alone on bytes already on the device, by events, per chunk_bits of --chunks  device ms
    3  pillow      Pillow decode of the same bytes on --threads host threads and the raw upload through one reused pinned
                   stage, UPLOAD_CHUNK frames at a time: the decode and upload of from_data_dir today, without its file reads  wall ms
    4  clip        ResidentClip.from_data_dir on a directory of the files, decode="device" and decode="host"              wall ms

Every leg is warmed up once, then the legs alternate for --rounds rounds; a line carries the median, the lowest and the highest
round (leg 2: the settings of --chunks alternate the same way, each figure the median of three calls).  A difference between two
legs counts only where it exceeds that spread.  Leg 2 is one figure for the four kernels and the memset together: the entry
enqueues them in one call.  The split per kernel comes from a profiler run of its own,
``rocprofv3 --kernel-trace --stats -- python tools/jpeg_decode_bench.py --kernels-only --contents smooth``.  Beside them the
rounds the entropy plan needed on the first file at the default chunk_bits (the host model, jpeg.sync_states).

It needs a GPU and does not fall back.
"""
from __future__ import annotations

import argparse
import io
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
    """casync_op_jpegdec_decode on a batch whose bytes are already on the device, at one chunk_bits"""

    def __init__(self, files, chunk_bits):
        import torch
        from calipsync_amd import _lib, jpeg
        self.plan = jpeg.plan_decode(files, chunk_bits)
        need = _lib.load().casync_op_jpegdec_workspace_bytes(len(files), H, W, self.plan.subsampling, self.plan.total_sub)
        self.data = torch.from_numpy(self.plan.blob.copy()).cuda()
        self.scratch = torch.empty(need, dtype=torch.uint8, device="cuda:0")
        self.out = torch.empty((len(files), H, W, 3), dtype=torch.uint8, device="cuda:0")
        self.status = torch.empty(len(files), dtype=torch.int32, device="cuda:0")

    def ms(self, repeats=3):
        """device ms of one call by events: the median of `repeats`"""
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
    ap.add_argument("--chunks", default="256,512,1024,2048")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "jpeg_decode.json"))
    ap.add_argument("--kernels-only", action="store_true", help="only the decode call at the default chunk_bits, six times: for a profiler run")
    a = ap.parse_args()
    if a.rounds < 3:
        raise SystemExit("at least three rounds per leg")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/jpeg_decode_bench.py needs an MI355X: no GPU is visible (there is no fallback)")
    from PIL import Image
    import jpeg_bench
    from calipsync_amd import build, frame_loop, jpeg
    from calipsync_amd.resident_clip import UPLOAD_CHUNK, ResidentClip
    from frame_data import make_frames

    _, lms, _ = make_frames(1, H, W, seed=5)
    pool = ThreadPoolExecutor(max_workers=a.threads)

    def write(frame):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(buf, format="JPEG", quality=a.quality)
        return buf.getvalue()

    lines = []
    for kind in a.contents.split(","):
        files = list(pool.map(write, jpeg_bench.make_content(kind, a.frames)))
        B = len(files)
        if a.kernels_only:                                     # for a profiler run of its own: the default chunk_bits, nothing else
            k = Kernels(files, 0)
            print(json.dumps({"content": kind, "files": B, "chunk_bits": k.plan.chunk_bits, "ms": [round(k.ms(1), 3) for _ in range(6)]}), flush=True)
            continue
        chunks = [int(v) for v in a.chunks.split(",")]
        sweep_ms = {c: [] for c in chunks}
        for r in range(a.rounds + 1):                          # round 0 warms up; the settings alternate (their buffers do not live side by side)
            for c in chunks:
                k = Kernels(files, c)
                k.ms(1)
                t = k.ms(3)
                subs = k.plan.total_sub
                del k
                if r:
                    sweep_ms[c].append(t)
                sweep_ms[(c, "subs")] = subs
        sweep = {str(c): dict(spread(sweep_ms[c]), frames_per_s=round(B / statistics.median(sweep_ms[c]) * 1e3, 1), subsequences=sweep_ms[(c, "subs")])
                 for c in chunks}
        with tempfile.TemporaryDirectory() as root:
            for d in ("frames", "positions", "masks"):
                os.makedirs(os.path.join(root, d))
            for i, f in enumerate(files):
                with open(os.path.join(root, "frames", f"{i:06d}.jpg"), "wb") as fh:
                    fh.write(f)
                np.savetxt(os.path.join(root, "positions", f"{i:06d}.txt"), lms[0])

            def leg(name):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "device":
                    out = jpeg.decode_jpeg_device(files, fallback="raise")
                elif name == "pillow":                         # as ResidentClip._upload: UPLOAD_CHUNK frames at a time through one reused pinned stage
                    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda:0")
                    stage = frame_loop._acquire_pinned(min(B, UPLOAD_CHUNK) * H * W * 3)
                    for at in range(0, B, UPLOAD_CHUNK):
                        frames = list(pool.map(jpeg._decode_pillow, files[at:at + UPLOAD_CHUNK]))
                        torch.cuda.synchronize()
                        view = stage[:len(frames) * H * W * 3].view(len(frames), H, W, 3)
                        np.stack(frames, out=view.numpy())
                        out[at:at + len(frames)].copy_(view, non_blocking=True)
                    torch.cuda.synchronize()
                    frame_loop._release_pinned(stage)
                else:
                    out = ResidentClip.from_data_dir(root, "cuda:0", io_workers=a.threads, decode=name[5:]).frames
                torch.cuda.synchronize()
                assert tuple(out.shape) == (B, H, W, 3)
                return (time.perf_counter() - t0) * 1e3

            ms = {name: [] for name in ("device", "pillow", "clip_device", "clip_host")}
            for r in range(a.rounds + 1):                      # round 0 warms every leg up
                for name in ms:
                    t = leg(name)
                    if r:
                        ms[name].append(t)
        # the host model walks every symbol in Python: only for files of footage size
        sync = jpeg.sync_states(jpeg.parse_jpeg(files[0]), files[0]) if len(files[0]) <= (1 << 20) else None
        res = {"content": kind, "files": B, "quality": a.quality, "frame": [H, W], "rounds": a.rounds, "host_threads": a.threads,
               "mean_file_bytes": sum(len(f) for f in files) // B, "raw_bytes": H * W * 3, "default_chunk_bits": jpeg.DEFAULT_CHUNK_BITS,
               "kernels_by_chunk_bits": sweep,
               "plan_rounds_first_file": None if sync is None else {"rounds": sync.total_rounds, "subsequences": int(sync.rounds.size),
                                                                    "needed_more_than_two": int((sync.rounds > 2).sum())}}
        for key, name in (("1_device", "device"), ("3_pillow_upload", "pillow"), ("4_clip_device", "clip_device"), ("4_clip_host", "clip_host")):
            res[key] = dict(spread(ms[name]), frames_per_s=round(B / statistics.median(ms[name]) * 1e3, 1))
        lines.append(res)
        print(json.dumps(res), flush=True)
    if a.kernels_only:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        args = " ".join(f"--{k.replace('_', '-')} {v}" for k, v in sorted(vars(a).items()) if k not in ("json", "kernels_only") and v is not None)
        json.dump({"what": f"tools/jpeg_decode_bench.py {args} on one MI355X, profiler off", "source_hash": build.source_hash(), "lines": lines}, f,
                  indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
