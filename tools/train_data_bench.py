"""The trainer's batches built on the device from a resident clip against a host loader that does the dataset's work, on one
MI355X, in one process (plus the host loader's worker processes, which never open the GPU).

    python tools/train_data_bench.py [--frames 256] [--height 1080 --width 1920] [--quality 95] [--batches 16,64] [--workers 4,16]
                                     [--rounds 3] [--device-epochs 20] [--json profiles/train_data.json]

A temporary dataset directory is written first (Pillow): ``full_body_img/{i}.jpg`` synthetic noise frames with a plausible
landmark set (tests/frame_data.make_frames; noise compresses badly, so decoding is at its slowest) and ``landmarks/{i}.lms``;
--frames + 1 feature steps, so that an epoch is --frames samples.

    device      calipsync_amd.train_data.TrainingBatches over the clip decoded once by clip_from_dataset_dir: --device-epochs epochs
                a round (an epoch of 256 samples is too short a window), samples per second of wall time up to a device
                synchronise.  The one-time clip build (read, decode, upload) is reported separately, for both decoders.
    host_wN     torch's DataLoader with N worker processes over a Dataset that does what MyDataset.__getitem__ does per sample:
                two files decoded with Pillow (libjpeg, as cv2.imread), two landmark files parsed, the project's host resize
                (oracle/frame_ops_oracle.resize_linear_u8: the same bytes as the kernel; cv2.resize itself is absent here and is
                faster than this numpy restatement, see the per-stage times), the slice, the rectangle, / 255 and the audio window;
                the collated batch is uploaded.  One epoch a round, the SAME (item, reference item) pairs as the device leg's
                first epoch.  The workers are spawned once per (N, batch) and kept; their start-up is not timed.

Each leg is warmed up once, then the legs alternate for --rounds rounds; a line carries the median, the lowest and the highest
round of each leg.  A difference between two legs counts only where it exceeds that spread.  Beside them: the device time of one
casync_op_train_batch call by events, and what one host sample costs stage by stage in this process.

A full training step (forward, loss, backward, optimiser) is NOT timed here: whether the reference's training is bound by its
loader depends on that step, which this tool does not run.  It needs a GPU and does not fall back (--rehearse runs the host side
alone at whatever size is given, for trying the tool out where there is no GPU; it writes no file).
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


class HostDataset:
    """MyDataset.__getitem__ (dataset/dataset.py:136-178) with this project's host pieces; item k is the k-th (idx, ex) pair"""

    def __init__(self, root, n_img, features, pairs):
        self.root, self.n_img, self.features, self.pairs = root, n_img, features, pairs

    def __len__(self):
        return len(self.pairs)

    def stages(self, k, clock=None):
        import numpy as np
        import torch
        from PIL import Image
        from calipsync_amd import frame_loop, train_data
        from oracle.frame_ops_oracle import resize_linear_u8
        tick = (lambda name: None) if clock is None else clock
        idx, ex = self.pairs[k]
        t, r = min(idx, self.n_img - 1), min(ex, self.n_img - 1)
        imgs = []
        for f in (t, r):
            with Image.open(os.path.join(self.root, "full_body_img", f"{f}.jpg")) as im:
                imgs.append(np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1]))
        tick("decode")
        reals = []
        for f, img in zip((t, r), imgs):
            y0, x0, h, w = train_data.dataset_crop_box(train_data.read_lms(os.path.join(self.root, "landmarks", f"{f}.lms")), *img.shape[:2])
            reals.append(resize_linear_u8(img[y0:y0 + h, x0:x0 + w], (168, 168))[4:164, 4:164].copy())
        tick("lms_resize")
        masked = reals[0].copy()
        masked[5:150, 5:155] = 0
        chw = lambda a: torch.from_numpy(a.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0))
        out = (torch.cat([chw(reals[1]), chw(masked)], 0), chw(reals[0]), torch.from_numpy(frame_loop.audio_windows_host(self.features, [t])[0]))
        tick("tensors")
        return out

    def __getitem__(self, k):
        return self.stages(k)


def write_dataset(root, a):
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from frame_data import make_frames
    imgs, lms, _ = make_frames(a.frames, a.height, a.width, seed=12)
    for d in ("full_body_img", "landmarks"):
        os.makedirs(os.path.join(root, d))

    def save(i):
        Image.fromarray(np.ascontiguousarray(imgs[i][:, :, ::-1])).save(os.path.join(root, "full_body_img", f"{i}.jpg"), quality=a.quality)
        np.savetxt(os.path.join(root, "landmarks", f"{i}.lms"), lms[i].astype(np.int32), fmt="%d")
        return os.path.getsize(os.path.join(root, "full_body_img", f"{i}.jpg"))

    with ThreadPoolExecutor(max_workers=16) as pool:
        sizes = list(pool.map(save, range(a.frames)))
    return sum(sizes)


def spread(seconds, samples):
    rate = sorted(samples / s for s in seconds)
    return {"samples_per_s": round(statistics.median(rate), 1), "min_max": [round(rate[0], 1), round(rate[-1], 1)]}


def host_epoch(loader, upload):
    n = 0
    t0 = time.perf_counter()
    for cat, real, audio in loader:
        if upload:
            cat, real, audio = cat.cuda(non_blocking=False), real.cuda(), audio.cuda()
        n += cat.shape[0]
    if upload:
        import torch
        torch.cuda.synchronize()
    return time.perf_counter() - t0, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--workers", default="4,16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--device-epochs", type=int, default=20)
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "train_data.json"))
    a = ap.parse_args()
    if a.rounds < 3:
        raise SystemExit("at least three rounds per leg")
    import numpy as np
    import torch
    from torch.utils.data import DataLoader
    gpu = torch.cuda.is_available()
    if not gpu and not a.rehearse:
        raise SystemExit("tools/train_data_bench.py needs an MI355X: no GPU is visible (there is no fallback)")
    from calipsync_amd import build, train_data

    batches, workers = [int(v) for v in a.batches.split(",")], [int(v) for v in a.workers.split(",")]
    feats = np.random.default_rng(3).standard_normal((a.frames + 1, 2, 1024)).astype(np.float32)
    lines = []

    def say(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        jpeg_bytes = write_dataset(root, a)
        say({"what": "dataset", "frames": a.frames, "frame": [a.height, a.width], "quality": a.quality, "jpeg_MB": round(jpeg_bytes / 2 ** 20, 1),
             "written_in_s": round(time.perf_counter() - t0, 2)})
        pairs = [(int(i), int(e)) for items, refs in train_data.TrainSampler(a.frames, a.frames, max(batches), True, False, seed=21).epoch()
                 for i, e in zip(items, refs)]
        data = HostDataset(root, a.frames, feats, pairs)
        # what one host sample costs, stage by stage, in this process (medians over 8 samples)
        marks = {}
        for k in range(8):
            last = [time.perf_counter()]

            def clock(name):
                now = time.perf_counter()
                marks.setdefault(name, []).append(now - last[0])
                last[0] = now
            data.stages(k, clock)
        say({"what": "host_sample_ms", **{k: round(1e3 * statistics.median(v), 2) for k, v in marks.items()}})

        clip = None
        if gpu:
            for decode in ("host", "device"):
                if clip is not None:
                    clip.close()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                clip = train_data.clip_from_dataset_dir(root, "cuda:0", decode=decode)
                torch.cuda.synchronize()
                say({"what": "clip_build", "decode": decode, "seconds": round(time.perf_counter() - t0, 3),
                     "device_MB": round(a.frames * a.height * a.width * 3 / 2 ** 20, 1)})

        for B in batches:
            loaders = {w: DataLoader(data, batch_size=B, shuffle=False, num_workers=w, persistent_workers=True, multiprocessing_context="spawn")
                       for w in workers}
            legs = {"device": []} if gpu else {}
            legs.update({f"host_w{w}": [] for w in workers})
            dev, first_equal, kernel_ms = None, None, None
            if gpu:
                dev = train_data.TrainingBatches(clip, feats, batch_size=B, seed=21)
                items, refs = [p[0] for p in pairs[:B]], [p[1] for p in pairs[:B]]
                want = dev.batch_for(items, refs)
                got = next(iter(loaders[workers[0]]))
                first_equal = all(torch.equal(g.cuda(), w_) for g, w_ in zip(got, want))
                rec = np.zeros((B, 12), dtype=np.int32)
                rec[:, 0], rec[:, 1:5], rec[:, 5], rec[:, 6:10] = items, dev.boxes[items], refs, dev.boxes[refs]
                ms = []
                for r in range(22):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record()
                    train_data.train_batch(clip.frames, rec)
                    ev[1].record()
                    torch.cuda.synchronize()
                    if r >= 2:
                        ms.append(ev[0].elapsed_time(ev[1]))
                kernel_ms = statistics.median(ms)
            for r in range(a.rounds + 1):                            # round 0 warms every leg up (and starts the workers)
                if gpu:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    n = 0
                    for _ in range(a.device_epochs):
                        for cat, real, audio in dev:
                            n += cat.shape[0]
                    torch.cuda.synchronize()
                    if r:
                        legs["device"].append((time.perf_counter() - t0) / n)
                for w in workers:
                    secs, n = host_epoch(loaders[w], gpu)
                    assert n == a.frames
                    if r:
                        legs[f"host_w{w}"].append(secs / n)
            res = {"what": "legs", "batch": B, "rounds": a.rounds, "samples_per_host_round": a.frames,
                   "samples_per_device_round": a.frames * a.device_epochs, "legs": {k: spread(v, 1) for k, v in legs.items()}}
            if gpu:
                out_bytes = B * 9 * 25600 * 4
                res.update(first_batch_equal=bool(first_equal), train_batch_call_ms=round(kernel_ms, 4),
                           train_batch_store_GBps=round(out_bytes / kernel_ms / 1e6, 1))
            say(res)
            for ld in loaders.values():
                del ld
            loaders.clear()
        if clip is not None:
            clip.close()
    if a.rehearse:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        args = " ".join(f"--{k.replace('_', '-')} {v}" for k, v in sorted(vars(a).items()) if k not in ("json", "rehearse"))
        json.dump({"what": f"tools/train_data_bench.py {args} on one MI355X, profiler off; a full training step was not timed",
                   "source_hash": build.source_hash(), "lines": lines}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
