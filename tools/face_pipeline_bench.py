"""Frames to landmarks on one MI355X: the host path (LandmarkDetector.detect_landmarks with an S3FDDetector, every resize and
crop on the CPU) against the device path (detect_landmarks_device) from host frames and from frames already resident, in one
process, alternating, with per-stage times of the device path.

    python tools/face_pipeline_bench.py [--batches 1,8,16] [--precisions fp32,bf16] [--rounds 7] [--warmup 2] [--json FILE]

Frames: the recipe's 270 x 480 detector frames (recipe.make_s3fd_inputs) tiled 4 x 4 pixel-wise to 1080 x 1920, so the detector
at the reference's scale 0.25 sees recipe frames; weights are the recipes' (synthetic), so the number of "faces" per frame is
whatever those weights give -- it is printed, and PFLD's share of the time scales with it.  --max-faces keeps only the first
N boxes of a frame in BOTH paths (a wrapper around the detector), 0 keeps all.

One JSON line per (precision, batch): medians over --rounds of host_ms, device_from_host_ms, device_resident_ms, which library
did the host path's resizes (cv2 or Pillow: different arithmetic from the device path's, so the landmarks are compared only as
a count), and the stages of the device path, each timed on its own between synchronisations: upload, downscale, s3fd,
candidates_nms (compaction, download, host NMS), crops, pfld, finalize (with its download).  Stage times carry a
synchronisation each and do not add up to the end-to-end figure exactly.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def resize_library() -> str:
    try:
        import cv2  # noqa: F401
        return "cv2"
    except ImportError:
        return "Pillow"


class FirstFaces:
    """the detector with at most n boxes per frame, in both its host and its device form"""

    def __init__(self, det, n):
        self.det, self.n = det, n

    def _cut(self, detections):
        return [(b[:self.n], i[:self.n]) if self.n and len(i) > self.n else (b, i) for b, i in detections]

    def detect_device(self, frames):
        return self._cut(self.det.detect_device(frames))

    def __call__(self, images):
        return [[tuple(float(v) for v in box) for box in boxes] for boxes, _ in self._cut(self.det.detect(images))]


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stages(lm, det, frames_host):
    """one pass of the device path, stage by stage -> {stage: ms}"""
    import numpy as np
    import torch
    from calipsync_amd import face_ops, facedet
    t = {}
    t["upload"], dev = timed(lambda: det.frames_to_device(frames_host))
    t["downscale"], small = timed(lambda: face_ops.resize_frames_u8(dev, fx=det.scale))
    t["s3fd"], dense = timed(lambda: det.det_net.forward_u8(small))

    def nms():
        counts_dev, rows_dev = face_ops.s3fd_candidates(dense, facedet.CONF_THRESH, min(det.candidate_cap, dense.shape[1]))
        counts = counts_dev.cpu().numpy()
        rows = rows_dev[:, :max(1, min(int(counts.max()), rows_dev.shape[1]))].cpu().numpy()
        return [facedet.detect_faces_rows(facedet.detect_output(rows[i, :min(int(c), rows.shape[1])][None])[0], dev.shape[2], dev.shape[1],
                                          det.conf_threshold) for i, c in enumerate(counts)], counts

    t["candidates_nms"], (rows, counts) = timed(nms)
    boxes = [[(r[0], r[1], r[2] - r[0], r[3] - r[1]) for r in fr] for fr in rows]
    if lm.face_detector.n:
        boxes = [b[:lm.face_detector.n] for b in boxes]
    table = np.asarray([(i,) + lm._crop_geometry(dev.shape[1], dev.shape[2], b) for i, bs in enumerate(boxes) for b in bs], dtype=np.int32)
    if len(table) == 0:
        return t, counts, 0
    t["crops"], crops = timed(lambda: face_ops.face_crops192(dev, table))
    t["pfld"], y = timed(lambda: lm.pfld_backbone.forward_u8(crops))
    mean = torch.from_numpy(lm.mean_face).to(dev.device)
    t["finalize"], _ = timed(lambda: face_ops.landmarks_finalize(y, mean, table).cpu())
    return t, counts, len(table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,16")
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-faces", type=int, default=0)
    ap.add_argument("--json")
    a = ap.parse_args()
    import numpy as np
    import torch
    from calipsync_amd import build, facedet, landmarks, recipe
    if not torch.cuda.is_available():
        raise SystemExit("face_pipeline_bench: no GPU; nothing is measured on a CPU")
    lm = landmarks.LandmarkDetector(state_dict=recipe.make_pfld_state_dict(), mean_face=np.full(220, 0.5, np.float32))
    sd = recipe.make_s3fd_state_dict()
    lines = []
    for precision in a.precisions.split(","):
        det = facedet.S3FDDetector(state_dict=sd, precision=precision)
        lm.face_detector = FirstFaces(det, a.max_faces)
        for b in [int(v) for v in a.batches.split(",")]:
            small = recipe.make_s3fd_inputs(min(b, 4), 270, 480)
            small = np.concatenate([small] * ((b + len(small) - 1) // len(small)))[:b]
            frames = list(np.repeat(np.repeat(small, 4, 1), 4, 2))
            resident = torch.from_numpy(np.stack(frames)).cuda()
            runs = {"host": lambda: lm.detect_landmarks(frames), "device_from_host": lambda: lm.detect_landmarks_device(frames),
                    "device_resident": lambda: lm.detect_landmarks_device(resident)}
            ms = {k: [] for k in runs}
            st = {}
            faces = {}
            for r in range(a.warmup + a.rounds):
                for k, fn in runs.items():               # alternating: a drift of the box hits all three alike
                    t, out = timed(fn)
                    faces[k] = sum(len(f) for f in out if f is not None)
                    if r >= a.warmup:
                        ms[k].append(t)
                ts, counts, n_crops = stages(lm, det, frames)
                if r >= a.warmup:
                    for k, v in ts.items():
                        st.setdefault(k, []).append(v)
            med = {k: statistics.median(v) for k, v in ms.items()}
            res = {"precision": precision, "batch": b, "frame": [1080, 1920], "host_resizes": resize_library(), "rounds": a.rounds,
                   "host_ms": round(med["host"], 3), "device_from_host_ms": round(med["device_from_host"], 3),
                   "device_resident_ms": round(med["device_resident"], 3),
                   "host_ms_min_max": [round(min(ms["host"]), 3), round(max(ms["host"]), 3)],
                   "device_from_host_ms_min_max": [round(min(ms["device_from_host"]), 3), round(max(ms["device_from_host"]), 3)],
                   "host_over_device_from_host": round(med["host"] / med["device_from_host"], 2),
                   "host_over_device_resident": round(med["host"] / med["device_resident"], 2),
                   "faces": faces, "candidates_per_frame_max": int(counts.max()), "crops": n_crops,
                   "stages_ms": {k: round(statistics.median(v), 3) for k, v in st.items()}}
            lines.append(res)
            print(json.dumps(res), flush=True)
        lm.face_detector = None
        det.release()
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"what": "tools/face_pipeline_bench.py " + " ".join(sys.argv[1:]) + " on one MI355X, profiler off",
                       "source_hash": build.source_hash(), "lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
