"""Frames to landmarks on one MI355X: the host path (LandmarkDetector.detect_landmarks with an S3FDDetector, every resize and
crop on the CPU) against the device path (detect_landmarks_device) from host frames and from frames already resident, in one
process, alternating, with per-stage times of the device path.

    python tools/face_pipeline_bench.py [--batches 1,8,16] [--precisions fp32,bf16] [--nms host,device] [--rounds 7] [--warmup 2]
                                        [--json FILE]

Frames: the recipe's 270 x 480 detector frames (recipe.make_s3fd_inputs) tiled 4 x 4 pixel-wise to 1080 x 1920, so the detector
at the reference's scale 0.25 sees recipe frames; weights are the recipes' (synthetic), so the number of "faces" per frame is
whatever those weights give -- it is printed, and PFLD's share of the time scales with it.  --max-faces keeps only the first
N boxes of a frame in BOTH paths (a wrapper around the detector), 0 keeps all.

--nms host | device | host,device says where detect_device runs S3FD's two NMS passes (S3FDDetector(nms=...)): it changes the
device legs and the candidates_nms stage, not the host path.  With both, every round runs the legs and the stages of one and
then of the other, alternating, in this one process, and there is one line for each.

One JSON line per (precision, batch, nms): medians over --rounds of host_ms, device_from_host_ms, device_resident_ms (with the
lowest and highest round of each), which library did the host path's resizes (cv2 or Pillow: different arithmetic from the
device path's, so the landmarks are compared only as a count), and the stages of the device path, each timed on its own
between synchronisations: upload, downscale, s3fd, candidates_nms (S3FDDetector.detections_from_dense: compaction, then download
and host NMS, or the NMS kernel and the download of the faces), crops, pfld, finalize (with its download).  Stage times carry a
synchronisation each and do not add up to the end-to-end figure exactly.

Behind them one line per batch for the NMS operator alone on 1024 candidate rows per frame (the crowded case of
tests/nms_cases.py, a seed per frame): face_ops.s3fd_nms with the download of status and faces, against numpy
(facedet.detect_output + detect_faces_rows) on the same rows.
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
    t["candidates_nms"], found = timed(lambda: det.detections_from_dense(dense, dev.shape[2], dev.shape[1]))
    counts = (dense[:, :, 0] > facedet.CONF_THRESH).sum(dim=1).cpu().numpy()
    boxes = [[tuple(float(v) for v in box) for box in bs] for bs, _ in found]
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


def nms_operator(batch, rounds, warmup, width=1920, height=1080, conf_th=0.1):
    """face_ops.s3fd_nms + the download of status and faces against numpy on the same 1024 rows per frame -> one result line"""
    import numpy as np
    import torch
    from calipsync_amd import face_ops, facedet
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nms_cases
    rows = np.stack([nms_cases.candidate_rows(1024, 300, seed=i) for i in range(batch)])
    rows_dev = torch.from_numpy(rows).cuda()
    counts_dev = torch.full((batch,), 1024, dtype=torch.int32, device="cuda")
    status = torch.empty((batch,), dtype=torch.int32, device="cuda")
    faces = torch.empty((batch, face_ops.NMS_TOP_K, 5), dtype=torch.float64, device="cuda")

    def device():
        face_ops.s3fd_nms(counts_dev, rows_dev, width, height, conf_th, status=status, faces=faces)
        st = status.cpu().numpy()
        return st, faces[:, :max(1, int(st.max()))].cpu().numpy()

    def kernel():
        face_ops.s3fd_nms(counts_dev, rows_dev, width, height, conf_th, status=status, faces=faces)

    def numpy_():
        return [facedet.detect_faces_rows(facedet.detect_output(r[None])[0], width, height, conf_th) for r in rows]

    ms = {"device": [], "kernel": [], "numpy": []}
    for r in range(warmup + rounds):
        for k, fn in (("numpy", numpy_), ("device", device), ("kernel", kernel)):
            t, out = timed(fn)
            if r >= warmup:
                ms[k].append(t)
            if k == "numpy":
                want = out
            elif k == "device":
                same = all(len(w) == s and np.array_equal(w, f[:s]) for w, s, f in zip(want, out[0], out[1]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"operator": "s3fd_nms", "rows_per_frame": 1024, "batch": batch, "frame": [height, width], "rounds": rounds,
            "faces_per_frame": [int(len(w)) for w in want], "equal_to_numpy": bool(same),
            "kernel_and_download_ms": round(med["device"], 4), "kernel_ms": round(med["kernel"], 4), "numpy_ms": round(med["numpy"], 4),
            "kernel_and_download_ms_min_max": [round(min(ms["device"]), 4), round(max(ms["device"]), 4)],
            "numpy_ms_min_max": [round(min(ms["numpy"]), 4), round(max(ms["numpy"]), 4)],
            "numpy_over_device": round(med["numpy"] / med["device"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,16")
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-faces", type=int, default=0)
    ap.add_argument("--nms", default="host,device", help="host, device, or host,device: both, alternating within every round")
    ap.add_argument("--json")
    a = ap.parse_args()
    import numpy as np
    import torch
    from calipsync_amd import build, facedet, landmarks, recipe
    places = a.nms.split(",")
    if not places or any(p not in facedet.NMS_PLACES for p in places):
        raise SystemExit(f"face_pipeline_bench: --nms {a.nms!r}, expected host, device or host,device")
    if not torch.cuda.is_available():
        raise SystemExit("face_pipeline_bench: no GPU; nothing is measured on a CPU")
    lm = landmarks.LandmarkDetector(state_dict=recipe.make_pfld_state_dict(), mean_face=np.full(220, 0.5, np.float32))
    sd = recipe.make_s3fd_state_dict()
    lines = []
    for precision in a.precisions.split(","):
        det = facedet.S3FDDetector(state_dict=sd, precision=precision, nms=places[0])
        lm.face_detector = FirstFaces(det, a.max_faces)
        for b in [int(v) for v in a.batches.split(",")]:
            small = recipe.make_s3fd_inputs(min(b, 4), 270, 480)
            small = np.concatenate([small] * ((b + len(small) - 1) // len(small)))[:b]
            frames = list(np.repeat(np.repeat(small, 4, 1), 4, 2))
            resident = torch.from_numpy(np.stack(frames)).cuda()
            runs = {"host": lambda: lm.detect_landmarks(frames), "device_from_host": lambda: lm.detect_landmarks_device(frames),
                    "device_resident": lambda: lm.detect_landmarks_device(resident)}
            ms = {p: {k: [] for k in runs} for p in places}
            st = {p: {} for p in places}
            faces = {p: {} for p in places}
            for r in range(a.warmup + a.rounds):
                for p in places:                             # alternating: a drift of the box hits every leg of both alike
                    det.nms = p
                    for k, fn in runs.items():
                        if k == "host" and p != places[0]:   # the host path has no NMS switch: once per round
                            continue
                        t, out = timed(fn)
                        faces[p][k] = sum(len(f) for f in out if f is not None)
                        if r >= a.warmup:
                            ms[p][k].append(t)
                    ts, counts, n_crops = stages(lm, det, frames)
                    if r >= a.warmup:
                        for k, v in ts.items():
                            st[p].setdefault(k, []).append(v)
            for p in places:
                ms[p]["host"], faces[p]["host"] = ms[places[0]]["host"], faces[places[0]]["host"]
                med = {k: statistics.median(v) for k, v in ms[p].items()}
                res = {"precision": precision, "batch": b, "nms": p, "frame": [1080, 1920], "host_resizes": resize_library(), "rounds": a.rounds,
                       "host_ms": round(med["host"], 3), "device_from_host_ms": round(med["device_from_host"], 3),
                       "device_resident_ms": round(med["device_resident"], 3),
                       "host_ms_min_max": [round(min(ms[p]["host"]), 3), round(max(ms[p]["host"]), 3)],
                       "device_from_host_ms_min_max": [round(min(ms[p]["device_from_host"]), 3), round(max(ms[p]["device_from_host"]), 3)],
                       "device_resident_ms_min_max": [round(min(ms[p]["device_resident"]), 3), round(max(ms[p]["device_resident"]), 3)],
                       "host_over_device_from_host": round(med["host"] / med["device_from_host"], 2),
                       "host_over_device_resident": round(med["host"] / med["device_resident"], 2),
                       "faces": faces[p], "candidates_per_frame_max": int(counts.max()), "crops": n_crops,
                       "stages_ms": {k: round(statistics.median(v), 3) for k, v in st[p].items()},
                       "candidates_nms_ms_min_max": [round(min(st[p]["candidates_nms"]), 3), round(max(st[p]["candidates_nms"]), 3)]}
                lines.append(res)
                print(json.dumps(res), flush=True)
        lm.face_detector = None
        det.release()
    if "device" in places:
        for b in [int(v) for v in a.batches.split(",")]:
            res = nms_operator(b, a.rounds, a.warmup)
            lines.append(res)
            print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"what": "tools/face_pipeline_bench.py " + " ".join(sys.argv[1:]) + " on one MI355X, profiler off",
                       "source_hash": build.source_hash(), "lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
