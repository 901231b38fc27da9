"""Generate the error bar of the bf16 S3FD precision by running the REFERENCE itself (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_s3fd_bf16_bar.py      # -> s3fd_bf16_bar.npz

The bar is ``S3FDNet`` under ``torch.autocast("cpu", dtype=torch.bfloat16)`` against its own float64 run on the recipe weights.
The reference is reached exactly as ``make_s3fd_golden.py`` reaches it (that script is imported for its stand-in modules, its
hooks and its helpers).  Only data is written; nothing under ``tests/`` imports this script.

Case 1, the two frames of ``s3fd_b2.npz``: per stage ``[max, mean]`` of |autocast - float64| at that fixture's sample
positions, the same over the whole ``loc``, conf logits, face-logit difference ``conf[..., 1] - conf[..., 0]``, score and box,
and ``c1.fp32_vs_fixture`` = max |float32 run here - stored value|, which ties this file to that fixture.

Case 2, two decision-stable frames: the first two seeds s = 1, 2, ... of ``recipe.make_s3fd_inputs(1, 77, 93, seed=s)`` on
which the float32 reference meets the conditions asserted in ``conditions()``:
  1. every prior's face-logit difference is farther from logit(0.05), logit(0.1) and logit(0.8) than 1.5 x autocast's max
     face-logit-difference error on that frame;
  2. among the priors scoring above 0.03 no IoU is within 4 x autocast's largest change of those IoUs of 0.3 or 0.1;
  3. at least 2 faces at 0.1 and 1 at 0.8, and the reference under autocast returns the same priors in the same order as
     float32 at both thresholds.
A fourth condition was asked for: no x, y, w or h of a box ``S3FDFaceDetector.detect`` keeps (LandmarkDetector truncates
them to cut its crop) within autocast's largest displacement of a kept box of an integer.  It is evaluated and recorded
(``c2.crop_margin.<i>`` against ``c2.displacement.<i>``) but cannot be required: a value is at most 0.5 from an integer, a
frame keeps two or three boxes (8 to 12 truncated values) and autocast displaces them by 0.12 to 0.6 pixel.  Of the seeds
1 .. 3290, 33 meet conditions 1-3 and none the fourth; the largest crop margin of any candidate is 0.22 pixel.  So integer
crops are not decided by any margin on such frames, under autocast or any other bf16 rounding.
Recorded per frame: the seed and the frame, the dense ``det`` in float64 and float32, the float32 ``Detect`` output, the faces
``detect_faces(scales=[1])`` returns at 0.1 and 0.8 with their priors, the boxes ``detect`` returns, the margins, autocast's
error figures as in case 1 and its displacement in pixels.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_s3fd_golden as G                                   # noqa: E402  (stand-ins, hooks, helpers; reaches the reference)
from calipsync_amd import facedet, recipe                     # noqa: E402

H, W, P = G.H, G.W, 596
THRESHOLDS = (0.05, 0.1, 0.8)
MAX_SEED = 400


def stat(a, b) -> np.ndarray:
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return np.array([d.max(), d.mean()])


def npf(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().numpy() if t.dtype == torch.bfloat16 else t.detach().numpy()


def dlogit(conf) -> np.ndarray:
    conf = np.asarray(conf, dtype=np.float64)
    return conf[..., 1] - conf[..., 0]


def logit(p: float) -> float:
    return float(np.log(p / (1.0 - p)))


def figures(tac, t64, prefix: str, store: dict) -> None:
    """autocast's [max, mean] error against float64: the nine stages at the sample positions, the rest over everything"""
    for n in facedet.STAGES[:9]:
        a, b = npf(tac[n]).reshape(-1), npf(t64[n]).reshape(-1)
        idx = G.sample_indices(a.size)
        store[f"{prefix}.{n}"] = stat(a[idx], b[idx])
    store[f"{prefix}.loc"] = stat(npf(tac["loc"]), npf(t64["loc"]))
    store[f"{prefix}.conf"] = stat(npf(tac["conf"]), npf(t64["conf"]))
    store[f"{prefix}.dlogit"] = stat(dlogit(npf(tac["conf"])), dlogit(npf(t64["conf"])))
    store[f"{prefix}.score"] = stat(npf(tac["det"])[..., 0], npf(t64["det"])[..., 0])
    store[f"{prefix}.box"] = stat(npf(tac["det"])[..., 1:], npf(t64["det"])[..., 1:])


def autocast_run(net, x):
    with torch.autocast("cpu", dtype=torch.bfloat16):
        return G.run(net, x)


def to_x(u8: np.ndarray) -> torch.Tensor:
    return torch.from_numpy((u8.astype(np.float32) - facedet.IMG_MEAN).transpose(0, 3, 1, 2).copy())


def conditions(m: dict) -> list:
    """the names of the conditions a candidate's measurements miss ([] = a stable frame)"""
    bad = []
    if not m["margin_logit"] > 1.5 * m["dlogit_err"]:
        bad.append("logit")
    if not m["margin_iou"] > 4.0 * m["iou_change"]:
        bad.append("iou")
    if not (m["n01"] >= 2 and m["n08"] >= 1 and m["same_priors"]):
        bad.append("faces")
    return bad


def crop_condition(m: dict) -> bool:
    """the fourth condition (recorded only: see the module docstring)"""
    return m["crop_margin"] > m["displacement"]


def main() -> None:
    torch.manual_seed(0)
    torch.set_num_threads(8)
    sd = {k: torch.from_numpy(v.copy()) for k, v in recipe.make_s3fd_state_dict().items()}
    net = G.S3FDNet("cpu").eval()
    net.load_state_dict(sd, strict=True)
    net64 = G.S3FDNet("cpu").double().eval()
    net64.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    s3fd = G.S3FD.__new__(G.S3FD)
    s3fd.device, s3fd.net = "cpu", net
    store: dict = {}

    # ---- case 1 ----------------------------------------------------------------------------------------------------------
    fx = np.load(os.path.join(HERE, "s3fd_b2.npz"))
    x = to_x(recipe.make_s3fd_inputs(G.BATCH, H, W))
    _, t32 = G.run(net, x)
    _, t64 = G.run(net64, x.double())
    _, tac = autocast_run(net, x)
    tie = 0.0
    for n in facedet.STAGES[:9]:
        flat = npf(t32[n]).reshape(-1).astype(np.float64)
        tie = max(tie, float(np.abs(flat[G.sample_indices(flat.size)] - fx[f"{n}.samples"]).max()))
    for n in ("loc", "conf", "det"):
        tie = max(tie, float(np.abs(npf(t32[n]).astype(np.float64) - fx[f"{n}64"]).max()))
    store["c1.fp32_vs_fixture"] = np.array(tie)
    figures(tac, t64, "c1", store)
    for k in sorted(store):
        print(k, store[k])
    assert tie <= max(float(fx[f"ref_err.{n}"]) for n in facedet.STAGES[:9] + ("loc", "conf", "det")), tie

    # ---- case 2: the search ----------------------------------------------------------------------------------------------
    found = []
    for seed in range(1, MAX_SEED + 1):
        u8 = recipe.make_s3fd_inputs(1, H, W, seed=seed)
        x = to_x(u8)
        y32, t32 = G.run(net, x)
        d32 = npf(t32["det"])[0]
        dl32 = dlogit(npf(t32["conf"])[0])
        m = {"margin_logit": min(float(np.abs(dl32 - logit(th)).min()) for th in THRESHOLDS)}
        rows01 = facedet.detect_faces_rows(facedet.detect_output(d32[None])[0], W, H, 0.1)     # (a cheap look before the slow runs:
        # autocast's face-logit error is above 0.1 on every frame seen, so a margin below 0.15 cannot pass)
        if m["margin_logit"] < 0.15 or len(rows01) < 2:
            continue
        _, t64 = G.run(net64, x.double())
        yac, tac = autocast_run(net, x)
        d64, dac = npf(t64["det"])[0], npf(tac["det"])[0]
        m["dlogit_err"] = float(np.abs(dlogit(npf(tac["conf"])[0]) - dlogit(npf(t64["conf"])[0])).max())
        sel = np.nonzero(d32[:, 0] > 0.03)[0]
        tri = np.triu_indices(sel.size, 1)
        iou32, iou64, iouac = (G.iou_matrix(d[sel, 1:].astype(np.float64))[tri] for d in (d32, d64, dac))
        m["iou_change"] = float(np.abs(iouac - iou64).max()) if iou32.size else 0.0
        m["margin_iou"] = min(float(np.abs(iou32 - th).min()) for th in (0.3, 0.1)) if iou32.size else 1.0
        faces, faces_ac, same = {}, {}, True
        for th, tag in ((0.1, "01"), (0.8, "08")):
            faces[tag] = s3fd.detect_faces(u8[0], conf_th=th, scales=[1])
            with torch.autocast("cpu", dtype=torch.bfloat16):
                faces_ac[tag] = s3fd.detect_faces(u8[0], conf_th=th, scales=[1])
            p32 = G.prior_of(faces[tag][:, 4], d32[:, 0]) if len(faces[tag]) else []
            pac = G.prior_of(faces_ac[tag][:, 4], dac[:, 0]) if len(faces_ac[tag]) else []
            same = same and p32 == pac
            m[f"priors{tag}"] = p32
        m["n01"], m["n08"], m["same_priors"] = len(faces["01"]), len(faces["08"]), same
        if not same or m["n01"] < 2 or m["n08"] < 1:
            continue
        m["displacement"] = max(float(np.abs(faces_ac[t][:, :4] - faces[t][:, :4]).max()) for t in ("01", "08"))
        det = G.S3FDFaceDetector.__new__(G.S3FDFaceDetector)
        det.conf_threshold, det.nms_threshold, det.last_detection = 0.1, 0.5, None

        class Scale1:
            def detect_faces(self, image, conf_th=0.8, scales=None):
                return s3fd.detect_faces(image, conf_th=conf_th, scales=[1])

        det.det_net = Scale1()
        xywh = np.asarray(det.detect([u8[0]])[0][0])
        m["crop_margin"] = float(np.abs(xywh - np.round(xywh)).min())
        bad = conditions(m)
        print(f"seed {seed}: logit margin {m['margin_logit']:.3f} vs 1.5 x {m['dlogit_err']:.3f}, IoU margin {m['margin_iou']:.4f} vs 4 x "
              f"{m['iou_change']:.4f}, faces {m['n01']}/{m['n08']}, displacement {m['displacement']:.3f} px, crop margin "
              f"{m['crop_margin']:.3f}: {'ok' if not bad else 'misses ' + ' '.join(bad)}{'' if crop_condition(m) else ' (crop condition not met)'}", flush=True)
        if bad:
            continue
        i = len(found)
        found.append(seed)
        store[f"c2.frame.{i}"] = u8[0]
        store[f"c2.det64.{i}"], store[f"c2.det32.{i}"], store[f"c2.detect32.{i}"] = d64, d32, y32.numpy()[0]
        for tag in ("01", "08"):
            store[f"c2.faces{tag}.{i}"] = faces[tag]
            store[f"c2.priors{tag}.{i}"] = np.asarray(m[f"priors{tag}"], dtype=np.int64)
        store[f"c2.boxes.{i}"] = xywh
        store[f"c2.crop_condition.{i}"] = np.array(int(crop_condition(m)))
        for k in ("margin_logit", "dlogit_err", "margin_iou", "iou_change", "displacement", "crop_margin"):
            store[f"c2.{k}.{i}"] = np.array(m[k])
        figures(tac, t64, f"c2.{i}", store)
        assert conditions(m) == []
        if len(found) == 2:
            break
    assert len(found) == 2, f"{len(found)} stable frames among the seeds 1..{MAX_SEED}"
    store["c2.seeds"] = np.asarray(found, dtype=np.int64)
    path = os.path.join(HERE, "s3fd_bf16_bar.npz")
    np.savez_compressed(path, **store)
    print("seeds", found, "wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
