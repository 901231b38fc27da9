"""A functional restatement of the reference's S3FD detector in torch, for shapes the fixture does not cover: the network
(tools/s3fd/nets.py:109-171) from a state dict in any dtype, its priors and decode (box_utils.py:41-59,195-217), and the
post-processing behind it (box_utils.py:62-173, main.py:45-58, detect_face.py:41-75) written with the tensor operations the
reference uses.  tests/golden/s3fd_b2.npz pins it to the reference itself (tests/test_facedet.py)."""
from __future__ import annotations

import itertools

import numpy as np
import torch
import torch.nn.functional as F

from calipsync_amd import facedet

STAGE_AFTER = {2: "conv1_2", 7: "conv2_2", 14: "conv3_3", 21: "conv4_3", 28: "conv5_3", 31: "fc6", 33: "fc7"}
POOLS = {2: False, 7: False, 14: True, 21: False, 28: False}       # vgg index of the conv in front of a pool -> ceil_mode
SOURCES = ("conv3_3", "conv4_3", "conv5_3", "fc7", "conv6_2", "conv7_2")   # the taps the heads read, in prior order
# every conv of the trunk in forward order: (state-dict prefix, engine name, conv2d arguments, ceil_mode of the pool behind it
# or None, the tap it ends or None)
_CONVS = tuple((f"vgg.{idx}", name, dict(padding=6, dilation=6) if name == "fc6" else dict(padding=k // 2), POOLS.get(idx),
                STAGE_AFTER.get(idx)) for idx, name, _cin, _cout, k in facedet.VGG) + \
    tuple((f"extras.{idx}", name, dict(stride=2 if k == 3 else 1, padding=k // 2), None, name if k == 3 else None)
          for idx, name, _cin, _cout, k in facedet.EXTRAS)
_TAPS = tuple(c[4] for c in _CONVS if c[4])
assert _TAPS == facedet.STAGES[:9]


def _param(sd, key, dtype):
    v = sd[key]
    return (v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))).to(dtype)   # (tensors: any device)


def segment(sd, x, start, dtype=torch.float64, post=None):
    """One stretch of the trunk: from the tensor at tap `start` (a name or an index of facedet.STAGES[:9]; None = the
    mean-subtracted input [B,3,H,W]) to the next tap -> (name, NCHW tensor).  A tap is taken after its ReLU and before its pool,
    so the pool behind tap `start` opens this segment.  post, where given, is applied to the output of every conv (after the
    ReLU): a model of an engine that rounds there."""
    start = _TAPS[start] if isinstance(start, int) else start
    first = 0 if start is None else 1 + [c[4] for c in _CONVS].index(start)
    if first >= len(_CONVS):
        raise ValueError(f"s3fd_ref.segment: no tap behind {start}")
    x = torch.as_tensor(x).to(dtype)
    if first and _CONVS[first - 1][3] is not None:
        x = F.max_pool2d(x, 2, 2, ceil_mode=_CONVS[first - 1][3])
    for prefix, _name, kw, _pool, tap in _CONVS[first:]:
        x = F.relu(F.conv2d(x, _param(sd, f"{prefix}.weight", dtype).to(x.device), _param(sd, f"{prefix}.bias", dtype).to(x.device), **kw))
        if post is not None:
            x = post(x)
        if tap:
            return tap, x
        if _pool is not None:
            x = F.max_pool2d(x, 2, 2, ceil_mode=_pool)
    raise AssertionError("unreachable: the last conv ends a tap")


def heads(sd, taps, dtype=torch.float64, post=None):
    """the six source taps (SOURCES order; a list, or a dict that holds them) -> (loc [B,P,4], conf [B,P,2] logits after conf[0]'s
    max-out, maps): L2Norm on the first three, then loc[k] / conf[k].  post, where given, is applied to x / norm."""
    if isinstance(taps, dict):
        taps = [taps[n] for n in SOURCES]
    loc, conf, maps = [], [], []
    for k, s in enumerate(taps):
        s = torch.as_tensor(s).to(dtype)
        if k < 3:
            norm = s.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10
            s = torch.div(s, norm)
            s = _param(sd, f"{facedet.L2NORMS[k][0]}.weight", dtype).to(s.device).view(1, -1, 1, 1) * (s if post is None else post(s))
        lo = F.conv2d(s, _param(sd, f"loc.{k}.weight", dtype).to(s.device), _param(sd, f"loc.{k}.bias", dtype).to(s.device), padding=1)
        co = F.conv2d(s, _param(sd, f"conf.{k}.weight", dtype).to(s.device), _param(sd, f"conf.{k}.bias", dtype).to(s.device), padding=1)
        if k == 0:
            co = torch.cat((co[:, 0:3].max(dim=1, keepdim=True)[0], co[:, 3:]), dim=1)
        loc.append(lo.permute(0, 2, 3, 1).reshape(lo.shape[0], -1))
        conf.append(co.permute(0, 2, 3, 1).reshape(co.shape[0], -1))
        maps.append(tuple(s.shape[2:]))
    b = loc[0].shape[0]
    return torch.cat(loc, 1).view(b, -1, 4), torch.cat(conf, 1).view(b, -1, 2), maps


def network(sd, x, dtype=torch.float64):
    """x [B,3,H,W] (mean subtracted) -> {stage: NCHW tensor, "loc": [B,P,4], "conf": [B,P,2] logits after the max-out}: the nine
    segments in a row, then the heads"""
    taps, start = {}, None
    for _ in _TAPS:
        start, x = segment(sd, x, start, dtype)
        taps[start] = x
    taps["loc"], taps["conf"], taps["maps"] = heads(sd, taps, dtype)
    return taps


def priors(h, w, maps):
    """PriorBox.forward: Python floats, rounded once by torch.FloatTensor"""
    mean = []
    for k, (fh, fw) in enumerate(maps):
        step, size = 4 << k, 16 << k
        for i, j in itertools.product(range(fh), range(fw)):
            mean += [(j + 0.5) / (w / step), (i + 0.5) / (h / step), size / w, size / h]
    return torch.FloatTensor(mean).view(-1, 4)


def dense(taps, h, w, dtype=torch.float64, pr=None):
    """-> det [B,P,5] = (softmax(conf)[..., 1], decode(loc, priors, [0.1, 0.2])); pr: the priors, where the caller keeps them"""
    pr = (priors(h, w, taps["maps"]) if pr is None else pr).to(taps["loc"].device, dtype)
    loc, conf = taps["loc"].to(dtype), taps["conf"].to(dtype)
    b = loc.shape[0]
    l, q = loc.reshape(-1, 4), pr.repeat(b, 1)
    boxes = torch.cat((q[:, :2] + l[:, :2] * 0.1 * q[:, 2:], q[:, 2:] * torch.exp(l[:, 2:] * 0.2)), 1)
    boxes[:, :2] -= boxes[:, 2:] / 2
    boxes[:, 2:] += boxes[:, :2]
    score = torch.softmax(conf, dim=-1)[..., 1:]
    return torch.cat((score, boxes.view(b, -1, 4)), 2)


# ---- post-processing, with torch's own float32 operations -----------------------------------------------------------------
def detect_torch(det):
    """Detect.forward on the dense det [B,P,5] (float32 tensor) -> [B,2,750,5]"""
    det = torch.as_tensor(det, dtype=torch.float32)
    out = torch.zeros(det.shape[0], 2, facedet.TOP_K, 5)
    for i in range(det.shape[0]):
        scores_all, boxes_all = det[i, :, 0].clone(), det[i, :, 1:].clone()
        mask = scores_all.gt(facedet.CONF_THRESH)
        scores, boxes = scores_all[mask], boxes_all[mask.unsqueeze(1).expand_as(boxes_all)].view(-1, 4)
        if boxes.numel() == 0:
            continue
        area = torch.mul(boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1])
        _, idx = scores.sort(dim=0, stable=True)
        idx = idx[-facedet.NMS_TOP_K:]
        keep = []
        while idx.numel() > 0:
            top = idx[-1]
            keep.append(int(top))
            if idx.size(0) == 1:
                break
            idx = idx[:-1]
            xx1 = torch.clamp(boxes[:, 0].index_select(0, idx), min=boxes[top, 0])
            yy1 = torch.clamp(boxes[:, 1].index_select(0, idx), min=boxes[top, 1])
            xx2 = torch.clamp(boxes[:, 2].index_select(0, idx), max=boxes[top, 2])
            yy2 = torch.clamp(boxes[:, 3].index_select(0, idx), max=boxes[top, 3])
            inter = torch.clamp(xx2 - xx1, min=0.0) * torch.clamp(yy2 - yy1, min=0.0)
            union = (area.index_select(0, idx) - inter) + area[top]
            idx = idx[(inter / union).le(facedet.NMS_THRESH)]
        keep = torch.tensor(keep[:facedet.TOP_K], dtype=torch.long)
        out[i, 1, :keep.numel()] = torch.cat((scores[keep].unsqueeze(1), boxes[keep]), 1)
    return out


def detect_faces_torch(detections, width, height, conf_th):
    """S3FD.detect_faces behind the network for one image: detections [2,750,5] tensor -> float64 rows"""
    bboxes = np.empty(shape=(0, 5))
    scale = torch.Tensor([width, height, width, height])
    for i in range(detections.size(0)):
        j = 0
        while detections[i, j, 0] > conf_th:
            pt = (detections[i, j, 1:] * scale).numpy()
            bboxes = np.vstack((bboxes, (pt[0], pt[1], pt[2], pt[3], detections[i, j, 0])))
            j += 1
    return bboxes[facedet.nms_(bboxes, facedet.FINAL_NMS)] if len(bboxes) else bboxes
