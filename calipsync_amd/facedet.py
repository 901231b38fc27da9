"""Face boxes on the HIP engine: the drop-in for the reference's ``S3FDFaceDetector``
(utils/lip_detector/tools/detect_face.py:5-81; tools/s3fd/nets.py, box_utils.py, main.py) without the reference tree.

* ``manifest()`` / ``check_state_dict(sd)`` cover the 65 keys of ``S3FDNet`` (22,459,110 parameters).
* ``pack`` / ``unpack`` write the convs into the engine's packed buffer (``casync_s3fd_packed_*``): dense 3x3 as
  [cout][(ky,kx,cin)], 1x1 as [N][K], ``loc[k]`` over ``conf[k]`` per source with the L2Norm weight folded in (float64, one
  rounding).
* ``S3FDEngine`` runs the network on float NCHW frames (mean subtracted) or on the uint8 frames themselves and returns the
  dense ``det`` [B,P,5] = (face probability, x1, y1, x2, y2) of every prior.
* ``detect_output`` / ``detect_faces_rows`` / ``nms_`` restate, in numpy and in the reference's own dtypes,
  ``Detect.forward`` + ``nms`` (box_utils.py:62-173; float32), ``S3FD.detect_faces`` (main.py:45-58; float32 scaling, float64
  rows) and Girshick's ``nms_`` (box_utils.py:7-38).
* ``S3FDDetector`` keeps ``S3FDFaceDetector.detect`` (detect_face.py:27-75) and is callable as the ``face_detector`` of
  ``calipsync_amd.landmarks.LandmarkDetector``.  The ``cv2.resize(fx=s, fy=s, INTER_LINEAR)`` in front of the network
  (main.py:34) uses cv2 where it imports, else Pillow's bilinear filter; cv2 is not in the build image, so that step is NOT
  pinned against the reference, like ``landmarks.resize192``.  ``scale=1`` bypasses it entirely.
* ``S3FDDetector.detect_device`` / ``dense_device`` are the same detector on frames resident on the device (DESIGN section
  8e): the downscale is a kernel with OpenCV's arithmetic on every box (``calipsync_amd.face_ops``), and only the rows above
  ``CONF_THRESH`` come back to the host (``nms="host"``) or, with both NMS passes on the device too (``nms="device"``,
  ``face_ops.s3fd_nms``), only the faces.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .engine_base import _PackedEngine

# nn.Conv2d(cin, cout, k) of S3FDNet.vgg by ModuleList index (nets.py:34-75), with the engine's name
VGG = ((0, "conv1_1", 3, 64, 3), (2, "conv1_2", 64, 64, 3), (5, "conv2_1", 64, 128, 3), (7, "conv2_2", 128, 128, 3),
       (10, "conv3_1", 128, 256, 3), (12, "conv3_2", 256, 256, 3), (14, "conv3_3", 256, 256, 3),
       (17, "conv4_1", 256, 512, 3), (19, "conv4_2", 512, 512, 3), (21, "conv4_3", 512, 512, 3),
       (24, "conv5_1", 512, 512, 3), (26, "conv5_2", 512, 512, 3), (28, "conv5_3", 512, 512, 3),
       (31, "fc6", 512, 1024, 3), (33, "fc7", 1024, 1024, 1))
L2NORMS = (("L2Norm3_3", 256), ("L2Norm4_3", 512), ("L2Norm5_3", 512))                      # nets.py:77-79
EXTRAS = ((0, "conv6_1", 1024, 256, 1), (1, "conv6_2", 256, 512, 3), (2, "conv7_1", 512, 128, 1), (3, "conv7_2", 128, 256, 3))
SOURCE_CHANNELS = (256, 512, 512, 1024, 512, 256)                                           # nets.py:88-104
CONF_OUT = (4, 2, 2, 2, 2, 2)
N_PARAMETERS = 22459110
STAGES = ("conv1_2", "conv2_2", "conv3_3", "conv4_3", "conv5_3", "fc6", "fc7", "conv6_2", "conv7_2", "loc", "conf", "det")
_STAGE_C = (64, 128, 256, 512, 512, 1024, 1024, 512, 256)
IMG_MEAN = np.array([123.0, 117.0, 104.0], dtype=np.float32)   # per channel of the image as given (main.py:38-41: the swaps cancel)
# Detect() and the callers' constants (box_utils.py:131-133, main.py:57)
CONF_THRESH, NMS_THRESH, NMS_TOP_K, TOP_K, FINAL_NMS = 0.05, 0.3, 5000, 750, 0.1
PRECISIONS = {"fp32": 0, "bf16": 1}     # casync_s3fd_create_ex
NMS_PLACES = ("device", "host")         # S3FDDetector(nms=...): where detect_device runs the two NMS passes
NMS_HEAD = 32                           # detect_device, nms="device": face rows per frame that come back with the status in one copy


def manifest() -> List[Tuple[str, Tuple[int, ...]]]:
    """[(key, shape)] of S3FDNet().state_dict() in its own order (65 keys)."""
    keys: List[Tuple[str, Tuple[int, ...]]] = []
    for idx, _n, cin, cout, k in VGG:
        keys += [(f"vgg.{idx}.weight", (cout, cin, k, k)), (f"vgg.{idx}.bias", (cout,))]
    keys += [(f"{n}.weight", (c,)) for n, c in L2NORMS]
    for idx, _n, cin, cout, k in EXTRAS:
        keys += [(f"extras.{idx}.weight", (cout, cin, k, k)), (f"extras.{idx}.bias", (cout,))]
    for head, outs in (("loc", (4,) * 6), ("conf", CONF_OUT)):
        for k, (c, o) in enumerate(zip(SOURCE_CHANNELS, outs)):
            keys += [(f"{head}.{k}.weight", (o, c, 3, 3)), (f"{head}.{k}.bias", (o,))]
    return keys


def check_state_dict(sd) -> None:
    """ValueError naming the first missing or unexpected key, or wrong shape."""
    want = manifest()
    for key, shape in want:
        if key not in sd:
            raise ValueError(f"S3FD checkpoint lacks {key}")
        if tuple(sd[key].shape) != shape:
            raise ValueError(f"S3FD checkpoint: {key} has shape {tuple(sd[key].shape)}, S3FDNet has {shape}")
    names = {k for k, _ in want}
    for key in sd:
        if key not in names:
            raise ValueError(f"S3FD checkpoint has an unexpected key {key}")


def _f64(v) -> np.ndarray:
    return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float64)


def _rows(w: np.ndarray) -> np.ndarray:
    """[cout, cin, kh, kw] -> [cout][(ky, kx, cin)]"""
    return w.transpose(0, 2, 3, 1).reshape(w.shape[0], -1)


def packed_tensors(sd) -> Dict[str, np.ndarray]:
    """The engine's named tensors (include/casync_hip.h, casync_s3fd_packed_*)."""
    check_state_dict(sd)
    out: Dict[str, np.ndarray] = {}
    for idx, name, _cin, _cout, _k in VGG:
        w = _f64(sd[f"vgg.{idx}.weight"])
        out[f"{name}.w"] = _rows(w).T if name == "conv1_1" else _rows(w)      # conv1_1: [(ky,kx,ci)][64]
        out[f"{name}.b"] = _f64(sd[f"vgg.{idx}.bias"])
    for idx, name, _cin, _cout, _k in EXTRAS:
        out[f"{name}.w"], out[f"{name}.b"] = _rows(_f64(sd[f"extras.{idx}.weight"])), _f64(sd[f"extras.{idx}.bias"])
    for k, c in enumerate(SOURCE_CHANNELS):
        w = np.zeros((8, c, 3, 3))
        b = np.zeros(8)
        w[:4], b[:4] = _f64(sd[f"loc.{k}.weight"]), _f64(sd[f"loc.{k}.bias"])
        w[4:4 + CONF_OUT[k]], b[4:4 + CONF_OUT[k]] = _f64(sd[f"conf.{k}.weight"]), _f64(sd[f"conf.{k}.bias"])
        if k < 3:       # conv(weight * x / norm) = conv'(x / norm) with conv'.w[o, c] = conv.w[o, c] * weight[c]: float64, one rounding
            w = w * _f64(sd[f"{L2NORMS[k][0]}.weight"]).reshape(1, c, 1, 1)
        out[f"head{k}.w"], out[f"head{k}.b"] = _rows(w), b
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def pack(sd) -> np.ndarray:
    """The flat float32 buffer casync_s3fd_load_weights_* takes."""
    from . import _lib
    return _lib.pack_named(packed_tensors(sd), _lib.s3fd_layout())


def unpack(buf: np.ndarray) -> Dict[str, np.ndarray]:
    """Inverse of pack (flat shapes)."""
    from . import _lib
    return _lib.unpack_named(buf, _lib.s3fd_layout())


def map_sizes(h: int, w: int) -> Optional[List[Tuple[int, int]]]:
    """The six source maps of an h x w frame (pools 1, 2, 4, 5 floor, pool 3 ceil, the extras' stride-2 convs); None for a
    size the network cannot run (a pooled dimension of 0)."""
    def half(v):
        return v // 2
    m = [(half(half(h)), half(half(w)))]
    if min(m[0]) < 1:
        return None
    m.append(((m[0][0] + 1) // 2, (m[0][1] + 1) // 2))
    m.append((half(m[1][0]), half(m[1][1])))
    m.append((half(m[2][0]), half(m[2][1])))
    if min(m[3]) < 1:
        return None
    m.append(((m[3][0] - 1) // 2 + 1, (m[3][1] - 1) // 2 + 1))
    m.append(((m[4][0] - 1) // 2 + 1, (m[4][1] - 1) // 2 + 1))
    return m


def n_priors(h: int, w: int) -> int:
    m = map_sizes(h, w)
    return sum(a * b for a, b in m) if m else 0


class S3FDEngine(_PackedEngine):
    """S3FDNet().eval() up to Detect.forward, on the HIP engine: forward(x [B,3,H,W] float, mean subtracted) or
    forward_u8(frames [B,H,W,3] uint8) -> the dense det [B,P,5] on the device.  There is no CPU path.  precision "bf16"
    runs the network on bf16 activations; inputs, outputs and taps stay float32."""

    _destroy = "casync_s3fd_destroy"

    def __init__(self, sd, device: str = "cuda:0", precision: str = "fp32"):
        if precision not in PRECISIONS:
            raise ValueError(f"S3FD engine: precision {precision!r}, expected one of {sorted(PRECISIONS)}")
        self.precision = precision
        buf = pack(sd)                 # (checks the checkpoint before any device call)
        self._open(device, "casync_s3fd_create_ex", (PRECISIONS[precision],), "casync_s3fd_load_weights_host", buf)

    def workspace_bytes(self, batch: int, h: int, w: int) -> int:
        return self._lib.casync_s3fd_workspace_bytes_ex(PRECISIONS[self.precision], batch, h, w)

    def _workspace(self, batch: int, h: int, w: int) -> torch.Tensor:
        need = max(self.workspace_bytes(batch, h, w), 256)     # (0: the forward itself says why it refuses the shape)
        return self._grow_workspace(need)

    def stage_shape(self, stage: int, batch: int, h: int, w: int) -> Tuple[int, ...]:
        m = map_sizes(h, w) or [(0, 0)] * 6
        p = sum(a * b for a, b in m)
        if stage >= 9:
            return (batch, p, (4, 2, 5)[stage - 9])
        hw = [(h, w), (h // 2, w // 2), m[0], m[1], m[2], m[3], m[3], m[4], m[5]][stage]
        return (batch, hw[0], hw[1], _STAGE_C[stage])

    def _run(self, x: torch.Tensor, u8: bool, h: int, w: int, stage, out, ws):
        from . import _lib
        b = x.shape[0]
        ws = self._workspace(b, h, w) if ws is None else ws
        last = len(STAGES) - 1
        stage = last if stage is None else STAGES.index(stage) if isinstance(stage, str) else int(stage)
        if out is None:
            out = torch.empty(self.stage_shape(stage, b, h, w), dtype=torch.float32, device=self.device)
        strm = torch.cuda.current_stream(self.device).cuda_stream
        st = self._lib.casync_s3fd_forward_tap(self._h, x.data_ptr(), int(u8), b, h, w, stage, out.data_ptr(), ws.data_ptr(),
                                               ws.numel() * ws.element_size(), strm)
        _lib.check(st, "casync_s3fd_forward")
        return out

    def forward(self, x: torch.Tensor, stage=None, out=None, workspace=None) -> torch.Tensor:
        """x [B,3,H,W] float as main.py:36-42 hands it over -> det [B,P,5]; stage (name or index of STAGES) = that
        intermediate instead (NHWC)."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"S3FD engine: input {tuple(x.shape)}, expected [B,3,H,W]")
        return self._run(x.to(self.device, torch.float32).contiguous(), False, x.shape[2], x.shape[3], stage, out, workspace)

    def forward_u8(self, frames, stage=None, out=None, workspace=None) -> torch.Tensor:
        """frames [B,H,W,3] uint8 (numpy or tensor) -> det [B,P,5]; the mean is subtracted on the device."""
        frames = torch.as_tensor(frames)
        if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8:
            raise ValueError(f"S3FD engine: frames {tuple(frames.shape)} {frames.dtype}, expected uint8 [B,H,W,3]")
        return self._run(frames.to(self.device).contiguous(), True, frames.shape[1], frames.shape[2], stage, out, workspace)

    def forward_tap(self, x, stage, u8: bool = False) -> torch.Tensor:
        return self.forward_u8(x, stage) if u8 else self.forward(x, stage)

    __call__ = forward


# ---- post-processing on the host: the reference's arithmetic in its own dtypes ------------------------------------------
def nms_f32(boxes: np.ndarray, scores: np.ndarray, overlap: float = NMS_THRESH, top_k: int = NMS_TOP_K):
    """box_utils.py:62-126 (nms) on float32 arrays -> (keep indices, count).  Every operation is the float32 one torch runs:
    area = (x2 - x1) * (y2 - y1), union = (area[idx] - inter) + area[i], IoU <= float32(overlap)."""
    boxes = np.asarray(boxes, dtype=np.float32)
    scores = np.asarray(scores, dtype=np.float32)
    keep = np.zeros(scores.shape[0], dtype=np.int64)
    if boxes.size == 0:
        return keep, 0
    x1, y1, x2, y2 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    area = (x2 - x1) * (y2 - y1)
    idx = np.argsort(scores, kind="stable")[-top_k:]       # ascending; (torch's sort leaves the order of ties open)
    thr = np.float32(overlap)
    count = 0
    while idx.size > 0:
        i = idx[-1]
        keep[count] = i
        count += 1
        if idx.size == 1:
            break
        idx = idx[:-1]
        xx1, yy1 = np.maximum(x1[idx], x1[i]), np.maximum(y1[idx], y1[i])
        xx2, yy2 = np.minimum(x2[idx], x2[i]), np.minimum(y2[idx], y2[i])
        w, h = np.maximum(xx2 - xx1, np.float32(0.0)), np.maximum(yy2 - yy1, np.float32(0.0))
        inter = w * h
        union = (area[idx] - inter) + area[i]
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = inter / union
        idx = idx[iou <= thr]
    return keep, count


def detect_output(det: np.ndarray) -> np.ndarray:
    """Detect.forward (box_utils.py:142-173) from the dense det [B,P,5] (score, box) -> [B,2,750,5] float32."""
    det = np.asarray(det, dtype=np.float32)
    out = np.zeros((det.shape[0], 2, TOP_K, 5), dtype=np.float32)
    for i in range(det.shape[0]):
        mask = det[i, :, 0] > np.float32(CONF_THRESH)
        scores, boxes = det[i, mask, 0], det[i, mask, 1:]
        ids, count = nms_f32(boxes, scores, NMS_THRESH, NMS_TOP_K)
        count = min(count, TOP_K)
        out[i, 1, :count, 0] = scores[ids[:count]]
        out[i, 1, :count, 1:] = boxes[ids[:count]]
    return out


def nms_(dets: np.ndarray, thresh: float) -> np.ndarray:
    """box_utils.py:7-38 on float64 rows (x1, y1, x2, y2, score)."""
    x1, y1, x2, y2, scores = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3], dets[:, 4]
    areas = (x2 - x1) * (y2 - y1)
    order = scores.argsort()[::-1]
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(int(i))
        xx1, yy1 = np.maximum(x1[i], x1[order[1:]]), np.maximum(y1[i], y1[order[1:]])
        xx2, yy2 = np.minimum(x2[i], x2[order[1:]]), np.minimum(y2[i], y2[order[1:]])
        w, h = np.maximum(0.0, xx2 - xx1), np.maximum(0.0, yy2 - yy1)
        inter = w * h
        with np.errstate(divide="ignore", invalid="ignore"):
            ovr = inter / (areas[i] + areas[order[1:]] - inter)
        order = order[np.where(ovr <= thresh)[0] + 1]
    return np.array(keep).astype(int)


def detect_faces_rows(detections: np.ndarray, width: int, height: int, conf_th: float) -> np.ndarray:
    """main.py:45-58 for one image and one scale: detections [2,750,5] (Detect.forward's output for it) -> float64 rows
    (x1, y1, x2, y2, score) in pixels of the width x height image, after nms_(rows, 0.1).  As in the reference, 750 rows
    above conf_th run the walk off the end of the array: IndexError."""
    bboxes = np.empty(shape=(0, 5))
    scale = np.array([width, height, width, height], dtype=np.float32)
    th = np.float32(conf_th)
    for i in range(detections.shape[0]):
        j = 0
        while detections[i, j, 0] > th:          # (IndexError at j == 750, as detections[0, i, j, 0] there)
            pt = detections[i, j, 1:] * scale     # float32
            bboxes = np.vstack((bboxes, (pt[0], pt[1], pt[2], pt[3], detections[i, j, 0])))
            j += 1
    return bboxes[nms_(bboxes, FINAL_NMS)]


def resize_scale(image: np.ndarray, s: float) -> np.ndarray:
    """cv2.resize(image, (0, 0), fx=s, fy=s, INTER_LINEAR) where cv2 imports, else Pillow's bilinear filter at the size cv2
    would choose.  Not pinned against the reference."""
    try:
        import cv2
        return cv2.resize(image, dsize=(0, 0), fx=s, fy=s, interpolation=cv2.INTER_LINEAR)
    except ImportError:
        from PIL import Image
        size = (int(round(image.shape[1] * s)), int(round(image.shape[0] * s)))
        return np.asarray(Image.fromarray(image).resize(size, Image.BILINEAR))


class S3FDDetector:
    """The reference's S3FDFaceDetector(weight_path, conf_threshold) on the HIP engine.  weight_base_dir holds
    ``sfd_face.pth``; or pass state_dict.  detect(images) -> [(bboxes_xywh float64 [n,4], indices)] as detect_face.py:27-75;
    calling the object gives per image the list of (x, y, w, h) boxes LandmarkDetector's face_detector returns.  Images of
    one size run through one batched forward.  nms says where detect_device runs the two NMS passes behind the network:
    "device" (face_ops.s3fd_nms) or "host" (numpy on the downloaded candidate rows); the detections are the same.  The default
    is "host" until tools/face_pipeline_bench.py --nms host,device has been run on an MI355X."""

    def __init__(self, weight_base_dir: Optional[str] = None, *, state_dict=None, conf_threshold: float = 0.1, scale: float = 0.25,
                 device: str = "cuda:0", precision: str = "fp32", nms: str = "host"):
        if precision not in PRECISIONS:
            raise ValueError(f"S3FDDetector: precision {precision!r}, expected one of {sorted(PRECISIONS)}")
        if nms not in NMS_PLACES:
            raise ValueError(f"S3FDDetector: nms {nms!r}, expected one of {list(NMS_PLACES)}")
        if state_dict is None:
            if weight_base_dir is None:
                raise ValueError("S3FDDetector: weight_base_dir or state_dict is needed")
            state_dict = dict(torch.load(os.path.join(weight_base_dir, "sfd_face.pth"), map_location="cpu", weights_only=True))
        self.conf_threshold = conf_threshold
        self.scale = scale
        self.precision = precision
        self.nms = nms
        self.last_detection = None
        self.candidate_cap = 1024       # detect_device: rows per frame brought back compacted; a frame with more falls back to its dense rows
        self.det_net = self._make_engine(state_dict, device, precision)
        self._stager = None

    @staticmethod
    def _make_engine(state_dict, device, precision="fp32"):
        return S3FDEngine(state_dict, device, precision)

    def dense(self, images: Sequence[np.ndarray]) -> List[np.ndarray]:
        """per image the dense det [P,5] (float32, host); equal-sized images share a forward"""
        scaled = [np.ascontiguousarray(img if self.scale == 1 else resize_scale(img, self.scale)) for img in images]
        out: List[Optional[np.ndarray]] = [None] * len(scaled)
        groups: Dict[Tuple[int, ...], List[int]] = {}
        for i, img in enumerate(scaled):
            groups.setdefault(img.shape, []).append(i)
        for idxs in groups.values():
            det = self.det_net.forward_u8(np.stack([scaled[i] for i in idxs]))
            det = det.detach().cpu().numpy() if isinstance(det, torch.Tensor) else np.asarray(det)
            for i, d in zip(idxs, det):
                out[i] = d
        return out

    def detect_faces(self, image: np.ndarray, dense: np.ndarray) -> np.ndarray:
        """S3FD.detect_faces (main.py:26-60) behind the network: the rows of one image"""
        return detect_faces_rows(detect_output(dense[None])[0], image.shape[1], image.shape[0], self.conf_threshold)

    def _detection(self, bboxes: np.ndarray):
        """detect_face.py:49-75 for one image's rows: (bboxes_xywh, indices), or the last detection where there is none"""
        if len(bboxes) == 0:                                       # detect_face.py:49-56
            return (np.array([]), []) if self.last_detection is None else self.last_detection
        bboxes_np = np.array([box[:-1] for box in bboxes])
        converted = np.column_stack((bboxes_np[:, :2], bboxes_np[:, 2:] - bboxes_np[:, :2]))
        current = (converted, list(range(len(bboxes))))
        self.last_detection = current
        return current

    def detect(self, images: Sequence[np.ndarray]):
        return [self._detection(self.detect_faces(img, dense)) for img, dense in zip(images, self.dense(images))]

    # ---- the same detector on frames resident on the device -----------------------------------------------------------
    def frames_to_device(self, frames) -> torch.Tensor:
        """a uint8 [B,H,W,3] device tensor as it is; equal-sized numpy frames through one pinned buffer in one copy"""
        from . import face_ops
        if self._stager is None:
            self._stager = face_ops.FrameStager(self.det_net.device)
        return self._stager.upload(frames, "S3FDDetector.detect_device", "detect / dense")

    def dense_device(self, frames) -> torch.Tensor:
        """frames -> the dense det [B,P,5] ON THE DEVICE: the downscale (cv2.resize(fx=scale, fy=scale) in OpenCV's arithmetic;
        scale == 1 skips it) and forward_u8, nothing downloaded."""
        from . import face_ops
        frames = self.frames_to_device(frames)
        small = frames if self.scale == 1 else face_ops.resize_frames_u8(frames, fx=self.scale)
        return self.det_net.forward_u8(small)

    def detect_device(self, frames):
        """detect() for frames on the device (or equal-sized numpy frames, uploaded once).  nms == "host": only the per-frame
        counts and the rows above CONF_THRESH, compacted in prior order on the device, come back; the NMS and everything behind
        it is the host code of detect() on those rows, which it would have selected from the dense tensor in the same order.
        nms == "device": both NMS passes run on those rows where they are and only each frame's face rows come back
        (_faces_device); _detection, with its last_detection state, is the same host code frame by frame."""
        frames = self.frames_to_device(frames)
        if frames.shape[0] == 0:
            return []
        return self.detections_from_dense(self.dense_device(frames), frames.shape[2], frames.shape[1])

    def detections_from_dense(self, det: torch.Tensor, width: int, height: int):
        """detect_device behind the network: the dense det [B,P,5] on the device, of frames of width x height -> detections"""
        from . import face_ops
        if self.nms not in NMS_PLACES:
            raise ValueError(f"S3FDDetector: nms {self.nms!r}, expected one of {list(NMS_PLACES)}")
        b = det.shape[0]
        cap = max(1, min(int(self.candidate_cap), det.shape[1]))
        counts_dev, rows_dev = face_ops.s3fd_candidates(det, CONF_THRESH, cap)
        if self.nms == "device":
            return self._faces_device(det, counts_dev, rows_dev, width, height)
        counts = counts_dev.cpu().numpy()
        rows = rows_dev[:, :max(1, min(int(counts.max()), cap))].cpu().numpy()
        detections = []
        for i in range(b):
            n = int(counts[i])
            cand = rows[i, :n] if n <= cap else det[i].cpu().numpy()        # more than cap: that frame's dense rows
            detections.append(self._detection(detect_faces_rows(detect_output(cand[None])[0], width, height, self.conf_threshold)))
        return detections

    def _faces_device(self, det: torch.Tensor, counts_dev: torch.Tensor, rows_dev: torch.Tensor, width: int, height: int):
        """detect_device behind the candidate rows with the NMS on the device: ONE download of [B, 1 + NMS_HEAD * 5] float64 =
        each frame's status and its first NMS_HEAD face rows; a frame with more faces costs one more copy, a frame with more
        candidates than the kernel takes (status -1) goes through the host code on its dense rows, as with nms == "host"."""
        from . import face_ops
        b = det.shape[0]
        rows_dev = rows_dev[:, :face_ops.NMS_MAX_CAP]            # (a larger candidate_cap: frames beyond 1024 rows fall back)
        status_dev, faces_dev = face_ops.s3fd_nms(counts_dev, rows_dev, width, height, self.conf_threshold)
        head = torch.empty((b, 1 + NMS_HEAD * 5), dtype=torch.float64, device=det.device)
        head[:, 0].copy_(status_dev)
        head[:, 1:].unflatten(1, (NMS_HEAD, 5)).copy_(faces_dev[:, :NMS_HEAD])
        head = head.cpu().numpy()
        detections = []
        for i in range(b):
            n = int(head[i, 0])
            if n == face_ops.NMS_INDEX_ERROR:
                raise IndexError(f"index {TOP_K} is out of bounds for axis 1 with size {TOP_K}")     # (the host walk's own error)
            if n == face_ops.NMS_OVER_CAP:
                faces = detect_faces_rows(detect_output(det[i].cpu().numpy()[None])[0], width, height, self.conf_threshold)
            elif n <= NMS_HEAD:
                faces = head[i, 1:1 + n * 5].reshape(n, 5)
            else:
                faces = faces_dev[i, :n].cpu().numpy()
            detections.append(self._detection(faces))
        return detections

    def __call__(self, images: Sequence[np.ndarray]):
        return [[tuple(float(v) for v in box) for box in boxes] for boxes, _ in self.detect(images)]

    def release(self):
        if getattr(self, "det_net", None) is not None:
            self.det_net.close()
            self.det_net = None
