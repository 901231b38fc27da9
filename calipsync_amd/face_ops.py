"""The face pipeline's work between S3FD and PFLD on the device (csrc/face_ops.hip): thin wrappers over torch device tensors.

* ``resize_frames_u8(frames, dsize=None, fx=None)``: ``cv2.resize`` (INTER_LINEAR) of uint8 [B,H,W,3] frames, in either of its
  forms: ``dsize=(dw, dh)`` or ``fx`` (= fy) with the size cv2 would choose.
* ``face_crops192(frames, geom)``: the 192 x 192 PFLD crops of the records ``{frame, x1, y1, w, h}``.
* ``s3fd_candidates(det, thresh, cap)``: per frame the rows of the dense ``det`` above ``thresh``, in prior order.
* ``landmarks_finalize(y, mean_face, geom)``: PFLD's output to int32 landmarks in frame pixels.
* ``s3fd_nms(counts, rows, width, height, conf_th)``: S3FD's two NMS passes on those candidate rows (csrc/face_nms.hip): per
  frame a status and the float64 face rows ``S3FD.detect_faces`` returns, bit for bit ``facedet.detect_output`` +
  ``facedet.detect_faces_rows`` (tests/test_face_nms_gpu.py).

The arithmetic is OpenCV's as ``oracle/frame_ops_oracle.py`` restates it (bit for bit: tests/test_face_ops_gpu.py); like the
frame loop's, it is not pinned against the real cv2.  Every call launches on the current stream and does not synchronise.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

FACE = 192
GEOM_WORDS = 5          # frame, x1, y1, w, h
NMS_TOP_K = 750         # rows of faces / detect_out per frame (Detect.top_k)
NMS_MAX_CAP = 1024      # candidate rows per frame the NMS kernel takes
NMS_OVER_CAP, NMS_INDEX_ERROR = -1, -2      # status of a frame with more rows than cap / on which the reference raises IndexError


class FrameStager:
    """Host frames to one uint8 [B,H,W,3] device tensor through ONE pinned buffer and ONE copy; a device tensor passes
    through.  The buffer is kept and grown, and is not written again before the copy that last read it has finished."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._pinned: Optional[torch.Tensor] = None
        self._copied: Optional[torch.cuda.Event] = None

    def upload(self, frames, who: str, host_path: str) -> torch.Tensor:
        if isinstance(frames, torch.Tensor):
            if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError(f"{who}: frames {tuple(frames.shape)} {frames.dtype}, expected uint8 [B,H,W,3]")
            return frames.to(self.device).contiguous()
        frames = [np.asarray(f) for f in frames]
        if not frames:
            raise ValueError(f"{who}: no frames")
        shape = frames[0].shape
        if len(shape) != 3 or shape[2] != 3 or any(f.shape != shape for f in frames) or any(f.dtype != np.uint8 for f in frames):
            raise ValueError(f"{who}: needs uint8 frames of one size [H,W,3], got {sorted({(f.shape, str(f.dtype)) for f in frames})}; "
                             f"frames of mixed sizes go through {host_path}")
        n = len(frames) * int(np.prod(shape))
        if self._copied is not None:
            self._copied.synchronize()
        if self._pinned is None or self._pinned.numel() < n:
            self._pinned = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        stage = self._pinned[:n].view(len(frames), *shape)
        np.stack(frames, out=stage.numpy())
        dev = stage.to(self.device, non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record(torch.cuda.current_stream(self.device))
        return dev


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _frames(frames: torch.Tensor, who: str) -> torch.Tensor:
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_cuda:
        raise ValueError(f"{who}: frames must be a uint8 [B,H,W,3] device tensor")
    return frames.contiguous()


def scaled_size(h: int, w: int, fx: float) -> Tuple[int, int]:
    """(dw, dh) of cv2.resize(src, (0, 0), fx=fx, fy=fx): cvRound, i.e. round half to even"""
    return int(round(w * fx)), int(round(h * fx))


def resize_frames_u8(frames: torch.Tensor, dsize: Optional[Tuple[int, int]] = None, fx: Optional[float] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cv2.resize(frame, dsize) with dsize = (dw, dh), or cv2.resize(frame, (0, 0), fx=fx, fy=fx), on every frame of a uint8
    [B,H,W,3] device tensor -> [B,dh,dw,3]."""
    frames = _frames(frames, "resize_frames_u8")
    b, sh, sw = frames.shape[:3]
    if (dsize is None) == (fx is None):
        raise ValueError("resize_frames_u8: give dsize or fx, not both")
    if fx is not None:
        if not fx > 0:
            raise ValueError(f"resize_frames_u8: fx {fx}")
        if fx == 0.5 and (sh % 2 or sw % 2):
            # cv::resize takes its 2x INTER_AREA path from the scale alone here; what that path does on the odd last row or
            # column is not restated by the oracle, so it is refused rather than guessed
            raise ValueError(f"resize_frames_u8: fx=0.5 on an odd side ({sh} x {sw}) is not pinned")
        dw, dh = scaled_size(sh, sw, fx)
        scale_x = scale_y = 1.0 / fx
    else:
        dw, dh = int(dsize[0]), int(dsize[1])
        if dw < 1 or dh < 1:
            raise ValueError(f"resize_frames_u8: dsize {dsize}")
        scale_x, scale_y = 1.0 / (float(dw) / float(sw)), 1.0 / (float(dh) / float(sh))
    if out is None:
        out = torch.empty((b, max(dh, 0), max(dw, 0), 3), dtype=torch.uint8, device=frames.device)
    if b == 0:
        return out
    st = _lib.load().casync_op_resize_linear_u8(frames.data_ptr(), b, sh, sw, out.data_ptr(), dh, dw, scale_x, scale_y,
                                                _stream(frames.device))
    _lib.check(st, "casync_op_resize_linear_u8")
    return out


def _geom(geom, who: str) -> np.ndarray:
    g = np.ascontiguousarray(np.asarray(geom, dtype=np.int32))
    if g.ndim != 2 or g.shape[1] != GEOM_WORDS:
        raise ValueError(f"{who}: geom must be [n,{GEOM_WORDS}] (frame, x1, y1, w, h), got {g.shape}")
    return g


def face_crops192(frames: torch.Tensor, geom, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frames uint8 [B,H,W,3] on the device, geom [n,5] int32 on the host = (frame, x1, y1, w, h) -> crops [n,192,192,3]: crop i
    is cv2.resize to (192, 192) of the h x w window at (x1, y1) of its frame, zero where the window leaves the frame."""
    frames = _frames(frames, "face_crops192")
    g = _geom(geom, "face_crops192")
    n = g.shape[0]
    if out is None:
        out = torch.empty((n, FACE, FACE, 3), dtype=torch.uint8, device=frames.device)
    if n == 0:
        return out
    st = _lib.load().casync_op_face_crops192(frames.data_ptr(), frames.shape[0], frames.shape[1], frames.shape[2], g.ctypes.data, n,
                                             out.data_ptr(), _stream(frames.device))
    _lib.check(st, "casync_op_face_crops192")
    return out


def s3fd_candidates(det: torch.Tensor, thresh: float, cap: int, counts: Optional[torch.Tensor] = None,
                    rows: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """det [B,P,5] float32 on the device -> (counts [B] int32, rows [B,cap,5]): rows[b, :min(counts[b], cap)] are the rows of
    det[b] with a score above thresh, in prior order; the rest of rows is not written."""
    if not isinstance(det, torch.Tensor) or det.dtype != torch.float32 or det.dim() != 3 or det.shape[2] != 5 or not det.is_cuda:
        raise ValueError("s3fd_candidates: det must be a float32 [B,P,5] device tensor")
    det = det.contiguous()
    b, p = det.shape[:2]
    cap = int(cap)
    if counts is None:
        counts = torch.empty((b,), dtype=torch.int32, device=det.device)
    if rows is None:
        rows = torch.empty((b, max(cap, 0), 5), dtype=torch.float32, device=det.device)
    if b == 0:
        return counts, rows
    st = _lib.load().casync_op_s3fd_candidates(det.data_ptr(), b, p, float(thresh), cap, counts.data_ptr(), rows.data_ptr(),
                                               _stream(det.device))
    _lib.check(st, "casync_op_s3fd_candidates")
    return counts, rows


def s3fd_nms(counts: torch.Tensor, rows: torch.Tensor, width: int, height: int, conf_th: float, status: Optional[torch.Tensor] = None,
             faces: Optional[torch.Tensor] = None, detect_out: Optional[torch.Tensor] = None, detect_n: Optional[torch.Tensor] = None):
    """counts [B] int32 and rows [B,cap,5] float32 on the device, as s3fd_candidates wrote them -> (status [B] int32, faces
    [B,750,5] float64): faces[b, :status[b]] = (x1, y1, x2, y2, score) of frame b in pixels of the width x height frame, what
    facedet.detect_faces_rows(facedet.detect_output(rows[b, :counts[b]])) returns; status NMS_OVER_CAP (-1) where counts[b] >
    cap (nothing written), NMS_INDEX_ERROR (-2) where 750 rows pass conf_th.  Rows behind status[b] are not written.
    With detect_out [B,750,5] float32 and detect_n [B] int32 given, they also receive Detect.forward's kept rows (score, box) and
    their number, and the call returns (status, faces, detect_out, detect_n)."""
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float32 or rows.dim() != 3 or rows.shape[2] != 5 or not rows.is_cuda:
        raise ValueError("s3fd_nms: rows must be a float32 [B,cap,5] device tensor")
    b, cap = rows.shape[:2]
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or tuple(counts.shape) != (b,) or counts.device != rows.device:
        raise ValueError(f"s3fd_nms: counts must be {b} int32 values on rows' device")
    if not 1 <= cap <= NMS_MAX_CAP:
        raise ValueError(f"s3fd_nms: {cap} rows per frame, the kernel takes 1..{NMS_MAX_CAP}")
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError(f"s3fd_nms: frame of {width} x {height} (w x h)")
    rows, counts = rows.contiguous(), counts.contiguous()
    if (detect_out is None) != (detect_n is None):
        raise ValueError("s3fd_nms: detect_out and detect_n go together")
    stage1 = detect_out is not None

    def given(t, shape, dtype, name):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=rows.device)
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or t.device != rows.device or not t.is_contiguous():
            raise ValueError(f"s3fd_nms: {name} must be a contiguous {dtype} {list(shape)} tensor on rows' device")
        return t

    status = given(status, (b,), torch.int32, "status")
    faces = given(faces, (b, NMS_TOP_K, 5), torch.float64, "faces")
    if stage1:
        detect_out = given(detect_out, (b, NMS_TOP_K, 5), torch.float32, "detect_out")
        detect_n = given(detect_n, (b,), torch.int32, "detect_n")
    if b:
        st = _lib.load().casync_op_s3fd_nms(rows.data_ptr(), counts.data_ptr(), b, cap, width, height, float(conf_th), status.data_ptr(),
                                            faces.data_ptr(), detect_out.data_ptr() if stage1 else None,
                                            detect_n.data_ptr() if stage1 else None, _stream(rows.device))
        _lib.check(st, "casync_op_s3fd_nms")
    return (status, faces, detect_out, detect_n) if stage1 else (status, faces)


def landmarks_finalize(y: torch.Tensor, mean_face: torch.Tensor, geom, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y [n,220] and mean_face [220] float32 on the device, geom [n,5] on the host -> int32 [n,110,2] =
    int32((y + mean_face) * (w, h) + (x1, y1)) in float32."""
    if not isinstance(y, torch.Tensor) or y.dtype != torch.float32 or y.dim() != 2 or y.shape[1] != 220 or not y.is_cuda:
        raise ValueError("landmarks_finalize: y must be a float32 [n,220] device tensor")
    if not isinstance(mean_face, torch.Tensor) or mean_face.dtype != torch.float32 or mean_face.numel() != 220 or mean_face.device != y.device:
        raise ValueError("landmarks_finalize: mean_face must be 220 float32 values on y's device")
    g = _geom(geom, "landmarks_finalize")
    n = y.shape[0]
    if g.shape[0] != n:
        raise ValueError(f"landmarks_finalize: {n} rows, {g.shape[0]} geometry records")
    y, mean_face = y.contiguous(), mean_face.contiguous()
    if out is None:
        out = torch.empty((n, 110, 2), dtype=torch.int32, device=y.device)
    if n == 0:
        return out
    st = _lib.load().casync_op_landmarks_finalize(y.data_ptr(), mean_face.data_ptr(), g.ctypes.data, n, out.data_ptr(), _stream(y.device))
    _lib.check(st, "casync_op_landmarks_finalize")
    return out
