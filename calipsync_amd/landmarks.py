"""110-point face landmarks on the HIP engine: the drop-in for the reference's ``LipDetector``
(utils/lip_detector/lip_detector.py:9-120) without the reference tree.

* ``check_state_dict(sd)`` accepts a ``PFLD_GhostOne(0.5, 192, 110)`` checkpoint in its train form (2090 keys, every
  MobileOneBlock with its branches) or in the inference form the reference's own ``reparameterize()`` leaves (107 keys).
* ``fold(sd)`` folds every MobileOneBlock into one conv + bias (base_module.py:329-400) in float64.
* ``pack`` / ``unpack`` write the folded convs into the engine's packed buffer (``casync_pfld_packed_*``).
* ``PFLDEngine`` runs the network on float NCHW input or on uint8 BGR crops.
* ``LandmarkDetector`` keeps ``LipDetector.detect_landmarks``.  Face detection stays outside: boxes or a detector callable
  are handed in.  The 192 x 192 resize uses ``cv2.resize`` where cv2 imports, else Pillow's bilinear filter; cv2 is not in
  the build image, so that step is NOT pinned against the reference, like the f1 resize of the frame loop.
* ``LandmarkDetector.detect_landmarks_device`` is the same call on frames resident on the device: crops,
  resize and the closing arithmetic are kernels (``calipsync_amd.face_ops``) with OpenCV's resize arithmetic on every box.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .engine_base import _PackedEngine

INPUT_SIZE = 192
N_LANDMARKS = 110
BN_EPS = 1e-5                      # nn.BatchNorm2d's default, what every block of the reference is built with
BRANCHES = 6                       # num_conv_branches of PFLD_GhostOne
# GhostOneBottleneck(in, hidden, out, stride) of pfld_mobileone.py:59-72 at width_factor 0.5
BOTTLENECKS = (("conv3_1", 32, 48, 40, 2), ("conv3_2", 40, 60, 40, 1), ("conv3_3", 40, 60, 40, 1),
               ("conv4_1", 40, 100, 48, 2), ("conv4_2", 48, 120, 48, 1), ("conv4_3", 48, 120, 48, 1),
               ("conv5_1", 48, 168, 72, 2), ("conv5_2", 72, 252, 72, 1), ("conv5_3", 72, 252, 72, 1), ("conv5_4", 72, 252, 72, 1),
               ("conv6", 72, 108, 8, 1))
STAGES = ("conv1", "conv2") + tuple(b[0] for b in BOTTLENECKS) + ("conv7", "conv8", "conv_out")   # casync_pfld_forward_tap
STAGE_SHAPES = ((96, 96, 32), (96, 96, 32)) + ((48, 48, 40),) * 3 + ((24, 24, 48),) * 3 + ((12, 12, 72),) * 4 + \
    ((12, 12, 8), (12, 12, 16), (1, 1, 64), (1, 1, 220))                                            # (H, W, C), NHWC
_EXTRA = (("conv8.0.weight", (64, 16, 12, 12)), ("conv_out.weight", (220, 256, 1, 1)), ("conv_out.bias", (220,)),
          ("localization.0.weight", (8, 1, 7, 7)), ("localization.0.bias", (8,)),
          ("localization.3.weight", (10, 8, 5, 5)), ("localization.3.bias", (10,)))   # localization.*: never used by forward


def blocks() -> List[Tuple[str, int, int, int, int, int]]:
    """The 50 MobileOneBlocks in state-dict order: (prefix, cin, cout, kernel, stride, groups)."""
    out = [("conv1", 3, 32, 3, 2, 1), ("conv2", 32, 32, 3, 1, 32)]
    for name, cin, hid, cout, s in BOTTLENECKS:
        p = f"{name}.ghost_conv"
        out += [(f"{p}.0.primary_conv", cin, hid // 2, 1, 1, 1), (f"{p}.0.cheap_operation", hid // 2, hid // 2, 3, 1, hid // 2)]
        if s == 2:
            out.append((f"{p}.1", hid, hid, 3, 2, hid))
        out += [(f"{p}.2.primary_conv", hid, cout // 2, 1, 1, 1), (f"{p}.2.cheap_operation", cout // 2, cout // 2, 3, 1, cout // 2)]
    out.append(("conv7", 8, 16, 3, 1, 1))
    return out


def _bn_keys(p: str, c: int):
    return [(f"{p}.weight", (c,)), (f"{p}.bias", (c,)), (f"{p}.running_mean", (c,)), (f"{p}.running_var", (c,)),
            (f"{p}.num_batches_tracked", ())]


def _branches(p: str, cin: int, cout: int, k: int, stride: int, groups: int):
    """(has skip, [(branch prefix, kernel size)]) of one train-form block"""
    br = [(f"{p}.rbr_conv.{i}", k) for i in range(BRANCHES)]
    if k > 1:
        br.append((f"{p}.rbr_scale", 1))
    return cin == cout and stride == 1, br


def manifest(form: str = "train") -> List[Tuple[str, Tuple[int, ...]]]:
    """[(key, shape)] of the state dict in the reference's order: form 'train' (2090 keys) or 'inference' (107)."""
    if form not in ("train", "inference"):
        raise ValueError(f"PFLD state-dict form {form!r} ('train' or 'inference')")
    keys: List[Tuple[str, Tuple[int, ...]]] = []
    for p, cin, cout, k, stride, groups in blocks():
        if form == "inference":
            keys += [(f"{p}.reparam_conv.weight", (cout, cin // groups, k, k)), (f"{p}.reparam_conv.bias", (cout,))]
            continue
        skip, br = _branches(p, cin, cout, k, stride, groups)
        if skip:
            keys += _bn_keys(f"{p}.rbr_skip", cin)
        for bp, bk in br:
            keys.append((f"{bp}.conv.weight", (cout, cin // groups, bk, bk)))
            keys += _bn_keys(f"{bp}.bn", cout)
    return keys + list(_EXTRA)


def check_state_dict(sd) -> str:
    """-> 'train' or 'inference'; ValueError naming the first missing or unexpected key (or wrong shape) otherwise.
    Only PFLD_GhostOne(width_factor=0.5, input_size=192, landmark_number=110) is accepted: any other width, input size or
    landmark count, and PFLD_GhostOne_WithSTN, differ in a key or a shape."""
    form = "inference" if "conv1.reparam_conv.weight" in sd else "train"
    want = manifest(form)
    for key, shape in want:
        if key.endswith("num_batches_tracked"):      # ignored: there or not, whatever its shape
            continue
        if key not in sd:
            raise ValueError(f"PFLD checkpoint ({form} form) lacks {key}")
        if tuple(sd[key].shape) != shape:
            raise ValueError(f"PFLD checkpoint: {key} has shape {tuple(sd[key].shape)}, PFLD_GhostOne(0.5, 192, 110) has {shape}")
    names = {k for k, _ in want}
    for key in sd:
        if key not in names:
            raise ValueError(f"PFLD checkpoint ({form} form) has an unexpected key {key}")
    return form


def _f64(v) -> np.ndarray:
    return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float64)


def _fuse_bn(sd, p: str, kernel: np.ndarray):
    """base_module.py:363-400 (_fuse_bn_tensor) in float64"""
    gamma, beta, mean, var = (_f64(sd[f"{p}.{n}"]) for n in ("weight", "bias", "running_mean", "running_var"))
    std = np.sqrt(var + BN_EPS)
    return kernel * (gamma / std).reshape(-1, 1, 1, 1), beta - mean * gamma / std


def fold(sd, dtype=np.float32) -> Dict[str, np.ndarray]:
    """The plain convs of the eval-mode network: {"<block>.w" [cout, cin/groups, k, k], "<block>.b" [cout]} for the 50
    blocks, "conv8.w", "conv_out.w", "conv_out.b".  Train form: the RepVGG algebra of _get_kernel_bias (base_module.py:
    329-361) in float64 -- the conv branches summed, the 1x1 scale branch zero-padded to k x k, the skip as an identity
    kernel with i % (cin / groups) indexing -- rounded once to `dtype`."""
    form = check_state_dict(sd)
    out: Dict[str, np.ndarray] = {}
    for p, cin, cout, k, stride, groups in blocks():
        if form == "inference":
            w, b = _f64(sd[f"{p}.reparam_conv.weight"]), _f64(sd[f"{p}.reparam_conv.bias"])
        else:
            skip, br = _branches(p, cin, cout, k, stride, groups)
            w, b = np.zeros((cout, cin // groups, k, k)), np.zeros(cout)
            for bp, bk in br:
                kw, kb = _fuse_bn(sd, f"{bp}.bn", _f64(sd[f"{bp}.conv.weight"]))
                pad = (k - bk) // 2
                w += np.pad(kw, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
                b += kb
            if skip:
                dim = cin // groups
                ident = np.zeros((cin, dim, k, k))
                ident[np.arange(cin), np.arange(cin) % dim, k // 2, k // 2] = 1.0
                kw, kb = _fuse_bn(sd, f"{p}.rbr_skip", ident)
                w += kw
                b += kb
        out[f"{p}.w"], out[f"{p}.b"] = w.astype(dtype), b.astype(dtype)
    out["conv8.w"] = _f64(sd["conv8.0.weight"]).astype(dtype)
    out["conv_out.w"] = _f64(sd["conv_out.weight"]).astype(dtype)
    out["conv_out.b"] = _f64(sd["conv_out.bias"]).astype(dtype)
    return out


def to_inference_form(sd) -> Dict[str, np.ndarray]:
    """The 107-key inference form of a checkpoint: what the reference's reparameterize() leaves, from our own fold."""
    f = fold(sd)
    out: Dict[str, np.ndarray] = {}
    for p, *_ in blocks():
        out[f"{p}.reparam_conv.weight"], out[f"{p}.reparam_conv.bias"] = f[f"{p}.w"], f[f"{p}.b"]
    out["conv8.0.weight"], out["conv_out.weight"], out["conv_out.bias"] = f["conv8.w"], f["conv_out.w"], f["conv_out.b"]
    for key, _shape in _EXTRA[3:]:
        out[key] = np.asarray(_f64(sd[key]), dtype=np.float32)
    return out


def _ceil(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def packed_tensors(sd) -> Dict[str, np.ndarray]:
    """The engine's named tensors (include/casync_hip.h, casync_pfld_packed_*): channels-last, the pointwise matrices
    zero-padded to the fp32 MFMA granule (K to 16 rows, N to 16 columns)."""
    f = fold(sd)
    out: Dict[str, np.ndarray] = {}

    def taps(w):        # depthwise [c, 1, 3, 3] -> [9][c]
        return w[:, 0].reshape(w.shape[0], 9).T

    def dense(w):       # [cout, cin, kh, kw] -> [(ky, kx, ci)][cout]
        return w.transpose(2, 3, 1, 0).reshape(-1, w.shape[0])

    def padded(a, rows, cols):
        z = np.zeros((rows, cols), dtype=np.float32)
        z[:a.shape[0], :a.shape[1]] = a
        return z

    out["conv1.w"], out["conv1.b"] = dense(f["conv1.w"]), f["conv1.b"]
    out["conv2.w"], out["conv2.b"] = taps(f["conv2.w"]), f["conv2.b"]
    for name, cin, hid, cout, s in BOTTLENECKS:
        for g, idx, ci, co in (("g1", 0, cin, hid), ("g2", 2, hid, cout)):
            p, half = f"{name}.ghost_conv.{idx}", co // 2
            np_ = _ceil(half, 16)
            out[f"{name}.{g}.pw.w"] = padded(f[f"{p}.primary_conv.w"][:, :, 0, 0].T, _ceil(ci, 16), np_)
            out[f"{name}.{g}.pw.b"] = padded(f[f"{p}.primary_conv.b"][None], 1, np_)
            out[f"{name}.{g}.dw.w"] = padded(taps(f[f"{p}.cheap_operation.w"]), 9, np_)
            out[f"{name}.{g}.dw.b"] = padded(f[f"{p}.cheap_operation.b"][None], 1, np_)
        if s == 2:
            out[f"{name}.dw.w"], out[f"{name}.dw.b"] = taps(f[f"{name}.ghost_conv.1.w"]), f[f"{name}.ghost_conv.1.b"]
    out["conv7.w"], out["conv7.b"] = dense(f["conv7.w"]), f["conv7.b"]
    out["conv8.w"] = dense(f["conv8.w"])
    out["conv_out.w"], out["conv_out.b"] = f["conv_out.w"][:, :, 0, 0].T, f["conv_out.b"]
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def pack(sd) -> np.ndarray:
    """The flat float32 buffer casync_pfld_load_weights_* takes, from either checkpoint form."""
    from . import _lib
    return _lib.pack_named(packed_tensors(sd), _lib.pfld_layout())


def unpack(buf: np.ndarray) -> Dict[str, np.ndarray]:
    """Inverse of pack (flat shapes)."""
    from . import _lib
    return _lib.unpack_named(buf, _lib.pfld_layout())


class PFLDEngine(_PackedEngine):
    """PFLD_GhostOne().eval() on the HIP engine: forward(x [B,3,192,192] float in [0,1]) or forward_u8(crops [B,192,192,3]
    uint8 BGR) -> [B,220] on the device.  There is no CPU path."""

    _destroy = "casync_pfld_destroy"

    def __init__(self, sd, device: str = "cuda:0"):
        buf = pack(sd)                 # (checks the checkpoint before any device call)
        self._open(device, "casync_pfld_create", (), "casync_pfld_load_weights_host", buf)

    def workspace_bytes(self, batch: int) -> int:
        need = self._lib.casync_pfld_workspace_bytes(batch)
        if need <= 0:
            raise ValueError(f"PFLD engine: batch {batch} (1..4096)")
        return need

    def _workspace(self, batch: int) -> torch.Tensor:
        return self._grow_workspace(self.workspace_bytes(batch))

    def _run(self, x: torch.Tensor, u8: bool, stage: Optional[int], out: Optional[torch.Tensor], ws: Optional[torch.Tensor]):
        from . import _lib
        b = x.shape[0]
        ws = self._workspace(b) if ws is None else ws
        last = len(STAGES) - 1
        stage = last if stage is None else STAGES.index(stage) if isinstance(stage, str) else int(stage)
        if out is None:
            h, w, c = STAGE_SHAPES[stage]
            out = torch.empty((b, 220) if stage == last else (b, h, w, c), dtype=torch.float32, device=self.device)
        strm = torch.cuda.current_stream(self.device).cuda_stream
        st = self._lib.casync_pfld_forward_tap(self._h, x.data_ptr(), int(u8), b, stage, out.data_ptr(), ws.data_ptr(),
                                               ws.numel() * ws.element_size(), strm)
        _lib.check(st, "casync_pfld_forward")
        return out

    def forward(self, x: torch.Tensor, stage=None, out=None, workspace=None) -> torch.Tensor:
        """x [B,3,192,192] float -> landmarks [B,220]; stage (name or index of STAGES) = that NHWC intermediate instead."""
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, INPUT_SIZE, INPUT_SIZE):
            raise ValueError(f"PFLD engine: input {tuple(x.shape)}, expected [B,3,{INPUT_SIZE},{INPUT_SIZE}]")
        return self._run(x.to(self.device, torch.float32).contiguous(), False, stage, out, workspace)

    def forward_u8(self, crops, stage=None, out=None, workspace=None) -> torch.Tensor:
        """crops [B,192,192,3] uint8 BGR (numpy or tensor) -> landmarks [B,220]; the division by 255 happens on the device."""
        crops = torch.as_tensor(crops)
        if crops.dim() != 4 or tuple(crops.shape[1:]) != (INPUT_SIZE, INPUT_SIZE, 3) or crops.dtype != torch.uint8:
            raise ValueError(f"PFLD engine: crops {tuple(crops.shape)} {crops.dtype}, expected uint8 [B,{INPUT_SIZE},{INPUT_SIZE},3]")
        return self._run(crops.to(self.device).contiguous(), True, stage, out, workspace)

    __call__ = forward


def _read_state_dict(weight_base_dir: str):
    path = os.path.join(weight_base_dir, "checkpoint_epoch_335.pth.tar")
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if "pfld_backbone" not in ckpt:
        raise KeyError(f"{path} has no 'pfld_backbone' entry")
    return dict(ckpt["pfld_backbone"])


def _read_mean_face(weight_base_dir: str) -> np.ndarray:
    with open(os.path.join(weight_base_dir, "mean_face.txt"), "r") as f:
        return np.asarray(f.read().split(" "), dtype=np.float32)      # lip_detector.py:16-18


def resize192(crop: np.ndarray) -> np.ndarray:
    """cv2.resize(crop, (192, 192)) where cv2 imports, else Pillow's bilinear filter.  Not pinned against the reference."""
    try:
        import cv2
        return cv2.resize(crop, (INPUT_SIZE, INPUT_SIZE))
    except ImportError:
        from PIL import Image
        return np.asarray(Image.fromarray(crop).resize((INPUT_SIZE, INPUT_SIZE), Image.BILINEAR))


class LandmarkDetector:
    """The reference's LipDetector(weight_base_dir) on the HIP engine.  weight_base_dir holds ``mean_face.txt`` and
    ``checkpoint_epoch_335.pth.tar`` (its 'pfld_backbone' entry); or pass state_dict / mean_face.  face_detector(images) ->
    per image a list of (x, y, w, h) boxes; without one, detect_landmarks needs boxes."""

    def __init__(self, weight_base_dir: Optional[str] = None, *, state_dict=None, mean_face=None,
                 face_detector: Optional[Callable] = None, device: str = "cuda:0"):
        if state_dict is None:
            if weight_base_dir is None:
                raise ValueError("LandmarkDetector: weight_base_dir or state_dict is needed")
            state_dict = _read_state_dict(weight_base_dir)
        if mean_face is None:
            if weight_base_dir is None:
                raise ValueError("LandmarkDetector: weight_base_dir or mean_face is needed")
            mean_face = _read_mean_face(weight_base_dir)
        self.mean_face = np.asarray(mean_face, dtype=np.float32).reshape(-1)
        if self.mean_face.size != 2 * N_LANDMARKS:
            raise ValueError(f"mean_face has {self.mean_face.size} values, {2 * N_LANDMARKS} are needed")
        self.face_detector = face_detector
        self.pfld_backbone = self._make_engine(state_dict, device)
        self._stager = None             # detect_landmarks_device: the pinned upload buffer and mean_face on the device, made on first use

    @staticmethod
    def _make_engine(state_dict, device):
        return PFLDEngine(state_dict, device)

    @staticmethod
    def _crop(img: np.ndarray, box: Sequence[float]):
        """lip_detector.py:46-75: the 1.05 x square around the box, zero borders where it leaves the image.
        -> (crop, (offset_x, offset_y))"""
        height, width = img.shape[:2]
        x1, y1 = int(box[0]), int(box[1])
        w, h = int(box[2]), int(box[3])
        x2, y2 = x1 + w, y1 + h
        cx, cy = (x2 + x1) // 2, (y2 + y1) // 2
        size = int(max(w, h) * 1.05)
        x1, y1 = cx - size // 2, cy - size // 2
        x2, y2 = x1 + size, y1 + size
        dx, dy = max(0, -x1), max(0, -y1)
        x1, y1 = max(0, x1), max(0, y1)
        edx, edy = max(0, x2 - width), max(0, y2 - height)
        x2, y2 = min(width, x2), min(height, y2)
        cropped = img[y1:y2, x1:x2]
        if dx > 0 or dy > 0 or edx > 0 or edy > 0:
            cropped = np.pad(cropped, ((dy, edy), (dx, edx)) + ((0, 0),) * (img.ndim - 2))
            y1, x1 = y1 - dy, x1 - dx
        return cropped, (x1, y1)

    @staticmethod
    def _crop_geometry(height: int, width: int, box: Sequence[float]) -> Tuple[int, int, int, int]:
        """The integer arithmetic of _crop without the pixels -> (x1, y1, w, h): _crop(img, box) returns a crop of shape (h, w)
        at offset (x1, y1) whose pixel (y, x) is img[y1 + y, x1 + x] inside the image and 0 outside.  That includes squares
        that miss the image, where numpy's slice (a negative end counts from the far side) and the padding leave a crop that
        is not square."""
        bx, by = int(box[0]), int(box[1])
        bw, bh = int(box[2]), int(box[3])
        size = int(max(bw, bh) * 1.05)

        def axis(lo: int, extent: int):
            hi = lo + size
            before, after = max(0, -lo), max(0, hi - extent)
            lo, hi = max(0, lo), min(extent, hi)
            kept = len(range(*slice(lo, hi).indices(extent)))        # what img[lo:hi] keeps along this axis
            return lo - before, before + kept + after

        x1, w = axis((2 * bx + bw) // 2 - size // 2, width)
        y1, h = axis((2 * by + bh) // 2 - size // 2, height)
        return x1, y1, w, h

    def landmarks_from_crops(self, crops192_u8, sizes, offsets) -> List[np.ndarray]:
        """crops192_u8 [N,192,192,3] uint8 (one forward), sizes [(w, h)] of the crops before the resize, offsets [(x, y)]
        -> N int32 [110,2] arrays: lip_detector.py:106-114 in float32, truncated by astype(np.int32)."""
        y = self.pfld_backbone.forward_u8(crops192_u8)
        y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        out = []
        for row, (w, h), (ox, oy) in zip(y, sizes, offsets):
            pre = (row.astype(np.float32) + self.mean_face).reshape(-1, 2)
            pre[:, 0] *= w
            pre[:, 1] *= h
            pre[:, 0] += ox
            pre[:, 1] += oy
            out.append(pre.astype(np.int32))
        return out

    def detect_landmarks(self, images, boxes=None):
        """images: BGR uint8 arrays; boxes: per image a list of (x, y, w, h) (or None -> face_detector(images)).
        -> per image the list of its faces' int32 [110,2] landmarks, None for an image without a box.  All crops of the
        call run in ONE forward."""
        if boxes is None:
            if self.face_detector is None:
                raise ValueError("detect_landmarks: no boxes and no face_detector")
            boxes = self.face_detector(images)
        crops, sizes, offsets, owner = [], [], [], []
        for i, (img, bs) in enumerate(zip(images, boxes)):
            for box in (bs if bs is not None else []):
                crop, off = self._crop(img, box)
                h, w = crop.shape[:2]
                crops.append(resize192(np.ascontiguousarray(crop)))
                sizes.append((w, h))
                offsets.append(off)
                owner.append(i)
        results: List[Optional[List[np.ndarray]]] = [None] * len(images)
        if crops:
            for i, lm in zip(owner, self.landmarks_from_crops(np.stack(crops), sizes, offsets)):
                if results[i] is None:
                    results[i] = []
                results[i].append(lm)
        return results

    def detect_landmarks_device(self, frames, boxes=None):
        """detect_landmarks on frames resident on the device: frames is a uint8 [B,H,W,3] device tensor, or equal-sized numpy
        frames (uploaded once, and shared with face_detector.detect_device where the detector has it).  The crops are cut and
        resized, PFLD runs and the landmarks are scaled and truncated on the device; one download brings the int32 landmarks
        back.  Same return value as detect_landmarks."""
        from . import face_ops
        dev = self.pfld_backbone.device
        if self._stager is None:
            self._stager = face_ops.FrameStager(dev)
            self._mean_face_dev = torch.from_numpy(self.mean_face).to(dev)
        frames_dev = self._stager.upload(frames, "LandmarkDetector.detect_landmarks_device", "detect_landmarks")
        n_frames, height, width = frames_dev.shape[:3]
        if boxes is None:
            if self.face_detector is None:
                raise ValueError("detect_landmarks_device: no boxes and no face_detector")
            if hasattr(self.face_detector, "detect_device"):
                boxes = [[tuple(float(v) for v in box) for box in bs] for bs, _ in self.face_detector.detect_device(frames_dev)]
            else:
                boxes = self.face_detector(list(frames_dev.cpu().numpy()) if isinstance(frames, torch.Tensor) else list(frames))
        geom, owner = [], []
        for i, bs in zip(range(n_frames), boxes):
            for box in (bs if bs is not None else []):
                geom.append((i,) + self._crop_geometry(height, width, box))
                owner.append(i)
        results: List[Optional[List[np.ndarray]]] = [None] * n_frames
        if geom:
            table = np.asarray(geom, dtype=np.int32)
            y = self.pfld_backbone.forward_u8(face_ops.face_crops192(frames_dev, table))
            lms = face_ops.landmarks_finalize(y, self._mean_face_dev, table).cpu().numpy()
            for i, lm in zip(owner, lms):
                if results[i] is None:
                    results[i] = []
                results[i].append(lm.copy())
        return results


def write_lms(path: str, landmarks: np.ndarray) -> None:
    """The .lms file of lip_detector.py:152 (what frame_loop.crop_box reads)."""
    np.savetxt(path, landmarks, fmt="%d")
