"""The trainer's loss on the HIP engine: L1 + the VGG19 perceptual term of the reference's step, with its gradient
(step2_train_unet.py:12-36,107-112; include/casync_ploss.h).

* ``manifest()`` names the fourteen tensors of ``vgg19().features[:15]`` the loss reads; ``pack`` writes them into the handle's
  packed buffer (``casync_ploss_packed_*``) and ignores every other key of a vgg19 state dict.
* ``PerceptualEngine`` is the handle: ``forward`` / ``backward`` and the taps of both directions.
* ``PerceptualLoss(loss, vgg_path)`` with ``get_loss(fakeIm, realIm)`` is the reference's class and signature;
  ``TrainingLoss(vgg_path)`` returns ``(loss, loss_pixel, loss_perceptual)`` of a step from one forward.  Both go through one
  ``torch.autograd.Function``: the gradient reaches the prediction only.  The VGG is frozen -- the gradients of its weights,
  which the reference accumulates and never reads, are not computed -- and the label gets none.

Inputs are contiguous float32 [B,3,H,W] tensors on a ROCm device, H, W >= 4.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .engine_base import _PackedEngine

# nn.Conv2d(cin, cout, 3, padding=1) of vgg19().features by index, with the engine's name; a ReLU follows all but the last, a
# MaxPool2d(2, 2) follows features.3 and features.8
VGG_CONVS = ((0, "conv1_1", 3, 64), (2, "conv1_2", 64, 64), (5, "conv2_1", 64, 128), (7, "conv2_2", 128, 128), (10, "conv3_1", 128, 256),
             (12, "conv3_2", 256, 256), (14, "conv3_3", 256, 256))
FORWARD_STAGES = ("conv1_1", "conv1_2", "pool1", "conv2_1", "conv2_2", "pool2", "conv3_1", "conv3_2", "conv3_3", "d")
BACKWARD_STAGES = ("conv3_3T", "mask3_2", "conv3_2T", "mask3_1", "conv3_1T", "pool2T", "conv2_2T", "mask2_1", "conv2_1T", "pool1T", "conv1_2T",
                   "mask1_1", "grad_pred")
PERCEPTUAL_WEIGHT = 0.1          # step2_train_unet.py:111


def manifest() -> List[Tuple[str, Tuple[int, ...]]]:
    """[(key, shape)] of the entries of a vgg19 state dict the loss needs, in the state dict's order."""
    keys: List[Tuple[str, Tuple[int, ...]]] = []
    for idx, _name, cin, cout in VGG_CONVS:
        keys += [(f"features.{idx}.weight", (cout, cin, 3, 3)), (f"features.{idx}.bias", (cout,))]
    return keys


def _f32(v) -> np.ndarray:
    return np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v), dtype=np.float32)


def packed_tensors(sd) -> Dict[str, np.ndarray]:
    """The engine's named tensors: conv1_1.w [(ky,kx,cin)][64], the others [cout][ky][kx][cin].  ValueError naming the first
    missing key or wrong shape; keys the loss does not need (the rest of vgg19) are ignored."""
    out: Dict[str, np.ndarray] = {}
    for key, shape in manifest():
        if key not in sd:
            raise ValueError(f"vgg19 state dict lacks {key}")
        if tuple(sd[key].shape) != shape:
            raise ValueError(f"vgg19 state dict: {key} has shape {tuple(sd[key].shape)}, vgg19 has {shape}")
    for idx, name, _cin, cout in VGG_CONVS:
        rows = _f32(sd[f"features.{idx}.weight"]).transpose(0, 2, 3, 1).reshape(cout, -1)
        out[f"{name}.w"] = np.ascontiguousarray(rows.T if name == "conv1_1" else rows)
        out[f"{name}.b"] = _f32(sd[f"features.{idx}.bias"])
    return out


def pack(sd) -> np.ndarray:
    """The flat float32 buffer casync_ploss_load_weights_* takes."""
    from . import _lib
    return _lib.pack_named(packed_tensors(sd), _lib.ploss_layout())


def weight_transform(w: np.ndarray, cout: int, cin: int) -> np.ndarray:
    """The numpy twin of casync_op_ploss_weight_transform: [cout][ky][kx][cin] -> [cin][2-ky][2-kx][cout] (flat in, flat out).
    The backward-data pass of a stride-1 pad-1 3x3 conv is the same conv on this matrix."""
    w = np.asarray(w).reshape(cout, 3, 3, cin)
    return np.ascontiguousarray(w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0)).reshape(-1)


def _check_pair(what: str, pred: torch.Tensor, label: torch.Tensor) -> Tuple[int, int, int]:
    for name, t in (("prediction", pred), ("label", label)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 3:
            raise RuntimeError(f"{what}: the {name} must be a float32 [B,3,H,W] tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{what}: the {name} must be on a ROCm device (no CPU fallback)")
        if not t.is_contiguous():
            raise RuntimeError(f"{what}: the {name} must be contiguous")
    if pred.shape != label.shape or pred.device != label.device:
        raise RuntimeError(f"{what}: prediction {tuple(pred.shape)} on {pred.device}, label {tuple(label.shape)} on {label.device}")
    b, _, h, w = pred.shape
    if b < 1 or h < 4 or w < 4:
        raise RuntimeError(f"{what}: {b} image(s) of {h} x {w} (one image of 4 x 4 at least)")
    return int(b), int(h), int(w)


class PerceptualEngine(_PackedEngine):
    """The casync_ploss handle.  Every call runs on torch's current stream, takes its buffers from torch's allocator and does not
    synchronise."""

    _destroy = "casync_ploss_destroy"

    def __init__(self, sd, device="cuda:0"):
        buf = pack(sd)                 # (checks the state dict before any device call)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"PerceptualEngine: device {device} (a ROCm device; no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._open(device, "casync_ploss_create", (), "casync_ploss_load_weights_host", buf)

    def saved_bytes(self, b: int, h: int, w: int) -> int:
        return self._lib.casync_ploss_saved_bytes(b, h, w)

    def scratch_bytes(self, b: int, h: int, w: int) -> int:
        return self._lib.casync_ploss_scratch_bytes(b, h, w)

    def _bytes(self, n: int) -> torch.Tensor:
        return torch.empty(max(int(n), 256), dtype=torch.uint8, device=self.device)     # (torch's blocks are 512-B aligned)

    def _scratch(self, b, h, w, scratch):
        return self._bytes(self.scratch_bytes(b, h, w)) if scratch is None else scratch

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def forward(self, pred, label, w_pix: float, w_perc: float, keep: bool = True, scratch=None, saved=None, losses=None):
        """-> (losses [3] = {total, pixel, perceptual} on the device, saved or None).  keep=False keeps nothing for a backward."""
        from . import _lib
        b, h, w = _check_pair("PerceptualEngine.forward", pred, label)
        ws = self._scratch(b, h, w, scratch)
        if keep and saved is None:
            saved = self._bytes(self.saved_bytes(b, h, w))
        if not keep:
            saved = None
        if losses is None:
            losses = torch.empty(3, dtype=torch.float32, device=self.device)
        st = self._lib.casync_ploss_forward(self._h, pred.data_ptr(), label.data_ptr(), b, h, w, w_pix, w_perc, losses.data_ptr(),
                                            saved.data_ptr() if saved is not None else None, saved.numel() if saved is not None else 0,
                                            ws.data_ptr(), ws.numel(), self._stream())
        _lib.check(st, "casync_ploss_forward")
        return losses, saved

    def backward(self, pred, label, grad_out, saved, w_pix: float, w_perc: float, scratch=None, out=None):
        """grad_out: a float32 device scalar -> d (grad_out * total) / d pred [B,3,H,W]"""
        from . import _lib
        b, h, w = _check_pair("PerceptualEngine.backward", pred, label)
        ws = self._scratch(b, h, w, scratch)
        if out is None:
            out = torch.empty_like(pred)
        st = self._lib.casync_ploss_backward(self._h, pred.data_ptr(), label.data_ptr(), grad_out.data_ptr(), out.data_ptr(), b, h, w, w_pix,
                                             w_perc, saved.data_ptr(), saved.numel(), ws.data_ptr(), ws.numel(), self._stream())
        _lib.check(st, "casync_ploss_backward")
        return out

    def tap_shape(self, backward: bool, stage: int, b: int, h: int, w: int) -> Tuple[int, ...]:
        h2, w2, h3, w3 = h // 2, w // 2, h // 2 // 2, w // 2 // 2
        if backward:
            return ([(b, h3, w3, 256)] * 4 + [(b, h3, w3, 128)] + [(b, h2, w2, 128)] * 3 + [(b, h2, w2, 64)] + [(b, h, w, 64)] * 3 +
                    [(b, 3, h, w)])[stage]
        shapes = [(h, w, 64), (h, w, 64), (h2, w2, 64), (h2, w2, 128), (h2, w2, 128), (h3, w3, 128), (h3, w3, 256), (h3, w3, 256), (h3, w3, 256)]
        return (b, h3, w3, 256) if stage == 9 else (2 * b,) + shapes[stage]

    def forward_tap(self, pred, label, stage, scratch=None) -> torch.Tensor:
        """One intermediate of the forward (a name or index of FORWARD_STAGES), NHWC: [2B, ...] -- the prediction's images, then
        the label's -- up to conv3_3, d [B,H/4,W/4,256]."""
        from . import _lib
        b, h, w = _check_pair("PerceptualEngine.forward_tap", pred, label)
        stage = FORWARD_STAGES.index(stage) if isinstance(stage, str) else int(stage)
        ws = self._scratch(b, h, w, scratch)
        out = torch.empty(self.tap_shape(False, stage, b, h, w), dtype=torch.float32, device=self.device)
        assert out.numel() == self._lib.casync_ploss_tap_floats(0, b, h, w, stage)
        st = self._lib.casync_ploss_forward_tap(self._h, pred.data_ptr(), label.data_ptr(), b, h, w, stage, out.data_ptr(), ws.data_ptr(),
                                                ws.numel(), self._stream())
        _lib.check(st, "casync_ploss_forward_tap")
        return out

    def backward_tap(self, pred, label, grad_out, saved, w_pix, w_perc, stage, scratch=None) -> torch.Tensor:
        """The gradient leaving one step of the backward (a name or index of BACKWARD_STAGES), NHWC; the last is grad_pred, NCHW."""
        from . import _lib
        b, h, w = _check_pair("PerceptualEngine.backward_tap", pred, label)
        stage = BACKWARD_STAGES.index(stage) if isinstance(stage, str) else int(stage)
        ws = self._scratch(b, h, w, scratch)
        out = torch.empty(self.tap_shape(True, stage, b, h, w), dtype=torch.float32, device=self.device)
        assert out.numel() == self._lib.casync_ploss_tap_floats(1, b, h, w, stage)
        st = self._lib.casync_ploss_backward_tap(self._h, pred.data_ptr(), label.data_ptr(), grad_out.data_ptr(), b, h, w, w_pix, w_perc,
                                                 saved.data_ptr(), saved.numel(), stage, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 self._stream())
        _lib.check(st, "casync_ploss_backward_tap")
        return out


class _LossFunction(torch.autograd.Function):
    """(pred, label) -> (total, pixel, perceptual), 0-dim views of the handle's losses[3].  Only `total` carries a gradient, to
    `pred` only."""

    @staticmethod
    def forward(ctx, pred, label, engine, w_pix, w_perc):
        losses, saved = engine.forward(pred, label, w_pix, w_perc, keep=True)
        ctx.engine, ctx.w = engine, (w_pix, w_perc)
        ctx.saved_bytes = saved            # the handle's `saved`: an output of this forward, an input of the backward
        ctx.save_for_backward(pred, label)
        total, pixel, perceptual = losses[0], losses[1], losses[2]
        ctx.mark_non_differentiable(pixel, perceptual)
        return total, pixel, perceptual

    @staticmethod
    def backward(ctx, grad_total, _grad_pixel, _grad_perceptual):
        pred, label = ctx.saved_tensors
        g = grad_total.to(torch.float32).contiguous()      # a device scalar: no host round trip
        grad = ctx.engine.backward(pred, label, g, ctx.saved_bytes, *ctx.w)
        return grad, None, None, None, None


def _apply(engine, pred, label, w_pix, w_perc):
    _check_pair("calipsync_amd.losses", pred, label)
    if pred.device != engine.device:
        raise RuntimeError(f"calipsync_amd.losses: tensors on {pred.device}, the loss on {engine.device}")
    # under no_grad, or for a prediction that needs no gradient, nothing is saved (asked here: inside Function.forward autograd
    # has switched gradients off)
    if not (torch.is_grad_enabled() and pred.requires_grad):
        losses, _ = engine.forward(pred, label, w_pix, w_perc, keep=False)
        return losses[0], losses[1], losses[2]
    return _LossFunction.apply(pred, label.detach(), engine, w_pix, w_perc)


def _load_state_dict(vgg_path, state_dict):
    if (vgg_path is None) == (state_dict is None):
        raise ValueError("calipsync_amd.losses: give vgg_path (a torch.load-able vgg19 state dict) or state_dict, one of them")
    if state_dict is not None:
        return state_dict
    sd = torch.load(vgg_path, map_location="cpu")
    return sd.state_dict() if hasattr(sd, "state_dict") else sd


class PerceptualLoss:
    """The reference's PerceptualLoss (step2_train_unet.py:12-36): ``get_loss(fakeIm, realIm)`` = loss(F(fakeIm), F(realIm).detach())
    with F = vgg19().features[:15].  `loss` must be a mean-reduction ``torch.nn.MSELoss``: that is what the handle computes."""

    def __init__(self, loss, vgg_path=None, *, state_dict=None, device=None):
        if not isinstance(loss, torch.nn.MSELoss) or loss.reduction != "mean":
            raise ValueError("PerceptualLoss: the criterion must be torch.nn.MSELoss() with reduction='mean' (the handle computes the mean "
                             f"squared feature difference), got {loss!r}")
        self.criterion = loss
        self.engine = PerceptualEngine(_load_state_dict(vgg_path, state_dict), device or "cuda:0")

    def get_loss(self, fakeIm, realIm):
        return _apply(self.engine, fakeIm, realIm, 0.0, 1.0)[0]       # total = 0 * 0 + 1 * perceptual: the perceptual term's bits


class TrainingLoss:
    """The loss of a training step (step2_train_unet.py:107-112): ``loss, loss_pixel, loss_perceptual = TrainingLoss(path)(preds,
    labels)`` with loss = pixel_weight * L1 + perceptual_weight * perceptual, from one forward; ``loss.backward()`` reaches preds."""

    def __init__(self, vgg_path=None, perceptual_weight: float = PERCEPTUAL_WEIGHT, pixel_weight: float = 1.0, *, state_dict=None,
                 device=None):
        self.perceptual_weight, self.pixel_weight = float(perceptual_weight), float(pixel_weight)
        self.engine = PerceptualEngine(_load_state_dict(vgg_path, state_dict), device or "cuda:0")

    def __call__(self, preds, labels):
        return _apply(self.engine, preds, labels, self.pixel_weight, self.perceptual_weight)
