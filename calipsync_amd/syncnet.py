"""The reference's lip-sync judge ``SyncNet_color`` (module/syncnet.py:155-246) on the HIP engine, without the reference tree.

* ``manifest(mode)`` / ``check_state_dict`` name the 217 keys of a ``SyncNet_color(mode)`` state dict: 31 blocks of
  ``conv(bias) -> BatchNorm2d -> (+ x) -> ReLU``, 17 in the face encoder and 14 in the audio encoder.
* ``fold`` folds every BatchNorm (eval, eps 1e-5) into its conv in float64; ``pack`` / ``unpack`` write the folded convs into
  the engine's packed buffer (``casync_sync_packed_*``).
* ``SyncNetEngine`` runs the network: both embeddings, or any of the 31 block outputs in the reference's NCHW order.
* ``SyncNetColor`` (alias ``SyncNet_color``) keeps the reference's call: ``forward(face_sequences, audio_sequences) ->
  (audio_embedding, face_embedding)``; ``similarity`` is the cosine of ``cosine_loss`` (syncnet.py:357-361), ``offset_curve``
  that cosine between face i and audio i + s over a range of shifts, ``score_clip`` the curve of a clip from its HuBERT features.

The reference snapshot holds no trained SyncNet weights: the recipe weights of the tests pin the arithmetic, not a threshold.
There is no CPU path.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .engine_base import _PackedEngine

FACE_HW = 160
EMBED_DIM = 4608                   # 512 channels x 3 x 3
BN_EPS = 1e-5                      # nn.BatchNorm2d's default
AUDIO_SHAPE = {"hubert": (32, 32, 32), "wenet": (256, 16, 32)}
MAX_SHIFT = 4096                   # casync_op_sync_curve's limit
PRECISIONS = {"fp32": 0, "bf16": 1}   # casync_syncnet_create_ex's numbers


def check_precision(precision: str) -> int:
    """-> the C ABI's number; ValueError for anything but "fp32" / "bf16" (before any device call)."""
    if not isinstance(precision, str) or precision not in PRECISIONS:
        raise ValueError(f"SyncNet precision {precision!r}; the engine has {sorted(PRECISIONS)}")
    return PRECISIONS[precision]


def _stage(cin, cout, stride, pad, n_res):
    return [(3, cin, cout, stride, pad, False)] + [(3, cout, cout, (1, 1), 1, True)] * n_res


def blocks(mode: str = "hubert") -> List[Tuple[str, int, int, int, Tuple[int, int], int, bool]]:
    """The 31 blocks in state-dict order: (prefix, kernel, cin, cout, (stride_h, stride_w), pad, residual)."""
    if mode not in AUDIO_SHAPE:
        raise ValueError(f"SyncNet mode {mode!r} ('hubert' or 'wenet')")
    s2 = (2, 2)
    face = [(7, 3, 32, (1, 1), 3, False), (5, 32, 64, s2, 1, False), (3, 64, 64, (1, 1), 1, True), (3, 64, 64, (1, 1), 1, True)]
    face += _stage(64, 128, s2, 1, 3) + _stage(128, 256, s2, 1, 2) + _stage(256, 512, s2, 1, 2)
    face += _stage(512, 512, s2, 1, 0) + _stage(512, 512, (1, 1), 0, 0) + [(1, 512, 512, (1, 1), 0, False)]
    p1, p2 = (32, s2) if mode == "hubert" else (256, (1, 2))
    audio = _stage(p1, 256, (1, 1), 1, 2) + _stage(256, 256, p2, 1, 2) + _stage(256, 256, s2, 2, 2) + _stage(256, 512, s2, 1, 2)
    audio += _stage(512, 512, (1, 1), 0, 0) + [(1, 512, 512, (1, 1), 0, False)]
    return [(f"face_encoder.{i}",) + b for i, b in enumerate(face)] + [(f"audio_encoder.{i}",) + b for i, b in enumerate(audio)]


def _short(prefix: str) -> str:
    return prefix.replace("_encoder", "")          # the engine's names: face.<i>, audio.<i>


STAGES = tuple(_short(b[0]) for b in blocks())     # casync_sync_forward_tap's stage numbers, the same in both modes


def stage_shapes(mode: str = "hubert") -> List[Tuple[int, int, int]]:
    """(C, H, W) of the 31 block outputs."""
    out = []
    for p, k, cin, cout, (sh, sw), pad, res in blocks(mode):
        if p.endswith(".0"):
            h, w = (FACE_HW, FACE_HW) if p.startswith("face") else AUDIO_SHAPE[mode][1:]
        h, w = (h + 2 * pad - k) // sh + 1, (w + 2 * pad - k) // sw + 1
        out.append((cout, h, w))
    return out


def manifest(mode: str = "hubert") -> List[Tuple[str, Tuple[int, ...]]]:
    """[(key, shape)] of the state dict in the reference's order (217 keys)."""
    keys: List[Tuple[str, Tuple[int, ...]]] = []
    for p, k, cin, cout, stride, pad, res in blocks(mode):
        keys += [(f"{p}.conv_block.0.weight", (cout, cin, k, k)), (f"{p}.conv_block.0.bias", (cout,))]
        keys += [(f"{p}.conv_block.1.{n}", (cout,)) for n in ("weight", "bias", "running_mean", "running_var")]
        keys.append((f"{p}.conv_block.1.num_batches_tracked", ()))
    return keys


def check_state_dict(sd, mode: str = "hubert", strict: bool = True) -> None:
    """ValueError naming the first missing key, wrong shape or unexpected key.  strict=False lets the BatchNorm counters be
    absent and ignores keys the network does not have."""
    want = manifest(mode)
    for key, shape in want:
        counter = key.endswith("num_batches_tracked")
        if key not in sd:
            if counter and not strict:
                continue
            raise ValueError(f"SyncNet_color({mode!r}) checkpoint lacks {key}")
        if not counter and tuple(sd[key].shape) != shape:
            raise ValueError(f"SyncNet_color({mode!r}) checkpoint: {key} has shape {tuple(sd[key].shape)}, the network has {shape}")
    if strict:
        names = {k for k, _ in want}
        for key in sd:
            if key not in names:
                raise ValueError(f"SyncNet_color({mode!r}) checkpoint has an unexpected key {key}")


def _f64(v) -> np.ndarray:
    return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float64)


def fold(sd, mode: str = "hubert", dtype=np.float32, strict: bool = True) -> Dict[str, np.ndarray]:
    """The plain convs of the eval-mode network: {"face.<i>.w" [cout, cin, k, k], "face.<i>.b" [cout], "audio.<i>..."}: BatchNorm
    folded in float64, w' = w g / sqrt(var + eps), b' = (b - mean) g / sqrt(var + eps) + beta, rounded once to `dtype`."""
    check_state_dict(sd, mode, strict)
    out: Dict[str, np.ndarray] = {}
    for p, *_ in blocks(mode):
        w, b = _f64(sd[f"{p}.conv_block.0.weight"]), _f64(sd[f"{p}.conv_block.0.bias"])
        gamma, beta, mean, var = (_f64(sd[f"{p}.conv_block.1.{n}"]) for n in ("weight", "bias", "running_mean", "running_var"))
        scale = gamma / np.sqrt(var + BN_EPS)
        out[f"{_short(p)}.w"] = (w * scale.reshape(-1, 1, 1, 1)).astype(dtype)
        out[f"{_short(p)}.b"] = ((b - mean) * scale + beta).astype(dtype)
    return out


def packed_tensors(sd, mode: str = "hubert", strict: bool = True) -> Dict[str, np.ndarray]:
    """The engine's named tensors (include/casync_hip.h, casync_sync_packed_*): w [cout][(ky, kx, cin)], face.0's
    [(ky, kx, cin)][cout]."""
    f = fold(sd, mode, strict=strict)
    out: Dict[str, np.ndarray] = {}
    for name, v in f.items():
        if name.endswith(".w"):
            v = v.transpose(2, 3, 1, 0).reshape(-1, v.shape[0]) if name == "face.0.w" else v.transpose(0, 2, 3, 1).reshape(v.shape[0], -1)
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def pack(sd, mode: str = "hubert", strict: bool = True) -> np.ndarray:
    """The flat float32 buffer casync_sync_load_weights_* takes."""
    return _lib.pack_named(packed_tensors(sd, mode, strict), _lib.sync_layout(mode))


def unpack(buf: np.ndarray, mode: str = "hubert") -> Dict[str, np.ndarray]:
    """Inverse of pack (flat shapes)."""
    return _lib.unpack_named(buf, _lib.sync_layout(mode))


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class SyncNetEngine(_PackedEngine):
    """SyncNet_color(mode).eval() on the HIP engine.  Inputs are float32 device tensors, contiguous: face [B,3,160,160] in
    [0,1] (BGR), audio [B,32,32,32] (hubert) or [B,256,16,32] (wenet).  precision "bf16" runs the blocks on bf16 activations
    and a bf16 image of the same packed buffer (include/casync_hip.h); inputs, embeddings and taps stay float32."""

    _destroy = "casync_sync_destroy"

    def __init__(self, packed: np.ndarray, mode: str = "hubert", device: str = "cuda:0", precision: str = "fp32"):
        if mode not in AUDIO_SHAPE:
            raise ValueError(f"SyncNet mode {mode!r} ('hubert' or 'wenet')")
        self._precision = check_precision(precision)
        self.mode, self.precision = mode, precision
        self._open(device, "casync_syncnet_create_ex", (_lib.AUDIO_MODES[mode], self._precision), "casync_sync_load_weights_host", packed)

    def workspace_bytes(self, batch: int) -> int:
        need = self._lib.casync_syncnet_workspace_bytes_ex(_lib.AUDIO_MODES[self.mode], self._precision, batch)
        if need <= 0:
            raise ValueError(f"SyncNet engine: batch {batch} (1..65536)")
        return need

    def _check(self, t: Optional[torch.Tensor], shape: Tuple[int, ...], what: str) -> int:
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or tuple(t.shape[1:]) != shape:
            got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"SyncNet engine ({self.mode}): {what} {got}, expected [B,{','.join(map(str, shape))}]")
        if t.dtype != torch.float32 or t.device != self.device:
            raise ValueError(f"SyncNet engine: {what} must be float32 on {self.device}, got {t.dtype} on {t.device}")
        if not t.is_contiguous():
            raise ValueError(f"SyncNet engine: {what} must be contiguous")
        return t.shape[0]

    def forward(self, face: torch.Tensor, audio: torch.Tensor, workspace: Optional[torch.Tensor] = None):
        """-> (audio_embedding, face_embedding), both [B,4608] on the device, valid on torch's current stream."""
        b = self._check(face, (3, FACE_HW, FACE_HW), "face_sequences")
        if self._check(audio, AUDIO_SHAPE[self.mode], "audio_sequences") != b:
            raise ValueError(f"SyncNet engine: {b} faces and {audio.shape[0]} audio windows")
        a_emb = torch.empty((b, EMBED_DIM), dtype=torch.float32, device=self.device)
        f_emb = torch.empty((b, EMBED_DIM), dtype=torch.float32, device=self.device)
        if b:
            ws = self._grow_workspace(self.workspace_bytes(b)) if workspace is None else workspace
            with torch.cuda.device(self.device):
                _lib.check(self._lib.casync_sync_forward(self._h, face.data_ptr(), audio.data_ptr(), b, a_emb.data_ptr(), f_emb.data_ptr(),
                                                         ws.data_ptr(), ws.numel() * ws.element_size(), _stream(self.device)),
                           "casync_sync_forward")
        return a_emb, f_emb

    def tap(self, stage, x: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The output of block `stage` (a name of STAGES or its index) in NCHW order; x is that encoder's input."""
        idx = STAGES.index(stage) if isinstance(stage, str) else int(stage)
        if not 0 <= idx < len(STAGES):
            raise ValueError(f"SyncNet engine: stage {stage!r}")
        is_face = STAGES[idx].startswith("face")
        b = self._check(x, (3, FACE_HW, FACE_HW) if is_face else AUDIO_SHAPE[self.mode], "face_sequences" if is_face else "audio_sequences")
        out = torch.empty((b,) + stage_shapes(self.mode)[idx], dtype=torch.float32, device=self.device)
        if b:
            ws = self._grow_workspace(self.workspace_bytes(b)) if workspace is None else workspace
            with torch.cuda.device(self.device):
                _lib.check(self._lib.casync_sync_forward_tap(self._h, x.data_ptr() if is_face else None, None if is_face else x.data_ptr(),
                                                             b, idx, out.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(),
                                                             _stream(self.device)), "casync_sync_forward_tap")
        return out

    __call__ = forward


def shift_similarity(face_emb: torch.Tensor, audio_emb: torch.Tensor, max_shift: int) -> torch.Tensor:
    """sim [2 S + 1, N] float32 on the device: sim[s + S, i] = cos(face_i, audio_(i+s)) in F.cosine_similarity's form (the dot
    product over max(|a| |b|, 1e-8)), 0 where i + s is outside [0, N) (casync_op_sync_curve)."""
    if face_emb.dim() != 2 or face_emb.shape != audio_emb.shape or face_emb.shape[0] < 1 or face_emb.shape[1] % 4:
        raise ValueError(f"shift_similarity: embeddings {tuple(face_emb.shape)} and {tuple(audio_emb.shape)} ([N,D] both, N >= 1, D % 4 == 0)")
    if face_emb.device.type != "cuda" or audio_emb.device != face_emb.device:
        raise RuntimeError("shift_similarity: the embeddings must be on one ROCm device (no CPU fallback)")
    if face_emb.dtype != torch.float32 or audio_emb.dtype != torch.float32:
        raise ValueError("shift_similarity: float32 embeddings")
    if not 0 <= int(max_shift) <= MAX_SHIFT:
        raise ValueError(f"shift_similarity: max_shift {max_shift} (0..{MAX_SHIFT})")
    f, a = face_emb.contiguous(), audio_emb.contiguous()
    n, d = f.shape
    sim = torch.empty((2 * int(max_shift) + 1, n), dtype=torch.float32, device=f.device)
    with torch.cuda.device(f.device):
        _lib.check(_lib.load().casync_op_sync_curve(f.data_ptr(), a.data_ptr(), n, d, int(max_shift), sim.data_ptr(), _stream(f.device)),
                   "casync_op_sync_curve")
    return sim


@dataclass
class OffsetCurve:
    """sim [2 S + 1, N] float32 and curve [2 S + 1] float64 on the device (curve[s + S] = the mean of sim[s + S] over its valid
    pairs, 0 where there is none), counts [2 S + 1] int64 on the host, best_shift the shift of the highest mean among those
    with a valid pair (the smallest |shift| first among equals)."""
    sim: torch.Tensor
    curve: torch.Tensor
    counts: torch.Tensor
    best_shift: int
    max_shift: int


def curve_of(sim: torch.Tensor) -> OffsetCurve:
    s2, n = sim.shape
    max_shift = (s2 - 1) // 2
    shifts = torch.arange(-max_shift, max_shift + 1)
    counts = (n - shifts.abs()).clamp_min(0)
    cd = counts.to(sim.device)
    curve = torch.where(cd > 0, sim.double().sum(1) / cd.clamp_min(1).double(), torch.zeros((), dtype=torch.float64, device=sim.device))
    c = curve.cpu()
    best, best_v = 0, None
    for i in sorted(range(s2), key=lambda i: (abs(int(shifts[i])), int(shifts[i]))):
        if int(counts[i]) > 0 and (best_v is None or float(c[i]) > best_v):
            best, best_v = int(shifts[i]), float(c[i])
    return OffsetCurve(sim, curve, counts, best, max_shift)


class SyncNetColor:
    """The reference's SyncNet_color(mode) in eval mode: load_state_dict takes its 217 keys, forward returns
    (audio_embedding, face_embedding).  precision "fp32" (the default) or "bf16": SyncNetEngine's."""

    def __init__(self, mode: str = "hubert", device: str = "cuda:0", state_dict=None, precision: str = "fp32"):
        if mode not in AUDIO_SHAPE:
            raise ValueError(f"SyncNet mode {mode!r} ('hubert' or 'wenet')")
        check_precision(precision)
        self.mode, self.precision = mode, precision
        self.device = torch.device(device)
        self._packed: Optional[np.ndarray] = None
        self._engine: Optional[SyncNetEngine] = None
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def load_state_dict(self, sd, strict: bool = True):
        self._packed = pack(sd, self.mode, strict)      # (checks the checkpoint before any device call)
        self._engine = None
        return self

    def eval(self):
        return self

    def to(self, device):
        device = torch.device(device)
        if device != self.device:
            self.device, self._engine = device, None
        return self

    @property
    def engine(self) -> SyncNetEngine:
        if self._packed is None:
            raise RuntimeError("SyncNetColor: no weights loaded (load_state_dict)")
        if self._engine is None:
            dev = self.device if self.device.index is not None else torch.device(self.device.type, 0)
            self._engine = SyncNetEngine(self._packed, self.mode, dev, self.precision)
        return self._engine

    def forward(self, face_sequences: torch.Tensor, audio_sequences: torch.Tensor):
        return self.engine.forward(face_sequences, audio_sequences)

    __call__ = forward

    def similarity(self, face: torch.Tensor, audio: torch.Tensor) -> torch.Tensor:
        """cosine_similarity(audio_embedding, face_embedding) of the B pairs -> [B] float32 on the device."""
        a, f = self.forward(face, audio)
        return shift_similarity(f, a, 0)[0]          # row 0 of the shift-0 curve

    def offset_curve(self, face: torch.Tensor, audio: torch.Tensor, max_shift: int) -> OffsetCurve:
        """The cosine between face i and audio i + s for s in [-max_shift, max_shift] over N consecutive frames."""
        a, f = self.forward(face, audio)
        return curve_of(shift_similarity(f, a, max_shift))

    def score_clip(self, faces: torch.Tensor, features: torch.Tensor, frame_indices, max_shift: int) -> OffsetCurve:
        """faces [N,3,160,160] (Model.forward's output as it is), features [T,2,1024] the clip's HuBERT features on the device,
        frame_indices the N frames' indices: the windows are frame_loop.audio_windows_device's."""
        if self.mode != "hubert":
            raise ValueError("score_clip builds HuBERT windows: mode 'hubert' only")
        from . import frame_loop
        return self.offset_curve(faces, frame_loop.audio_windows_device(features, frame_indices), max_shift)


SyncNet_color = SyncNetColor
