"""HuBERT-large feature extraction on the HIP engine: the drop-in for the reference's ``HubertExtractor``
(image_infer_v1/utils/hubert_extractor.py:7-65) without transformers.

* ``load_checkpoint(dir)`` reads a HuBERT checkpoint directory (``config.json``, ``preprocessor_config.json``,
  ``pytorch_model.bin`` or ``model.safetensors``) and checks that the config is the one the engine computes.
* ``pack(state_dict, layers)`` folds it into the engine's packed buffer (``casync_hubert_packed_*``): weight norm
  folded in float64, q/k/v fused with the 1/8 query scale folded in, conv weights channels-last.
* ``HubertEngine`` runs ``HubertModel(...).last_hidden_state`` for a batch of equal-length waveforms.
* ``HubertExtractor`` keeps the reference's ``extract_features`` / ``extract_from_file``; its normalisation and
  chunking (``chunked_features``) restate the reference exactly and take any encoder callable.
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess
import tempfile
import wave as _wave
from typing import Callable, Dict, List, Tuple

import numpy as np
import torch

from .engine_base import _PackedEngine

# the configuration the engine computes (transformers HubertConfig of hubert-large-ls960-ft); num_hidden_layers is free
REQUIRED_CONFIG = {
    "hidden_size": 1024,
    "num_attention_heads": 16,
    "intermediate_size": 4096,
    "hidden_act": "gelu",
    "layer_norm_eps": 1e-5,
    "feat_extract_norm": "layer",
    "feat_extract_activation": "gelu",
    "conv_dim": [512] * 7,
    "conv_kernel": [10, 3, 3, 3, 3, 2, 2],
    "conv_stride": [5, 2, 2, 2, 2, 2, 2],
    "conv_bias": True,
    "do_stable_layer_norm": True,
    "feat_proj_layer_norm": True,
    "num_conv_pos_embeddings": 128,
    "num_conv_pos_embedding_groups": 16,
}
KERNEL, STRIDE = 400, 320             # receptive field and hop of one token, in samples
CLIP = STRIDE * 1000                  # samples per chunk step (hubert_extractor.py:29)
CHUNK = CLIP - STRIDE + KERNEL        # samples of one full chunk: 320080 -> 1000 tokens


def check_config(cfg: dict) -> int:
    """-> num_hidden_layers; ValueError naming the first field that differs from what the engine computes."""
    for key, want in REQUIRED_CONFIG.items():
        got = cfg.get(key, want if key == "feat_proj_layer_norm" else None)   # (older configs omit it: True then)
        ok = (abs(float(got) - want) <= 1e-12 * abs(want)) if isinstance(want, float) and isinstance(got, (int, float)) else got == want
        if not ok:
            raise ValueError(f"HuBERT config field {key!r} is {got!r}; the engine computes {want!r}")
    layers = cfg.get("num_hidden_layers")
    if not isinstance(layers, int) or not 1 <= layers <= 48:
        raise ValueError(f"HuBERT config field 'num_hidden_layers' is {layers!r} (1..48)")
    if cfg.get("conv_pos_batch_norm", False):
        raise ValueError("HuBERT config field 'conv_pos_batch_norm' is True; the engine computes False")
    return layers


def _read_state_dict(path: str) -> Dict[str, torch.Tensor]:
    st = os.path.join(path, "model.safetensors")
    bn = os.path.join(path, "pytorch_model.bin")
    if os.path.exists(st):
        try:
            from safetensors.torch import load_file
        except ImportError:
            load_file = None
        if load_file is not None:
            return dict(load_file(st))
        if not os.path.exists(bn):
            raise RuntimeError(f"{st} needs the safetensors package, and there is no pytorch_model.bin beside it")
    if os.path.exists(bn):
        return dict(torch.load(bn, map_location="cpu", weights_only=True))
    raise FileNotFoundError(f"no model.safetensors or pytorch_model.bin in {path}")


def load_checkpoint(path: str) -> Tuple[dict, Dict[str, torch.Tensor], bool]:
    """-> (config, state dict without the ``hubert.`` prefix and the CTC head, do_normalize)."""
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    check_config(cfg)
    do_normalize = True
    pp = os.path.join(path, "preprocessor_config.json")
    if os.path.exists(pp):
        with open(pp) as f:
            do_normalize = bool(json.load(f).get("do_normalize", True))
    sd = {}
    for k, v in _read_state_dict(path).items():
        k = k[len("hubert."):] if k.startswith("hubert.") else k
        if k.startswith("lm_head.") or k == "masked_spec_embed":
            continue
        sd[k] = v
    return cfg, sd, do_normalize


def _weight_norm(sd: Dict[str, torch.Tensor], prefix: str) -> torch.Tensor:
    """pos_conv weight with weight norm over dim 2, folded in float64: W[:,:,k] = g[k] v[:,:,k] / ||v[:,:,k]||."""
    for gk, vk in (("weight_g", "weight_v"), ("parametrizations.weight.original0", "parametrizations.weight.original1")):
        if f"{prefix}.{gk}" in sd and f"{prefix}.{vk}" in sd:
            g = sd[f"{prefix}.{gk}"].double()
            v = sd[f"{prefix}.{vk}"].double()
            return g * v / v.norm(dim=(0, 1), keepdim=True)
    if f"{prefix}.weight" in sd:
        return sd[f"{prefix}.weight"].double()
    raise KeyError(f"{prefix}: no weight_g/weight_v or parametrizations.weight.original0/1")


def packed_tensors(sd: Dict[str, torch.Tensor], layers: int) -> Dict[str, np.ndarray]:
    """The engine's named tensors (include/casync_hip.h, casync_hubert_packed_*) from a HubertModel state dict."""
    def f(k):
        if k not in sd:
            raise KeyError(f"HuBERT checkpoint lacks {k}")
        return sd[k].detach().double()

    out: Dict[str, np.ndarray] = {}
    for i in range(7):
        p = f"feature_extractor.conv_layers.{i}"
        w = f(f"{p}.conv.weight")                       # [512, cin, k]
        out[f"fe.conv{i}.w"] = w.permute(0, 2, 1).reshape(512, -1).numpy()   # [cout][tap][cin]
        out[f"fe.conv{i}.b"] = f(f"{p}.conv.bias").numpy()
        out[f"fe.ln{i}.g"] = f(f"{p}.layer_norm.weight").numpy()
        out[f"fe.ln{i}.b"] = f(f"{p}.layer_norm.bias").numpy()
    out["fp.ln.g"] = f("feature_projection.layer_norm.weight").numpy()
    out["fp.ln.b"] = f("feature_projection.layer_norm.bias").numpy()
    out["fp.w"] = f("feature_projection.projection.weight").numpy()
    out["fp.b"] = f("feature_projection.projection.bias").numpy()
    wp = _weight_norm(sd, "encoder.pos_conv_embed.conv")            # [1024 out, 64 in, 128 taps]
    out["pos.w"] = wp.reshape(16, 64, 64, 128).permute(0, 3, 1, 2).numpy()   # [group][tap][n][c]
    out["pos.b"] = f("encoder.pos_conv_embed.conv.bias").numpy()
    scale = 64 ** -0.5                                             # exact: a power of two
    for l in range(layers):
        p, a = f"encoder.layers.{l}", f"encoder.layers.{l}.attention"
        out[f"layer{l}.ln1.g"] = f(f"{p}.layer_norm.weight").numpy()
        out[f"layer{l}.ln1.b"] = f(f"{p}.layer_norm.bias").numpy()
        out[f"layer{l}.qkv.w"] = torch.cat([f(f"{a}.q_proj.weight") * scale, f(f"{a}.k_proj.weight"), f(f"{a}.v_proj.weight")]).numpy()
        out[f"layer{l}.qkv.b"] = torch.cat([f(f"{a}.q_proj.bias") * scale, f(f"{a}.k_proj.bias"), f(f"{a}.v_proj.bias")]).numpy()
        out[f"layer{l}.o.w"] = f(f"{a}.out_proj.weight").numpy()
        out[f"layer{l}.o.b"] = f(f"{a}.out_proj.bias").numpy()
        out[f"layer{l}.ln2.g"] = f(f"{p}.final_layer_norm.weight").numpy()
        out[f"layer{l}.ln2.b"] = f(f"{p}.final_layer_norm.bias").numpy()
        out[f"layer{l}.ff1.w"] = f(f"{p}.feed_forward.intermediate_dense.weight").numpy()
        out[f"layer{l}.ff1.b"] = f(f"{p}.feed_forward.intermediate_dense.bias").numpy()
        out[f"layer{l}.ff2.w"] = f(f"{p}.feed_forward.output_dense.weight").numpy()
        out[f"layer{l}.ff2.b"] = f(f"{p}.feed_forward.output_dense.bias").numpy()
    out["enc.ln.g"] = f("encoder.layer_norm.weight").numpy()
    out["enc.ln.b"] = f("encoder.layer_norm.bias").numpy()
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def pack(sd: Dict[str, torch.Tensor], layers: int) -> np.ndarray:
    """The flat float32 buffer casync_hubert_load_weights_* takes."""
    from . import _lib
    return _lib.pack_named(packed_tensors(sd, layers), _lib.hubert_layout(layers))


def unpack(buf: np.ndarray, layers: int) -> Dict[str, np.ndarray]:
    """Inverse of pack (flat shapes)."""
    from . import _lib
    return _lib.unpack_named(buf, _lib.hubert_layout(layers))


def tokens(samples: int) -> int:
    """Tokens of a waveform of `samples` samples (0 below 400)."""
    t = samples
    for k, s in zip(REQUIRED_CONFIG["conv_kernel"], REQUIRED_CONFIG["conv_stride"]):
        t = (t - k) // s + 1 if t >= k else 0
    return t


PRECISIONS = {"fp32": 0, "bf16": 1}   # -> the dtype of casync_hubert_create_ex


def check_precision(precision: str) -> int:
    """-> engine dtype; ValueError for anything but "fp32" / "bf16" (before any device call)."""
    if precision not in PRECISIONS:
        raise ValueError(f"HuBERT precision {precision!r}; the engine has {sorted(PRECISIONS)}")
    return PRECISIONS[precision]


class HubertEngine(_PackedEngine):
    """HubertModel(...).last_hidden_state on the HIP engine: forward(wave [B,S] on the device) -> [B,T,1024], fp32 in and
    out.  precision "bf16" runs the GEMMs, the attention and the activations between them in bf16 (fp32 sums, fp32 residual
    stream: DESIGN section 8b); "fp32" is the default."""

    _destroy = "casync_hubert_destroy"

    def __init__(self, sd: Dict[str, torch.Tensor], layers: int, device: str = "cuda:0", precision: str = "fp32"):
        dtype = check_precision(precision)
        self.layers = layers
        self.precision = precision
        self._create(device, "casync_hubert_create_ex", layers, dtype)
        self._load_host("casync_hubert_load_weights_host", pack(sd, layers))

    def _workspace(self, batch: int, samples: int) -> torch.Tensor:
        need = self._lib.casync_hubert_workspace_bytes_h(self._h, batch, samples)
        if need <= 0:
            raise ValueError(f"HuBERT engine: {samples} samples give no token (at least {KERNEL} are needed)")
        return self._grow_workspace(need)

    def forward(self, wave: torch.Tensor, stage: int = 0, n_layers: int = 0) -> torch.Tensor:
        """wave [B,S] fp32 (normalised) -> last_hidden_state [B,T,1024]; stage 1/2/3 = debug taps (casync_hubert_forward_tap)."""
        from . import _lib
        wave = wave.to(self.device, torch.float32).contiguous()
        if wave.dim() == 1:
            wave = wave[None]
        b, s = wave.shape
        t = tokens(s)
        ws = self._workspace(b, s)
        out = torch.empty(b, t, 512 if stage == 1 else 1024, dtype=torch.float32, device=self.device)
        strm = torch.cuda.current_stream(self.device).cuda_stream
        if stage == 0:
            st = self._lib.casync_hubert_forward(self._h, wave.data_ptr(), b, s, out.data_ptr(), ws.data_ptr(), ws.numel() * 4, strm)
        else:
            st = self._lib.casync_hubert_forward_tap(self._h, wave.data_ptr(), b, s, stage, n_layers, out.data_ptr(), ws.data_ptr(),
                                                     ws.numel() * 4, strm)
        _lib.check(st, "casync_hubert_forward")
        return out

    __call__ = forward


def normalize(speech: np.ndarray, do_normalize: bool = True) -> np.ndarray:
    """Wav2Vec2FeatureExtractor(do_normalize): float32, then (x - mean) / sqrt(var + 1e-7) over the utterance."""
    x = np.asarray(speech)
    if x.dtype == np.float64:
        x = x.astype(np.float32)
    elif x.dtype != np.float32:
        x = np.asarray(x, dtype=np.float32)
    if do_normalize:
        x = (x - x.mean()) / np.sqrt(x.var() + 1e-7)
    return x


def chunked_features(input_values: torch.Tensor, encode: Callable[[List[torch.Tensor]], List[torch.Tensor]],
                     keep_device: bool = False) -> torch.Tensor:
    """The reference's chunking (hubert_extractor.py:27-58) over a [1, N] tensor; keep_device leaves the features where
    ``encode`` made them (the same pad, trim and even length, the same bits) instead of downloading them.  ``encode(chunks)`` gets the chunk
    tensors ([1, n_i]) in order and returns one [T_i, 1024] tensor per chunk; it is called with the full-length chunks
    (320080 samples) of the clip first, then once more with the rest (a cut-short last chunk, the tail), so an engine
    can run each call as one batched forward."""
    n = input_values.shape[1]
    num_iter = n // CLIP
    expected_t = (n - (KERNEL - STRIDE)) // STRIDE
    chunks = [input_values[:, CLIP * i:CLIP * i + CHUNK] for i in range(num_iter)]
    if num_iter == 0 or input_values[:, CLIP * num_iter:].shape[1] >= KERNEL:
        remaining = input_values[:, CLIP * num_iter:]
        if remaining.shape[1] >= KERNEL:
            chunks.append(remaining)
    full = [c for c in chunks if c.shape[1] == CHUNK]
    rest = [c for c in chunks if c.shape[1] != CHUNK]
    feats = (list(encode(full)) if full else []) + (list(encode(rest)) if rest else [])
    # (full chunks always precede the rest: only the last full-step chunk can be cut short, and the tail follows it)
    features = torch.cat(feats, dim=0)            # raises on an empty list, as the reference does
    if not keep_device:
        features = features.cpu()
    if features.shape[0] < expected_t:
        features = torch.nn.functional.pad(features, (0, 0, 0, expected_t - features.shape[0]))
    else:
        features = features[:expected_t]
    if features.shape[0] % 2 == 1:
        features = features[:features.shape[0] - 1]
    return features.reshape(-1, 2, 1024)


def read_wav(path: str) -> np.ndarray:
    """16 kHz PCM WAV -> float64 samples scaled as soundfile scales them (int / 2^(bits-1)); [N] mono, [N, C] otherwise."""
    with _wave.open(path, "rb") as w:
        if w.getcomptype() != "NONE":
            raise ValueError(f"{path}: compressed WAV ({w.getcomptype()}); ffmpeg is needed to read it")
        ch, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    if rate != 16000:
        raise ValueError(f"{path}: {rate} Hz; resampling to 16 kHz needs ffmpeg")
    if width == 1:
        x = (np.frombuffer(raw, np.uint8).astype(np.float64) - 128.0) / 128.0
    elif width == 2:
        x = np.frombuffer(raw, "<i2").astype(np.float64) / 32768.0
    elif width == 3:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.float64) / float(1 << 23)
    elif width == 4:
        x = np.frombuffer(raw, "<i4").astype(np.float64) / float(1 << 31)
    else:
        raise ValueError(f"{path}: {8 * width}-bit samples")
    return x if ch == 1 else x.reshape(-1, ch)


def load_audio_16k(path: str) -> np.ndarray:
    """The reference's convert_to_16k + soundfile.read: ``ffmpeg -i in -ar 16000 -ac 1`` where ffmpeg exists, else a
    16 kHz PCM WAV read with the standard library."""
    if shutil.which("ffmpeg"):
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "audio_16k.wav")
            res = subprocess.run(["ffmpeg", "-i", path, "-ar", "16000", "-ac", "1", "-y", out, "-loglevel", "error"],
                                 capture_output=True, text=True)
            if res.returncode != 0:
                raise RuntimeError(f"ffmpeg could not convert {path}: {res.stderr.strip()}")
            return read_wav(out)
    try:
        return read_wav(path)
    except (_wave.Error, EOFError) as exc:
        raise ValueError(f"{path} is not a PCM WAV file ({exc}); ffmpeg is needed to read it") from exc


class HubertExtractor:
    """The reference's HubertExtractor(hubert_path, device) on the HIP engine.

    ``frontend`` chooses what stands between an audio file and the engine.  "reference" (the default) is the reference's own:
    ``ffmpeg -ar 16000 -ac 1`` where ffmpeg exists, else a 16 kHz WAV, normalised on the host.  "device" reads a PCM WAV of any
    rate with the standard library and decodes, downmixes (``mono``: "mean" or "first"), resamples and normalises it on the
    device (calipsync_amd/audio.py): it never looks for ffmpeg, and its resampler is scipy's polyphase filter, not ffmpeg's."""

    def __init__(self, hubert_path: str, device: str = "cuda:0", precision: str = "fp32", frontend: str = "reference",
                 mono: str = "mean"):
        from . import audio
        check_precision(precision)
        self.frontend = audio.check_frontend(frontend)     # ValueErrors before anything touches the device
        audio.check_mono(mono)
        self.mono = mono
        self.device = device
        cfg, sd, self.do_normalize = load_checkpoint(hubert_path)
        self.model = HubertEngine(sd, cfg["num_hidden_layers"], device, precision)

    def _encode(self, chunks: List[torch.Tensor]) -> List[torch.Tensor]:
        if len({c.shape[1] for c in chunks}) == 1:
            out = self.model(torch.cat(chunks, dim=0))
            return [out[i] for i in range(len(chunks))]
        return [self.model(c)[0] for c in chunks]

    @torch.no_grad()
    def extract_features(self, speech) -> torch.Tensor:
        speech = np.asarray(speech)
        if speech.ndim == 2:
            speech = speech[:, 0]
        input_values = torch.from_numpy(normalize(speech, self.do_normalize))[None]
        return chunked_features(input_values, self._encode)

    @torch.no_grad()
    def extract_features_device(self, audio_path: str) -> torch.Tensor:
        """extract_from_file of the "device" front end without the download: the [T/2,2,1024] features as a tensor on the
        device.  ValueError for an extractor of the "reference" front end, whose waveform is made on the host."""
        if self.frontend != "device":
            raise ValueError('extract_features_device needs HubertExtractor(frontend="device")')
        from . import audio
        pcm, rate, width = audio.read_pcm_wav(audio_path)
        wave16k, normalised = audio.frontend_device(pcm, rate, width, self.mono, self.device)
        input_values = (normalised if self.do_normalize else wave16k)[None]
        return chunked_features(input_values, self._encode, keep_device=True)

    def extract_from_file(self, audio_path: str) -> np.ndarray:
        if self.frontend == "device":
            return self.extract_features_device(audio_path).cpu().numpy()
        return self.extract_features(load_audio_16k(audio_path)).detach().numpy()

    __call__ = extract_from_file
