"""CPU restatement of transformers' HubertModel (hubert-large config, do_stable_layer_norm) for the tests -- a plain
helper module, like tests/wenet_ref.py.  It computes from the engine's named packed tensors
(``calipsync_amd.hubert.packed_tensors``), so it checks the packing as well; ``tests/golden/hubert_*.npz`` pin it
against the reference's own ``HubertExtractor.extract_features`` (tests/test_hubert.py).

Also here: the recipe weights of the fixtures (``recipe_state_dict``: the repo's counter-based generator, never
``torch.randn``), the fixture waveforms (``golden_wave``) and the cheap stub model of the chunking fixture.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from calipsync_amd import recipe

EPS = 1e-5
SEED = 4242
# gains (x 1/sqrt(fan_in)) of the recipe weights, chosen so that attention over ~1000 keys is neither uniform nor one-hot
# (the generator records the mean max-softmax probability per layer) and the output depends on the input
GAINS = {"conv": 1.0, "fp": 1.0, "q": 2.0, "k": 2.0, "v": 1.0, "o": 0.6, "ff1": 1.0, "ff2": 0.5}


def _t(a) -> torch.Tensor:
    return torch.as_tensor(np.asarray(a, dtype=np.float32))


def forward(P: Dict[str, np.ndarray], layers: int, wave: torch.Tensor, taps: Optional[dict] = None,
            n_layers: Optional[int] = None) -> torch.Tensor:
    """wave [B,S] fp32 -> last_hidden_state [B,T,1024].  taps (optional) receives 'conv' [B,T,512], 'layer0_in' and
    'after<n>' (hidden states after n layers, before the final LayerNorm)."""
    x = wave.float()[:, None, :]
    for i, (k, s) in enumerate(zip((10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2))):
        cin = 1 if i == 0 else 512
        w = _t(P[f"fe.conv{i}.w"]).reshape(512, k, cin).permute(0, 2, 1)
        x = F.conv1d(x, w, _t(P[f"fe.conv{i}.b"]), stride=s)
        x = F.layer_norm(x.transpose(1, 2), (512,), _t(P[f"fe.ln{i}.g"]), _t(P[f"fe.ln{i}.b"]), EPS).transpose(1, 2)
        x = F.gelu(x)
    conv = x.transpose(1, 2)
    if taps is not None:
        taps["conv"] = conv
    h = F.layer_norm(conv, (512,), _t(P["fp.ln.g"]), _t(P["fp.ln.b"]), EPS)
    h = F.linear(h, _t(P["fp.w"]).reshape(1024, 512), _t(P["fp.b"]))
    wp = _t(P["pos.w"]).reshape(16, 128, 64, 64).permute(0, 2, 3, 1).reshape(1024, 64, 128)
    pc = F.conv1d(h.transpose(1, 2), wp, _t(P["pos.b"]), padding=64, groups=16)[:, :, :-1]
    h = h + F.gelu(pc).transpose(1, 2)
    if taps is not None:
        taps["layer0_in"] = h
    B, T, _ = h.shape
    for l in range(layers if n_layers is None else n_layers):
        p = f"layer{l}"
        t = F.layer_norm(h, (1024,), _t(P[f"{p}.ln1.g"]), _t(P[f"{p}.ln1.b"]), EPS)
        qkv = F.linear(t, _t(P[f"{p}.qkv.w"]).reshape(3072, 1024), _t(P[f"{p}.qkv.b"]))
        q, k, v = (z.reshape(B, T, 16, 64).transpose(1, 2) for z in qkv.split(1024, dim=-1))
        a = torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v            # q carries the 1/8
        a = a.transpose(1, 2).reshape(B, T, 1024)
        h = h + F.linear(a, _t(P[f"{p}.o.w"]).reshape(1024, 1024), _t(P[f"{p}.o.b"]))
        t = F.layer_norm(h, (1024,), _t(P[f"{p}.ln2.g"]), _t(P[f"{p}.ln2.b"]), EPS)
        t = F.gelu(F.linear(t, _t(P[f"{p}.ff1.w"]).reshape(4096, 1024), _t(P[f"{p}.ff1.b"])))
        h = h + F.linear(t, _t(P[f"{p}.ff2.w"]).reshape(1024, 4096), _t(P[f"{p}.ff2.b"]))
    if taps is not None:
        taps[f"after{layers if n_layers is None else n_layers}"] = h
    if n_layers is not None and n_layers != layers:
        return h
    return F.layer_norm(h, (1024,), _t(P["enc.ln.g"]), _t(P["enc.ln.b"]), EPS)


def config(layers: int) -> dict:
    """config.json of the fixtures' models (hubert-large-ls960-ft with `layers` layers)."""
    return {
        "model_type": "hubert", "architectures": ["HubertForCTC"], "hidden_size": 1024, "num_hidden_layers": layers,
        "num_attention_heads": 16, "intermediate_size": 4096, "hidden_act": "gelu", "layer_norm_eps": 1e-5,
        "feat_extract_norm": "layer", "feat_extract_activation": "gelu", "conv_dim": [512] * 7,
        "conv_kernel": [10, 3, 3, 3, 3, 2, 2], "conv_stride": [5, 2, 2, 2, 2, 2, 2], "conv_bias": True,
        "do_stable_layer_norm": True, "feat_proj_layer_norm": True, "num_conv_pos_embeddings": 128,
        "num_conv_pos_embedding_groups": 16, "vocab_size": 32, "hidden_dropout": 0.0, "attention_dropout": 0.0,
        "activation_dropout": 0.0, "feat_proj_dropout": 0.0, "layerdrop": 0.0, "apply_spec_augment": False,
    }


def recipe_state_dict(layers: int, weight_norm: str = "weight_g") -> Dict[str, torch.Tensor]:
    """HubertModel state dict (no prefix) from recipe.normal01 / uniform01.  weight_norm: the pos-conv spelling,
    "weight_g" (weight_g / weight_v) or "parametrizations" (parametrizations.weight.original0 / original1)."""
    sd: Dict[str, torch.Tensor] = {}

    def normal(key, shape, std, mean=0.0):
        n = int(np.prod(shape))
        sd[key] = torch.from_numpy((mean + std * recipe.normal01(SEED, recipe._stream(key), n)).reshape(shape).astype(np.float32))

    for i, k in enumerate((10, 3, 3, 3, 3, 2, 2)):
        cin = 1 if i == 0 else 512
        p = f"feature_extractor.conv_layers.{i}"
        normal(f"{p}.conv.weight", (512, cin, k), GAINS["conv"] / np.sqrt(cin * k))
        normal(f"{p}.conv.bias", (512,), 0.1)
        normal(f"{p}.layer_norm.weight", (512,), 0.1, 1.0)
        normal(f"{p}.layer_norm.bias", (512,), 0.1)
    normal("feature_projection.layer_norm.weight", (512,), 0.1, 1.0)
    normal("feature_projection.layer_norm.bias", (512,), 0.1)
    normal("feature_projection.projection.weight", (1024, 512), GAINS["fp"] / np.sqrt(512))
    normal("feature_projection.projection.bias", (1024,), 0.05)
    p = "encoder.pos_conv_embed.conv"
    g = (0.8 + 0.4 * recipe.uniform01(SEED, recipe._stream(p + ".g"), 128)).reshape(1, 1, 128).astype(np.float32)
    normal(p + ".v", (1024, 64, 128), 1.0)
    v = sd.pop(p + ".v")
    if weight_norm == "weight_g":
        sd[p + ".weight_g"], sd[p + ".weight_v"] = torch.from_numpy(g), v
    else:
        sd[p + ".parametrizations.weight.original0"], sd[p + ".parametrizations.weight.original1"] = torch.from_numpy(g), v
    normal(p + ".bias", (1024,), 0.05)
    for l in range(layers):
        p, a = f"encoder.layers.{l}", f"encoder.layers.{l}.attention"
        for n in ("q", "k", "v"):
            normal(f"{a}.{n}_proj.weight", (1024, 1024), GAINS[n] / 32.0)
            normal(f"{a}.{n}_proj.bias", (1024,), 0.05)
        normal(f"{a}.out_proj.weight", (1024, 1024), GAINS["o"] / 32.0)
        normal(f"{a}.out_proj.bias", (1024,), 0.05)
        for n in ("layer_norm", "final_layer_norm"):
            normal(f"{p}.{n}.weight", (1024,), 0.1, 1.0)
            normal(f"{p}.{n}.bias", (1024,), 0.1)
        normal(f"{p}.feed_forward.intermediate_dense.weight", (4096, 1024), GAINS["ff1"] / 32.0)
        normal(f"{p}.feed_forward.intermediate_dense.bias", (4096,), 0.05)
        normal(f"{p}.feed_forward.output_dense.weight", (1024, 4096), GAINS["ff2"] / 64.0)
        normal(f"{p}.feed_forward.output_dense.bias", (1024,), 0.05)
    normal("encoder.layer_norm.weight", (1024,), 0.1, 1.0)
    normal("encoder.layer_norm.bias", (1024,), 0.1)
    return sd


def golden_wave(n: int, seed: int) -> np.ndarray:
    """A speech-like float64 test waveform in [-1, 1): a few drifting tones under an envelope, plus noise."""
    t = np.arange(n, dtype=np.float64) / 16000.0
    u = recipe.uniform01(seed, 1, 8)
    x = np.zeros(n)
    for j in range(4):
        f0 = 120.0 + 600.0 * u[j]
        x += np.sin(2 * np.pi * (f0 * t + 30.0 * u[4 + j] * np.sin(2 * np.pi * 0.7 * t)))
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 3.1 * t + u[0]) ** 2
    x = 0.2 * env * x + 0.05 * recipe.normal01(seed, 2, n)
    return np.clip(x, -1.0, 1.0 - 2 ** -15)


def stub_encode(chunk: torch.Tensor) -> torch.Tensor:
    """A cheap deterministic stand-in for HubertModel(chunk).last_hidden_state[0] ([1, n] -> [T(n), 1024]): token t
    carries sums of its 400-sample window, so every sample position and the chunk seams show in the output."""
    x = chunk[0].double()
    n = x.shape[0]
    t = (n - 400) // 320 + 1
    idx = torch.arange(t)[:, None] * 320 + torch.arange(400)[None, :]
    win = x[idx]                                              # [T, 400]
    feats = torch.stack([win.sum(1), (win * torch.linspace(-1, 1, 400, dtype=torch.float64)).sum(1), win[:, 0], win[:, -1]], 1)
    j = torch.arange(1024, dtype=torch.float64)
    out = feats[:, j.long() % 4] * (1.0 + j / 1024.0) + torch.arange(t, dtype=torch.float64)[:, None] * 1e-3
    return out.float()
