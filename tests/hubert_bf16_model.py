"""CPU model of the bf16 HuBERT engine's numerics contract: tests/hubert_ref.forward with a bf16 round
at every point where the engine stores bf16.  Sums are fp32 (torch's), so this pins WHERE the engine rounds, not the order
it adds in -- two summation orders of this same contract already differ by most of its distance to fp32 (DESIGN), which is
why the GPU engine is held to the reference's fixtures and only compared with this model, never barred against it.

    conv0 + LayerNorm + GELU         fp32 arithmetic, output rounded
    conv1..6                         weights and input bf16, output rounded, LayerNorm + GELU in fp32, output rounded
    feature-projection LayerNorm     bf16 in, fp32 out; projection and positional conv fp32
    residual stream h                fp32
    LN1 / LN2                        read fp32 h, output rounded
    q|k|v, out-proj, FF1, FF2        bf16 weights and input, bias added in fp32, output rounded
    GELU of FF1                      fp32 on the rounded FF1 output, rounded again
    attention                        scores from the bf16 q, k in fp32; exp(s - max) summed in fp32, rounded to bf16 for P V;
                                     divided by the fp32 sum, output rounded
    out-proj / FF2 result            a rounded delta, added to h in fp32
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5


def r(x: torch.Tensor) -> torch.Tensor:
    """round to bf16 (nearest even), back in fp32"""
    return x.bfloat16().float()


def _t(a) -> torch.Tensor:
    return torch.as_tensor(np.asarray(a, dtype=np.float32))


def forward(P: Dict[str, np.ndarray], layers: int, wave: torch.Tensor, taps: Optional[dict] = None,
            n_layers: Optional[int] = None) -> torch.Tensor:
    """Same signature and taps as hubert_ref.forward ('conv', 'layer0_in', 'after<n>')."""
    x = wave.float()[:, None, :]
    for i, (k, s) in enumerate(zip((10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2))):
        cin = 1 if i == 0 else 512
        w = _t(P[f"fe.conv{i}.w"]).reshape(512, k, cin).permute(0, 2, 1)
        if i > 0:
            w = r(w)
        x = F.conv1d(x, w, _t(P[f"fe.conv{i}.b"]), stride=s)
        if i > 0:
            x = r(x)
        x = F.layer_norm(x.transpose(1, 2), (512,), _t(P[f"fe.ln{i}.g"]), _t(P[f"fe.ln{i}.b"]), EPS).transpose(1, 2)
        x = r(F.gelu(x))
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
        t = r(F.layer_norm(h, (1024,), _t(P[f"{p}.ln1.g"]), _t(P[f"{p}.ln1.b"]), EPS))
        qkv = r(F.linear(t, r(_t(P[f"{p}.qkv.w"]).reshape(3072, 1024)), _t(P[f"{p}.qkv.b"])))
        q, k, v = (z.reshape(B, T, 16, 64).transpose(1, 2) for z in qkv.split(1024, dim=-1))
        s_ = q @ k.transpose(-1, -2)                                       # q carries the 1/8
        e = torch.exp(s_ - s_.max(-1, keepdim=True).values)
        a = (r(e) @ v) / e.sum(-1, keepdim=True)
        a = r(a.transpose(1, 2).reshape(B, T, 1024))
        h = h + r(F.linear(a, r(_t(P[f"{p}.o.w"]).reshape(1024, 1024)), _t(P[f"{p}.o.b"])))
        t = r(F.layer_norm(h, (1024,), _t(P[f"{p}.ln2.g"]), _t(P[f"{p}.ln2.b"]), EPS))
        t = r(F.gelu(r(F.linear(t, r(_t(P[f"{p}.ff1.w"]).reshape(4096, 1024)), _t(P[f"{p}.ff1.b"])))))
        h = h + r(F.linear(t, r(_t(P[f"{p}.ff2.w"]).reshape(1024, 4096)), _t(P[f"{p}.ff2.b"])))
    if taps is not None:
        taps[f"after{layers if n_layers is None else n_layers}"] = h
    if n_layers is not None and n_layers != layers:
        return h
    return F.layer_norm(h, (1024,), _t(P["enc.ln.g"]), _t(P["enc.ln.b"]), EPS)
