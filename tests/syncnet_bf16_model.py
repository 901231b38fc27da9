"""The equal-contract model of the bf16 SyncNet_color handle (include/casync_hip.h, "SyncNet_color, bf16 precision"): torch on
the CPU, the folded float32 weights of syncnet.fold and exactly the roundings the handle makes, every sum in float64 (the
handle's fp32 accumulation is the only thing it does not restate).  Imports nothing of the reference.

  * face.0: float32 weights on the float32 input, + bias, ReLU, one rounding to bf16;
  * the audio window: one rounding to bf16;
  * every other block: bf16 activations and bf16-rounded weights, + the float32 bias, + the residual (bf16) before the ReLU,
    one rounding to bf16 -- but the last block of each encoder (face.16, audio.13) keeps float32;
  * the embedding from that float32 tensor as tests/syncnet_ref.py states it.
"""
import torch
import torch.nn.functional as F

import syncnet_ref
from calipsync_amd import syncnet

LAST = ("face.16", "audio.13")


def _bf16(t):
    """float64 -> the bf16 value nearest to its float32 rounding, as float64"""
    return t.float().bfloat16().double()


def forward(folded, face, audio, mode="hubert"):
    """folded: syncnet.fold(sd, mode) (float32 numpy); face, audio float32 tensors.
    -> (audio_embedding, face_embedding, {stage name: float32 NCHW tensor}) as SyncNetEngine(precision="bf16") returns them"""
    f = {k: torch.as_tensor(v).float() for k, v in folded.items()}
    stages = {}
    t = None
    for p, k, cin, cout, stride, pad, res in syncnet.blocks(mode):
        name = p.replace("_encoder", "")
        w, b = f[f"{name}.w"], f[f"{name}.b"].double()
        if name == "face.0":
            t = face.double()
            w = w.double()
        else:
            if name == "audio.0":
                t = _bf16(audio.double())
            w = w.bfloat16().double()
        y = F.conv2d(t, w, b, stride=stride, padding=pad)
        y = F.relu(y + t if res else y)
        t = y.float().double() if name in LAST else _bf16(y)
        stages[name] = t.float()
    a_emb = syncnet_ref.embed(stages["audio.13"].double()).float()
    f_emb = syncnet_ref.embed(stages["face.16"].double()).float()
    return a_emb, f_emb, stages
