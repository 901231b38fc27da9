"""Our own restatement of the folded SyncNet_color graph (reference module/syncnet.py:155-246 with every conv + BatchNorm as
one conv + bias) with torch.nn.functional, dtype-generic; imports nothing of the reference.  tests/test_syncnet.py pins it,
together with syncnet.fold, against the reference's own float64 run."""
import torch
import torch.nn.functional as F

from calipsync_amd import syncnet


def embed(t):
    """[B,512,3,3] -> [B,4608]: view(B, -1), x / max(|x|_2, 1e-12), LeakyReLU(0.01)"""
    v = t.reshape(t.shape[0], -1)
    v = v / v.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return F.leaky_relu(v, 0.01)


def forward(folded, face, audio, mode="hubert"):
    """folded: syncnet.fold(sd, mode, dtype) (numpy); face [B,3,160,160], audio [B,...] tensors (their dtype is the arithmetic's).
    -> (audio_embedding, face_embedding, {stage name: NCHW tensor} for the 31 names of syncnet.STAGES)"""
    f = {k: torch.as_tensor(v).to(dtype=face.dtype) for k, v in folded.items()}
    stages = {}
    t = None
    for p, k, cin, cout, stride, pad, res in syncnet.blocks(mode):
        name = p.replace("_encoder", "")
        if p.endswith(".0"):
            t = face if name.startswith("face") else audio
        y = F.conv2d(t, f[f"{name}.w"], f[f"{name}.b"], stride=stride, padding=pad)
        t = F.relu(y + t if res else y)
        stages[name] = t
    return embed(stages["audio.13"]), embed(stages["face.16"]), stages


def cosine(a, b):
    """F.cosine_similarity's form as the engine states it: the dot product over max(|a| |b|, 1e-8)"""
    return (a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1)).clamp_min(1e-8)


def shift_curve(face_emb, audio_emb, max_shift):
    """sim [2 S + 1, N]: sim[s + S, i] = cosine(face_i, audio_(i+s)), 0 where i + s is outside [0, N)"""
    n = face_emb.shape[0]
    sim = torch.zeros(2 * max_shift + 1, n, dtype=face_emb.dtype)
    for s in range(-max_shift, max_shift + 1):
        lo, hi = max(0, -s), min(n, n - s)
        if hi > lo:
            sim[s + max_shift, lo:hi] = cosine(face_emb[lo:hi], audio_emb[lo + s:hi + s])
    return sim
