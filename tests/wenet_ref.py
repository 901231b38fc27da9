"""CPU forward of the reference's ``Model(6, 'wenet')`` for the tests -- a plain helper module, not a conftest.

Composed from the public building blocks of ``oracle/unet_oracle.py`` (inverted residual, BN, MLP fusion,
attention block, Up block) with the one part the oracle does not have: ``AudioConvWenet`` (reference
module/unet.py:109-144) -- two residual blocks on 16x32 frames, conv3 with stride (1, 2) + BN + ReLU,
conv4, conv5 + BN + ReLU, conv6, conv7, and no bn7 / relu7.  ``tests/golden/unet_wenet_b2.npz`` pins it
against the reference itself (``tests/test_wenet.py``).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle.unet_oracle import _act, _bn, attention_block, double_conv, inverted_residual, mlp_fusion, up_block


def audio_encoder_wenet(sd, a: torch.Tensor, taps: Optional[dict] = None) -> torch.Tensor:
    """AudioConvWenet.forward: [B,256,16,32] -> [B,512,10,10]."""
    p = "audio_model"
    a = inverted_residual(sd, f"{p}.conv1", a, 1, True)
    if taps is not None:
        taps["audio_conv1"] = a
    a = inverted_residual(sd, f"{p}.conv2", a, 1, True)
    if taps is not None:
        taps["audio_conv2"] = a
    a = F.relu(_bn(sd, f"{p}.bn3", F.conv2d(a, sd[f"{p}.conv3.weight"], sd[f"{p}.conv3.bias"], (1, 2), 1)))
    if taps is not None:
        taps["audio_conv3"] = a
    a = inverted_residual(sd, f"{p}.conv4", a, 1, True)
    if taps is not None:
        taps["audio_conv4"] = a
    a = F.relu(_bn(sd, f"{p}.bn5", F.conv2d(a, sd[f"{p}.conv5.weight"], sd[f"{p}.conv5.bias"], 2, 3)))
    if taps is not None:
        taps["audio_conv5"] = a
    a = inverted_residual(sd, f"{p}.conv6", a, 1, True)
    return inverted_residual(sd, f"{p}.conv7", a, 1, True)


@torch.no_grad()
def forward(sd: Dict[str, torch.Tensor], x: torch.Tensor, audio: torch.Tensor, taps: Optional[dict] = None,
            n_blocks: int = 4) -> torch.Tensor:
    """Model.forward with mode='wenet': x [B,6,160,160], audio [B,256,16,32] -> [B,3,160,160] (fp32 or fp64)."""
    x1 = inverted_residual(sd, "inc.inconv.0", x, 1, False)
    x2 = double_conv(sd, "down1.maxpool_conv.0", x1, 2)
    x3 = double_conv(sd, "down2.maxpool_conv.0", x2, 2)
    x4 = double_conv(sd, "down3.maxpool_conv.0", x3, 2)
    x5 = double_conv(sd, "down4.maxpool_conv.0", x4, 2)
    a = audio_encoder_wenet(sd, audio, taps)
    tx = _bn(sd, "bn_tx", torch.cat([x5, a], 1) + mlp_fusion(sd, x5, a))
    ox = kx = tx
    for i in range(n_blocks):
        ox = attention_block(sd, f"attention_blocks.{i}", ox, a, tx)
        kx = ox + kx
    kx = _act(_bn(sd, "bn_kx", kx))
    f = double_conv(sd, "fuse_conv.0", kx, 1)
    f = double_conv(sd, "fuse_conv.1", f, 1)
    u1 = up_block(sd, "up1", f, x4)
    u2 = up_block(sd, "up2", u1, x3)
    u3 = up_block(sd, "up3", u2, x2)
    u4 = up_block(sd, "up4", u3, x1)
    out = torch.sigmoid(_bn(sd, "outc_bn", F.conv2d(u4, sd["outc.conv.weight"], sd["outc.conv.bias"])))
    if taps is not None:
        taps.update(x5=x5, a=a, tx=tx, kx=kx, fuse=f, u4=u4, out=out)
    return out
