"""A restatement of the reference's loss network in torch: torchvision's ``vgg19().features[:15]`` (step2_train_unet.py:12-36)
as an ``nn.Sequential`` under a module attribute ``features``, so that its state dict has the vgg19 state dict's own names,
``features.{0,2,5,7,10,12,14}.{weight,bias}``.  torchvision is not in the build image: the layer list below is written from
torchvision's ``cfgs['E']`` (64, 64, 'M', 128, 128, 'M', 256, 256, 256, ...; 3x3 convs with padding 1, ReLU behind each,
MaxPool2d(2, 2)) and is NOT pinned against torchvision's module itself.  The slice ends on features.14, the conv3_3 WITHOUT its
ReLU.  Also the step's loss (step2_train_unet.py:107-112) and the backward stages of the engine, one at a time."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from calipsync_amd import losses

# torchvision's cfgs['E'] up to the third conv of its third block, spelled out here and NOT taken from the module under test:
# 3 -> 64 -> 64 -> M -> 128 -> 128 -> M -> 256 -> 256 -> 256; make_layers() puts a ReLU behind every conv, so the convs sit at
# features.0, 2, 5, 7, 10, 12, 14 and the pools at features.4 and 9
CFG_E = (64, 64, "M", 128, 128, "M", 256, 256, 256)


def _layout():
    conv_at, pool_at, i, cin = {}, [], 0, 3
    for v in CFG_E:
        if v == "M":
            pool_at.append(i)
            i += 1
        else:
            conv_at[i] = (cin, v)
            cin = v
            i += 2
    return conv_at, tuple(pool_at), i - 1          # (the slice ends on the last conv, in front of its ReLU)


CONV_AT, POOL_AT, N_LAYERS = _layout()
assert sorted(CONV_AT) == [0, 2, 5, 7, 10, 12, 14] and POOL_AT == (4, 9) and N_LAYERS == 15
# the engine's forward taps (losses.FORWARD_STAGES[:9]) by the index of the layer whose output they are
TAP_LAYER = {"conv1_1": 1, "conv1_2": 3, "pool1": 4, "conv2_1": 6, "conv2_2": 8, "pool2": 9, "conv3_1": 11, "conv3_2": 13, "conv3_3": 14}


class Vgg19Features15(nn.Module):
    def __init__(self):
        super().__init__()
        layers = []
        for i in range(N_LAYERS):
            if i in CONV_AT:
                layers.append(nn.Conv2d(CONV_AT[i][0], CONV_AT[i][1], kernel_size=3, padding=1))
            elif i in POOL_AT:
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers.append(nn.ReLU(inplace=False))
        self.features = nn.Sequential(*layers)

    def forward(self, x):
        return self.features(x)

    def taps(self, x):
        """{tap name: NCHW tensor} of every conv output behind its ReLU (conv3_3 has none) and both pools"""
        out, name_of = {}, {v: k for k, v in TAP_LAYER.items()}
        for i, layer in enumerate(self.features):
            x = layer(x)
            if i in name_of:
                out[name_of[i]] = x
        return out


def model(sd, dtype=torch.float64) -> Vgg19Features15:
    """the restatement with the entries of `sd` (numpy or tensors; other keys ignored) in `dtype`, frozen as the reference's"""
    m = Vgg19Features15()
    own = {k: torch.as_tensor(np.asarray(sd[k])) for k in m.state_dict()}
    m.load_state_dict(own)
    m = m.to(dtype).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def step_loss(m, preds, labels, perceptual_weight=losses.PERCEPTUAL_WEIGHT, pixel_weight=1.0):
    """(loss, loss_pixel, loss_perceptual) as the step computes them"""
    perceptual = F.mse_loss(m(preds), m(labels).detach())
    pixel = F.l1_loss(preds, labels)
    return pixel_weight * pixel + perceptual_weight * perceptual, pixel, perceptual


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def conv_t(sd, idx, g, dtype):
    """the backward-data pass of features.<idx> on g (NCHW)"""
    w = torch.as_tensor(np.asarray(sd[f"features.{idx}.weight"])).to(dtype)
    return F.conv_transpose2d(g.to(dtype), w, padding=1)


def relu_mask(g, a):
    """g * (a > 0), exact in any dtype"""
    return torch.where(a > 0, g, torch.zeros_like(g))


def pool_adjoint(g_pool, a):
    """the adjoint of MaxPool2d(2, 2) on the post-ReLU activation a (NCHW) with the ReLU mask in front of it: the first maximum of
    each window in row-major order (torch's > rule) receives the gradient if it is positive; data movement only, exact"""
    b, c, h, w = a.shape
    ho, wo = h // 2, w // 2
    win = a[:, :, :2 * ho, :2 * wo].reshape(b, c, ho, 2, wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, ho, wo, 4)
    k = torch.zeros(win.shape[:-1], dtype=torch.long)
    m = win[..., 0].clone()
    for j in (1, 2, 3):
        better = win[..., j] > m
        k = torch.where(better, torch.full_like(k, j), k)
        m = torch.where(better, win[..., j], m)
    gv = torch.where(m > 0, g_pool, torch.zeros_like(g_pool))
    out = torch.zeros(b, c, ho, wo, 4, dtype=g_pool.dtype)
    out.scatter_(-1, k.unsqueeze(-1), gv.unsqueeze(-1))
    full = torch.zeros(b, c, h, w, dtype=g_pool.dtype)
    full[:, :, :2 * ho, :2 * wo] = out.reshape(b, c, ho, wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, 2 * ho, 2 * wo)
    return full
