"""What the GPU tests of the loss handle share (tests/test_ploss_gpu.py, tests/test_ploss_stream_contract_gpu.py): the shapes,
the recipe weights in three forms, and DECISION-STABLE inputs.

The gradient of the loss goes through six ReLU masks and two pool arg-maxima of the prediction's forward.  An input at which
some ReLU input sits within rounding distance of zero, or a pool window's two largest values within rounding distance of each
other, has a gradient that fp32 and float64 may take through different elements: an end-to-end comparison on it measures the
coin toss, not the arithmetic.  stable_pair() therefore returns inputs built on the CPU, in float64, for which
  margin_of(pred) = the smallest, over the stages, of min |ReLU input| / (the stage's largest magnitude) and of
                    min (largest - second largest of a pool window with a positive maximum) / (the stage's largest magnitude)
is at least MARGIN = 1e-4, the issue's figure, at every shape; the tests assert it.  With He-scaled weights about 2.4e-4 of all
ReLU inputs lie inside 1e-4 for any seed, so from the 7 x 9 batch (24 000 ReLU inputs) up no seed qualifies by itself (none of 400
did; the 4 x 4 image, 3 600 inputs, does with one seed in three).  tools/make_ploss_stable_inputs.py starts from the seeds below and
moves the prediction alone, by at most 3.5e-4 a pixel, down the gradient of the squared shortfalls until the margin is 1.5e-4 or
more; what it wrote is tests/golden/ploss_stable_inputs.npz.  Everything here runs on the CPU."""
from __future__ import annotations

import functools
import os

import numpy as np
import torch

import vgg_ref
from calipsync_amd import recipe

SHAPES = ((1, 4, 4), (3, 12, 20), (2, 10, 14), (2, 7, 9), (1, 160, 160))       # odd at the second pool; odd at both; production
END_TO_END = SHAPES[:4]
SEEDS = {(1, 4, 4): 0x2000, (2, 7, 9): 0x20F1, (2, 10, 14): 0x20D9, (3, 12, 20): 0x20FC}       # where the repair starts from
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ploss_stable_inputs.npz")
MARGIN = 1e-4                             # the issue's: of a stage's largest magnitude
RELU_INPUTS = (0, 2, 5, 7, 10, 12)        # features index of the convs a ReLU follows
POOL_INPUTS = (3, 8)                      # features index of the ReLUs a pool follows


@functools.lru_cache(maxsize=None)
def state_dict():
    return recipe.make_vgg19_state_dict()


@functools.lru_cache(maxsize=None)
def model(dtype):
    return vgg_ref.model(state_dict(), dtype)


def margin_of(pred) -> float:
    """the decision margin of a prediction's float64 forward (the module's docstring)"""
    worst = 1.0
    x = torch.as_tensor(pred).double()
    with torch.no_grad():
        for i, layer in enumerate(model(torch.float64).features):
            x = layer(x)
            top = float(x.abs().max())
            if i in RELU_INPUTS:
                worst = min(worst, float(x.abs().min()) / top)
            if i in POOL_INPUTS:
                b, c, h, w = x.shape
                ho, wo = h // 2, w // 2
                win = x[:, :, :2 * ho, :2 * wo].reshape(b, c, ho, 2, wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, ho, wo, 4)
                t = win.topk(2, dim=-1).values
                gap = torch.where(t[..., 0] > 0, t[..., 0] - t[..., 1], torch.ones((), dtype=torch.float64))
                worst = min(worst, float(gap.min()) / top)
    return worst


@functools.lru_cache(maxsize=None)
def stable_pair(b, h, w):
    """(pred, label) float32 [b,3,h,w] tensors of the fixture; margin_of(pred) >= MARGIN"""
    with np.load(GOLDEN) as z:
        pred, label = z[f"b{b}_{h}x{w}_pred"], z[f"b{b}_{h}x{w}_label"]
    return torch.from_numpy(np.ascontiguousarray(pred)), torch.from_numpy(np.ascontiguousarray(label))


def pair(b, h, w, seed_offset=0):
    """plain recipe inputs (the tests that compare the engine with its own taps need no stability)"""
    pred, label = recipe.make_loss_inputs(b, h, w, 0x1630 + 64 * seed_offset + b)
    return torch.from_numpy(pred), torch.from_numpy(label)


def saved_views(saved, b, h, w):
    """the seven tensors of the handle's `saved` bytes (include/casync_ploss.h), NHWC float32 views"""
    h2, w2, h3, w3 = h // 2, w // 2, h // 4, w // 4
    shapes = [("a1_1", (b, h, w, 64)), ("a1_2", (b, h, w, 64)), ("a2_1", (b, h2, w2, 128)), ("a2_2", (b, h2, w2, 128)),
              ("a3_1", (b, h3, w3, 256)), ("a3_2", (b, h3, w3, 256)), ("d", (b, h3, w3, 256))]
    out, off = {}, 0
    for name, shape in shapes:
        n = int(np.prod(shape)) * 4
        out[name] = saved[off:off + n].view(torch.float32).reshape(shape)
        off += (n + 255) // 256 * 256
    assert off == saved.numel(), (off, saved.numel())
    return out
