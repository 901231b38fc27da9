"""-m gpu: the loss handle (include/casync_ploss.h, calipsync_amd/losses.py) against the tests/vgg_ref.py restatement in float64
on the CPU, on recipe weights, computed live.  The bar of every summing stage is the project's bar for fp32 handles: max and
mean error against float64 at most 4x the error of the same restatement in fp32 on the CPU (kernel_ledger_ploss.ratio4; a
reference error below one rounding of the largest value counts as that rounding).  Stages that move, mask or compare data are
compared exactly.  The kernels alone are tests/test_kernel_ledger_ploss_gpu.py (the same helpers on the shapes named there).

Each of the three loss values is held ON ITS OWN to the 4x bar in test_each_loss_value_on_its_own, as root-mean-square relative
errors over DRAWS inputs per shape (the decision-stable pair first): one value's error over ONE realisation of fp32 torch's error is
a ratio of two roundings with a Cauchy-like tail (two independent zero-mean errors of equal size differ by more than 4x in 16 % of
draws), and fp32 torch's own error on loss_perceptual at 7 x 9 ranges from 2.6e-7 on the stable pair to an RMS of 3.9e-6.  Over the 24
draws the engine's RMS error on loss_perceptual measured 1.35x / 1.98x / 1.58x / 1.22x fp32 torch's, with no bias (means below a
quarter of the RMS) and no scale error in F (regression slope of the feature error on F: some 1e-9, fp32 torch's the same): the
1.4-2.0x of d itself, not a coherent excess.  The single-draw ratios on the stable pair are printed by the end-to-end test."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_ledger_ploss as kl
import ploss_cases as pc
import vgg_ref
from calipsync_amd import _lib, losses

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W_PIX, W_PERC = 1.0, losses.PERCEPTUAL_WEIGHT
IDS = [f"b{b}-{h}x{w}" for b, h, w in pc.SHAPES]


@functools.lru_cache(maxsize=None)
def engine():
    return losses.PerceptualEngine(pc.state_dict(), DEV)


@functools.lru_cache(maxsize=None)
def training_loss():
    return losses.TrainingLoss(state_dict=pc.state_dict(), device=DEV)


def held(got, ref64, ref32, what, missed=None):
    """missed: a list that collects the stages above the bar instead of stopping at the first (the caller asserts it empty)"""
    err, figures = kl.ratio4(got, ref64, ref32)
    print(f"{what}: {figures}")
    if missed is not None and err > 1.0:
        missed.append(f"{what}: {figures}")
        return
    assert err <= 1.0, f"{what}: {figures}: above 4x fp32 torch"


def scalar_figures(got, ref64, ref32, what):
    """printed only: one value's error as a multiple of fp32 torch's (at least one fp32 rounding of the value)"""
    e, r = abs(float(got) - float(ref64)), max(abs(float(ref32) - float(ref64)), 2.0 ** -24 * abs(float(ref64)))
    print(f"{what}: {float(got):.9g} against {float(ref64):.9g}: error {e:.3e}, {e / r:.2f}x fp32 torch")


# ------------------------------------------------------------------------------------------------ 1. kernels alone
def test_pool_adjoint_ties_zero_windows_and_dropped_edges():
    """the first of two equal positive maxima wins; an all-zero window and a dropped odd row and column get zeros"""
    a = torch.zeros(1, 5, 5, 4)
    a[0, 0, 0], a[0, 0, 1], a[0, 1, 0], a[0, 1, 1] = 0.5, 2.0, 2.0, 1.0          # window (0, 0): the maximum twice, (0, 1) first
    a[0, 2, 2, :], a[0, 3, 3, :] = 3.0, 3.0                                       # window (1, 1): twice, (0, 0) first
    a[0, 4, :, :], a[0, :, 4, :] = 9.0, 9.0                                       # the dropped row and column hold the largest values
    gp = torch.arange(1, 17, dtype=torch.float32).reshape(1, 2, 2, 4)
    out, ok = kl.run_pool_bwd(gp, a)
    out = out.cpu()
    assert ok and torch.equal(out[0, 0, 1], gp[0, 0, 0]) and torch.equal(out[0, 2, 2], gp[0, 1, 1])
    assert float(out.abs().sum()) == float(gp[0, 0, 0].sum() + gp[0, 1, 1].sum())          # windows (0, 1) and (1, 0) are all zero
    assert torch.equal(out, vgg_ref.nhwc(vgg_ref.pool_adjoint(vgg_ref.nchw(gp), vgg_ref.nchw(a))))


# ------------------------------------------------------------------------------------------------ 2. forward taps
@functools.lru_cache(maxsize=None)
def reference_taps(shape, dtype):
    pred, label = pc.pair(*shape)
    with torch.no_grad():
        t = pc.model(dtype).taps(torch.cat([pred, label]).to(dtype))
    t["d"] = t["conv3_3"][:shape[0]] - t["conv3_3"][shape[0]:]
    return {k: vgg_ref.nhwc(v) for k, v in t.items()}


@pytest.mark.parametrize("shape", pc.SHAPES, ids=IDS)
def test_forward_taps(shape):
    pred, label = (t.to(DEV) for t in pc.pair(*shape))
    ref64, ref32 = reference_taps(shape, torch.float64), reference_taps(shape, torch.float32)
    missed = []
    for name in ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "d"):
        held(engine().forward_tap(pred, label, name), ref64[name], ref32[name], f"{shape} {name}", missed)
    for pool, src in (("pool1", "conv1_2"), ("pool2", "conv2_2")):               # a pool of the engine's own tap: exact
        got, a = engine().forward_tap(pred, label, pool).cpu(), engine().forward_tap(pred, label, src).cpu()
        assert torch.equal(got, vgg_ref.nhwc(F.max_pool2d(vgg_ref.nchw(a), 2, 2))), pool
    assert not missed, "above 4x fp32 torch:\n" + "\n".join(missed)


def test_an_images_features_do_not_depend_on_the_batch():
    pred, label = (t.to(DEV) for t in pc.pair(3, 12, 20))
    for stage in ("conv1_2", "conv3_3", "d"):
        full = engine().forward_tap(pred, label, stage)
        for i in range(3):
            one = engine().forward_tap(pred[i:i + 1].contiguous(), label[i:i + 1].contiguous(), stage)
            assert torch.equal(one[0], full[i]), (stage, i)
            if stage != "d":
                assert torch.equal(one[1], full[3 + i]), (stage, i, "label")


# ------------------------------------------------------------------------------------------------ 3. backward, by segment
SEGMENTS = (("conv", 14, None), ("mask", None, "a3_2"), ("conv", 12, None), ("mask", None, "a3_1"), ("conv", 10, None), ("pool", None, "a2_2"),
            ("conv", 7, None), ("mask", None, "a2_1"), ("conv", 5, None), ("pool", None, "a1_2"), ("conv", 2, None), ("mask", None, "a1_1"))


@pytest.mark.parametrize("shape", pc.SHAPES[:4], ids=IDS[:4])
def test_backward_segment_by_segment(shape):
    """every backward stage applied in float64 (and in fp32 torch) to the ENGINE's own incoming gradient and saved activation:
    no mask flip can enter"""
    b, h, w = shape
    pred, label = (t.to(DEV) for t in pc.pair(*shape))
    sd = pc.state_dict()
    _, saved = engine().forward(pred, label, W_PIX, W_PERC)
    sv = {k: v.cpu() for k, v in pc.saved_views(saved, b, h, w).items()}
    assert torch.equal(sv["d"], engine().forward_tap(pred, label, "d").cpu())
    assert torch.equal(sv["a3_2"], engine().forward_tap(pred, label, "conv3_2").cpu()[:b])
    s = torch.tensor(0.75, device=DEV)
    taps = [engine().backward_tap(pred, label, s, saved, W_PIX, W_PERC, k).cpu() for k in range(len(losses.BACKWARD_STAGES))]
    incoming, missed = sv["d"], []
    for k, (kind, idx, act) in enumerate(SEGMENTS):
        what = f"{shape} backward stage {k} {losses.BACKWARD_STAGES[k]}"
        if kind == "conv":
            held(taps[k], vgg_ref.nhwc(vgg_ref.conv_t(sd, idx, vgg_ref.nchw(incoming), torch.float64)),
                 vgg_ref.nhwc(vgg_ref.conv_t(sd, idx, vgg_ref.nchw(incoming), torch.float32)), what, missed)
        elif kind == "mask":
            assert torch.equal(taps[k], vgg_ref.relu_mask(incoming, sv[act])), what
        else:
            assert torch.equal(taps[k], vgg_ref.nhwc(vgg_ref.pool_adjoint(vgg_ref.nchw(incoming), vgg_ref.nchw(sv[act])))), what
        incoming = taps[k]
    n_feat, n_pix = sv["d"].numel(), pred.numel()
    p, l = pred.cpu(), label.cpu()

    def last(dtype):
        g = vgg_ref.conv_t(sd, 0, vgg_ref.nchw(incoming), dtype)
        return 0.75 * (W_PERC * 2.0 / n_feat * g + W_PIX * torch.sign(p.to(dtype) - l.to(dtype)) / n_pix)
    held(taps[12], last(torch.float64), last(torch.float32), f"{shape} backward stage 12 grad_pred", missed)
    assert torch.equal(taps[12], engine().backward(pred, label, s, saved, W_PIX, W_PERC).cpu())
    assert not missed, "above 4x fp32 torch:\n" + "\n".join(missed)


# ------------------------------------------------------------------------------------------------ 4. end to end
@functools.lru_cache(maxsize=None)
def reference_step(shape, dtype):
    pred, label = pc.stable_pair(*shape)
    x = pred.detach().clone().to(dtype).requires_grad_(True)
    out = vgg_ref.step_loss(pc.model(dtype), x, label.to(dtype), W_PERC, W_PIX)
    out[0].backward()
    return [float(v.detach()) for v in out], x.grad


@pytest.mark.parametrize("shape", pc.END_TO_END, ids=IDS[:4])
def test_end_to_end_against_float64_autograd(shape):
    b, h, w = shape
    pred, label = pc.stable_pair(*shape)
    margin = pc.margin_of(pred)
    print(f"{shape}: decision margin {margin:.2e} (needs {pc.MARGIN:.0e})")
    assert margin >= pc.MARGIN
    (l64, g64), (l32, g32) = reference_step(shape, torch.float64), reference_step(shape, torch.float32)
    pd, ld = pred.to(DEV), label.to(DEV)
    got, saved = engine().forward(pd, ld, W_PIX, W_PERC)
    grad = engine().backward(pd, ld, torch.ones((), device=DEV), saved, W_PIX, W_PERC)
    got = got.cpu()
    held(grad, g64, g32, f"{shape} grad_pred")
    # the two sums against float64 sums over the engine's own d and pred - label: the bound of a tree sum of non-negative terms
    d = pc.saved_views(saved, b, h, w)["d"].cpu().double()
    for name, value, terms in (("perceptual", got[2], d ** 2), ("pixel", got[1], (pred.double() - label.double()).abs())):
        want, n = float(terms.sum()) / terms.numel(), terms.numel()
        bound = (math.log2(n) + 2) * 2.0 ** -24
        print(f"{shape} {name}: {float(value):.9g} against {want:.9g}: relative {abs(float(value) - want) / want:.2e} (bound {bound:.2e})")
        assert abs(float(value) - want) <= bound * want, name
    assert float(got[0]) == float(np.float32(W_PIX) * got[1].numpy() + np.float32(W_PERC) * got[2].numpy())
    for i, name in enumerate(("loss", "loss_pixel", "loss_perceptual")):
        scalar_figures(got[i], l64[i], l32[i], f"{shape} {name}")
    # (printed: one draw; each value is held on its own over DRAWS inputs, this pair among them, in test_each_loss_value_on_its_own)


DRAWS = 24


@functools.lru_cache(maxsize=None)
def loss_draws(shape):
    """DRAWS inputs of a shape (the decision-stable pair, then recipe seeds) with the three values in float64 and in fp32 torch"""
    out = []
    for k in range(DRAWS):
        pred, label = pc.stable_pair(*shape) if k == 0 else pc.pair(*shape, 100 + k)
        with torch.no_grad():
            l64 = [float(v) for v in vgg_ref.step_loss(pc.model(torch.float64), pred.double(), label.double(), W_PERC, W_PIX)]
            l32 = [float(v) for v in vgg_ref.step_loss(pc.model(torch.float32), pred, label, W_PERC, W_PIX)]
        out.append((pred, label, l64, l32))
    return out


@pytest.mark.parametrize("shape", pc.END_TO_END, ids=IDS[:4])
def test_each_loss_value_on_its_own(shape):
    """loss, loss_pixel and loss_perceptual, each alone: RMS relative error against float64 over DRAWS inputs at most 4x fp32
    torch's RMS relative error over the same inputs (at least one fp32 rounding)"""
    rel_e, rel_r = np.zeros((DRAWS, 3)), np.zeros((DRAWS, 3))
    for k, (pred, label, l64, l32) in enumerate(loss_draws(shape)):
        got, _ = engine().forward(pred.to(DEV), label.to(DEV), W_PIX, W_PERC, keep=False)
        got = got.cpu().double().numpy()
        rel_e[k] = (got - np.asarray(l64)) / np.asarray(l64)
        rel_r[k] = (np.asarray(l32) - np.asarray(l64)) / np.asarray(l64)
    rms_e, rms_r = np.sqrt((rel_e ** 2).mean(0)), np.maximum(np.sqrt((rel_r ** 2).mean(0)), 2.0 ** -24)
    for i, name in enumerate(("loss", "loss_pixel", "loss_perceptual")):
        print(f"{shape} {name}: RMS relative error {rms_e[i]:.2e}, fp32 torch {rms_r[i]:.2e}: {rms_e[i] / rms_r[i]:.2f}x; mean {rel_e[:, i].mean():+.2e}")
    assert (rms_e <= 4.0 * rms_r).all(), (rms_e / rms_r).tolist()


# ------------------------------------------------------------------------------------------------ 5. autograd
def test_autograd_through_a_conv_in_front():
    """a 1x1 conv (6 -> 3) whose output IS the decision-stable prediction (its input solved for in float64): loss.backward() gives
    the conv the gradients the restatement gives"""
    shape = (2, 7, 9)
    pred, label = (t.detach() for t in pc.stable_pair(*shape))
    gen = torch.Generator().manual_seed(0x1640)
    wt = torch.randn(3, 6, generator=gen, dtype=torch.float64) * 0.5
    bias = torch.randn(3, generator=gen, dtype=torch.float64) * 0.1
    x = torch.einsum("ck,bchw->bkhw", torch.linalg.pinv(wt).t(), pred.double() - bias.reshape(1, 3, 1, 1)).float()     # W x + b = pred

    def reference(dtype):
        conv = torch.nn.Conv2d(6, 3, 1).to(dtype)
        with torch.no_grad():
            conv.weight.copy_(wt.reshape(3, 6, 1, 1)), conv.bias.copy_(bias)
        vgg_ref.step_loss(pc.model(dtype), conv(x.to(dtype)), label.to(dtype), W_PERC, W_PIX)[0].backward()
        return conv.weight.grad, conv.bias.grad
    conv = torch.nn.Conv2d(6, 3, 1).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(wt.reshape(3, 6, 1, 1)), conv.bias.copy_(bias)
        assert pc.margin_of(conv(x.to(DEV)).cpu()) >= pc.MARGIN         # the conv's fp32 output is still stable
    loss, pixel, perceptual = training_loss()(conv(x.to(DEV)), label.to(DEV))
    assert loss.requires_grad and not pixel.requires_grad and not perceptual.requires_grad
    loss.backward()
    (w64, b64), (w32, b32) = reference(torch.float64), reference(torch.float32)
    held(conv.weight.grad, w64, w32, "conv weight gradient")
    held(conv.bias.grad, b64, b32, "conv bias gradient")


def test_scaling_get_loss_no_grad_and_repeats():
    shape = (2, 10, 14)
    pred, label = (t.to(DEV) for t in pc.pair(*shape))
    tl = training_loss()

    def grad_of(scale):
        p = pred.clone().requires_grad_(True)
        out = tl(p, label)
        (out[0] if scale == 1 else scale * out[0]).backward()
        return [o.detach().clone() for o in out], p.grad
    (l1, g1), (l1b, g1b), (_, g4) = grad_of(1), grad_of(1), grad_of(4)
    assert all(torch.equal(a, b) for a, b in zip(l1, l1b)) and torch.equal(g1, g1b)          # two calls in a row: identical bits
    assert torch.equal(g4, 4.0 * g1) and float(g1.abs().max()) > 0                            # (4 loss).backward(): exactly 4x the bits
    label_leaf = label.clone().requires_grad_(True)
    tl(pred.clone().requires_grad_(True), label_leaf)[0].backward()
    assert label_leaf.grad is None                                                            # no gradient reaches the label
    pl = losses.PerceptualLoss(torch.nn.MSELoss(), state_dict=pc.state_dict(), device=DEV)
    p = pred.clone().requires_grad_(True)
    got = pl.get_loss(p, label)
    assert torch.equal(got.detach(), l1[2])                                                   # TrainingLoss's third value, bit for bit
    got.backward()
    assert float(p.grad.abs().max()) > 0
    # under no_grad (or for a prediction that needs no gradient) nothing is saved
    kept, real = [], tl.engine.forward

    def spy(*a, **kw):
        out = real(*a, **kw)
        kept.append(out[1])
        return out
    tl.engine.forward = spy
    try:
        with torch.no_grad():
            quiet = tl(pred.clone().requires_grad_(True), label)
        plain = tl(pred, label)
        loud = tl(pred.clone().requires_grad_(True), label)
    finally:
        del tl.engine.forward
    assert kept[0] is None and kept[1] is None and kept[2] is not None
    assert not quiet[0].requires_grad and not plain[0].requires_grad and loud[0].requires_grad
    assert all(torch.equal(a, b) for a, b in zip(quiet, l1)) and all(torch.equal(a, b) for a, b in zip(plain, l1))
    with pytest.raises(RuntimeError, match="ROCm device"):
        tl(pred.cpu(), label.cpu())
    with pytest.raises(RuntimeError, match="contiguous"):
        tl(pred.transpose(2, 3), label.transpose(2, 3))


# ------------------------------------------------------------------------------------------------ 6. workspace, refusals
def test_scratch_contents_change_no_bit():
    b, h, w = shape = (2, 7, 9)
    pred, label = (t.to(DEV) for t in pc.pair(*shape))
    e = engine()
    s = torch.tensor(1.0, device=DEV)
    results = []
    for fill in ("nan", "zeros", "ones"):
        scratch = torch.empty(e.scratch_bytes(b, h, w), dtype=torch.uint8, device=DEV)
        words = scratch.view(torch.int32)
        words.fill_({"nan": 0x7FC00000, "zeros": 0, "ones": -1}[fill])            # quiet NaNs; zeros; all bits set (NaN as fp32 and fp64)
        saved = torch.zeros(e.saved_bytes(b, h, w), dtype=torch.uint8, device=DEV)
        got, _ = e.forward(pred, label, W_PIX, W_PERC, scratch=scratch, saved=saved)
        words.fill_({"nan": 0x7FC00000, "zeros": 0, "ones": -1}[fill])
        grad = e.backward(pred, label, s, saved, W_PIX, W_PERC, scratch=scratch)
        words.fill_({"nan": 0x7FC00000, "zeros": 0, "ones": -1}[fill])
        quiet, _ = e.forward(pred, label, W_PIX, W_PERC, keep=False, scratch=scratch)
        results.append([got.cpu(), saved.cpu(), grad.cpu(), quiet.cpu()])
    for other in results[1:]:
        for a, c in zip(results[0], other):
            assert torch.equal(a, c)
    assert bool(torch.isfinite(results[0][0]).all()) and bool(torch.isfinite(results[0][2]).all())
    assert torch.equal(results[0][0], results[0][3])                              # keeping nothing changes no loss bit


def test_no_pixel_kernel_without_a_pixel_weight():
    """w_pix == 0: the pixel reduction is not launched (pixel is 0) and the backward reads neither pred nor label"""
    import gpu_util
    b, h, w = shape = (2, 7, 9)
    pred, label = (t.to(DEV) for t in pc.pair(*shape))
    e = engine()
    with gpu_util.launched() as with_pix:
        e.forward(pred, label, 1.0, 1.0, keep=False)
    with gpu_util.launched() as without:
        got, saved = e.forward(pred, label, 0.0, 1.0)
    assert "ploss_absdiff_kernel" in with_pix and "ploss_absdiff_kernel" not in without and "ploss_sqdiff_kernel" in without
    got = got.cpu()
    assert float(got[1]) == 0.0 and float(got[0]) == float(got[2]) > 0
    s = torch.ones((), device=DEV)
    lib, ws, grad = _lib.load(), torch.empty(e.scratch_bytes(b, h, w), dtype=torch.uint8, device=DEV), torch.empty_like(pred)
    st = lib.casync_ploss_backward(e._h, None, None, s.data_ptr(), grad.data_ptr(), b, h, w, 0.0, 1.0, saved.data_ptr(), saved.numel(), ws.data_ptr(),
                                   ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.casync_last_error()
    assert torch.equal(grad, e.backward(pred, label, s, saved, 0.0, 1.0))


def test_refusals_come_before_any_launch():
    lib, e = _lib.load(), engine()
    t = torch.zeros(1024, device=DEV)
    args = (t.data_ptr(), t.data_ptr())
    strm = torch.cuda.current_stream().cuda_stream
    for b, h, w in ((328, 160, 160), (1, 3, 8), (1, 8, 3), (0, 8, 8)):             # [328,160,160,64] fp32 reaches 2 GiB
        st = lib.casync_ploss_forward(e._h, *args, b, h, w, 1.0, 0.1, t.data_ptr(), None, 0, t.data_ptr(), 4096, strm)
        assert st == -1 and _lib.load().casync_last_error(), (b, h, w)               # CASYNC_ERR_ARG
    lib.casync_ploss_forward(e._h, *args, 328, 160, 160, 1.0, 0.1, t.data_ptr(), None, 0, t.data_ptr(), 4096, strm)
    assert b"2 GiB" in lib.casync_last_error()                                     # the tensor is named
    st = lib.casync_ploss_forward(e._h, *args, 1, 8, 8, 1.0, 0.1, t.data_ptr(), None, 0, t.data_ptr(), 4096, strm)
    assert st < 0 and b"scratch" in lib.casync_last_error()                        # too small: refused, nothing launched
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0.0
