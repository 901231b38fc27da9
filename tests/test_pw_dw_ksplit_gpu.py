"""-m gpu: the expand + depthwise kernels (pw_dw.hip) where two waves share a channel tile and the pixel-tile count is odd:
the last pixel tile is split along K between the two waves (s-steps {0, 1} and {2, 3} of every 16-float k-group) and epilogue 1
adds the halves.  Through casync_op_pw_dw against plain PyTorch in float64, at the bound test_pw_dw_fused holds the same
kernels to (fp32 rounding: 3e-6 of the largest output).

Instances and their pixel tiles: 10x10 frame pairs 13 (6 + 6 whole ones and the shared one), one-frame deep-ring 10x10
tiles 7, 20x20 frames 25, 40x40 strips 25 (stride 1) and 23 (stride 2).  `deep` sets the engine option fuse_dw_deep: 0 sends
every 10x10 launch to the frame-pair tiles, 100 sends launches of 2..99 frames to the one-frame deep-ring tiles.  Every case
checks in the launch log that the instance it is about is the one that ran.

The frame-pair tile splits only while gemm_streamk is on: its shared tile holds the last pixels of the pair's SECOND frame, so a
frame's rounding would depend on its place in the launch, and gemm_streamk = 0 promises bits that do not."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from calipsync_amd import _lib
from gpu_util import dev, launched, nhwc, ok, options, ptr, stream

pytestmark = pytest.mark.gpu

BOUND = 3e-6   # test_pw_dw_fused / test_up_block_expand_with_commuted_upsample


def rel_err(got, ref):
    return float((got - ref).abs().max() / max(1e-6, float(ref.abs().max())))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def deep_option(deep):
    return options(fuse_dw_deep=deep) if deep is not None else contextlib.nullcontext()


def operands(hw, cin, cexp, frames, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(frames, cin, hw, hw, generator=g)
    w1 = torch.randn(cexp, cin, generator=g) / cin ** 0.5
    b1 = torch.randn(cexp, generator=g) * 0.3
    wd = torch.randn(cexp, 1, 3, 3, generator=g) / 3
    bd = torch.randn(cexp, generator=g) * 0.3
    return x, w1, b1, wd, bd


def reference(x, w1, b1, wd, bd, stride, addend=None):
    pre = F.conv2d(x.double(), w1.double()[:, :, None, None], b1.double())
    if addend is not None:
        pre = pre + addend
    e = F.leaky_relu(pre, 0.01)
    return F.leaky_relu(F.conv2d(e, wd.double(), bd.double(), stride, 1, 1, wd.shape[0]), 0.01).float()


def instance(hw, stride, frames, deep):
    if hw == 40:
        return "pw_dw_strip_kernel<40, 8, 1, 32, 16>" if stride == 1 else "pw_dw_strip_kernel<40, 4, 2, 32, 16>"
    if hw == 20:
        return f"pw_dw_kernel<20, 1, 32, 16, {stride}, 2>"
    assert hw == 10
    return "pw_dw_kernel<10, 1, 32, 32, 1, 4>" if 2 <= frames < (10 if deep is None else deep) else "pw_dw_kernel<10, 2, 32, 16, 1, 2>"


def run(lib, x, w1, b1, wd, bd, stride, deep, g_lo=None, streamk=1):
    """casync_op_pw_dw on NHWC operands; the output starts as NaN, so a pixel nobody wrote shows.  g_lo: the low-resolution
    tensor [frames * (hw/2)^2, cexp] whose bilinear x2 upsample is added in front of the first LeakyReLU."""
    frames, cin, hw, _ = x.shape
    cexp = w1.shape[0]
    ho = (hw - 1) // stride + 1
    xd, w1d, b1d, bdd = nhwc(x), w1.to(dev()), b1.to(dev()), bd.to(dev())
    wdp = wd.reshape(cexp, 9).T.contiguous().to(dev())          # tap-major [9][C]
    out = torch.full((frames, ho, ho, cexp), float("nan"), device=dev())
    with deep_option(deep), options(gemm_streamk=streamk), launched() as names:
        ok(lib.casync_op_pw_dw(ptr(xd), cin, ptr(w1d), ptr(b1d), ptr(wdp), ptr(bdd), ptr(out), cexp, frames, hw, stride, cin, cexp,
                               ptr(g_lo) if g_lo is not None else 0, cexp if g_lo is not None else 0, stream()))
    assert names == {instance(hw, stride, frames, deep)}, names
    o = out.cpu()
    assert not torch.isnan(o).any()
    return o.permute(0, 3, 1, 2)


CASES = [
    # hw, stride, cin, cexp, frames, deep
    (10, 1, 32, 32, 2, 0),        # frame pair: one workgroup, two k-tiles
    (10, 1, 32, 32, 2, None),
    (10, 1, 512, 64, 3, 0),       # the last workgroup of a channel tile holds one frame: its shared tile is wholly invalid
    (10, 1, 512, 64, 3, None),
    (10, 1, 64, 32, 1, None),     # one frame in a pair tile
    (10, 1, 64, 32, 2, 100),      # the one-frame deep-ring tile, 7 pixel tiles
    (10, 1, 64, 32, 12, 0),       # pair tiles
    (10, 1, 64, 32, 12, None),
    (20, 1, 64, 32, 1, None),
    (20, 2, 64, 32, 2, None),
    (40, 1, 32, 32, 1, None),     # strips: zero rows above and below the frame, the last strip's shared tile
    (40, 2, 32, 32, 1, None),
]


@pytest.mark.parametrize("hw,stride,cin,cexp,frames,deep", CASES)
def test_pw_dw_ksplit(lib, hw, stride, cin, cexp, frames, deep):
    x, w1, b1, wd, bd = operands(hw, cin, cexp, frames, hw * 1000 + cin + 7 * frames + stride)
    got = run(lib, x, w1, b1, wd, bd, stride, deep)
    err = rel_err(got, reference(x, w1, b1, wd, bd, stride))
    print(f"pw_dw {hw}x{hw} s{stride} cin={cin} cexp={cexp} frames={frames} deep={deep}: rel err {err:.3g}")
    assert err < BOUND, err


def upsampled(lo_pre):
    return F.interpolate(lo_pre, scale_factor=2, mode="bilinear", align_corners=True)


@pytest.mark.parametrize("hw,c_lo,cexp,frames", [(20, 32, 64, 3), (40, 32, 32, 1)])
def test_pw_dw_ksplit_upsampled_addend(lib, hw, c_lo, cexp, frames):
    """The variant with the upsampled addend: lrelu(W1b . skip + up(G) + b1), G given at half resolution."""
    x, w1, b1, wd, bd = operands(hw, c_lo, cexp, frames, hw + c_lo + frames)
    g = torch.Generator().manual_seed(99 + hw)
    g_lo = torch.randn(frames, cexp, hw // 2, hw // 2, generator=g)
    got = run(lib, x, w1, b1, wd, bd, 1, None, g_lo=nhwc(g_lo).reshape(-1, cexp).contiguous())
    err = rel_err(got, reference(x, w1, b1, wd, bd, 1, addend=upsampled(g_lo.double())))
    print(f"pw_dw + addend {hw}x{hw} c_lo={c_lo} cexp={cexp} frames={frames}: rel err {err:.3g}")
    assert err < BOUND, err


# one launch per instance with an odd tile count over a wave pair
# (the last entry: gemm_streamk; the frame pair runs its unsplit order with 0)
INSTANCES = [(10, 1, 2, 0, 1), (10, 1, 2, 0, 0), (10, 1, 2, 100, 1), (20, 1, 1, None, 1), (20, 2, 1, None, 1), (40, 1, 1, None, 1),
             (40, 2, 1, None, 1)]


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("hw,stride,frames,deep,streamk", INSTANCES)
def test_pw_dw_ksplit_each_half_alone(lib, hw, stride, frames, deep, streamk, half):
    """Inputs that are zero outside the channels one wave's s-steps cover (channel % 4 in {0, 1} for the first wave of a pair,
    {2, 3} for the second), then the complement: the shared tile's pixels then come from ONE wave's partial sum, so a dropped
    or doubled half is an error of the size of the output itself, not of its rounding."""
    cin, cexp = 64, 32
    x, w1, b1, wd, bd = operands(hw, cin, cexp, frames, hw * 10 + stride + half)
    keep = (torch.arange(cin) % 4 // 2) == half
    x = x * keep[None, :, None, None]
    got = run(lib, x, w1, b1, wd, bd, stride, deep, streamk=streamk)
    ref = reference(x, w1, b1, wd, bd, stride)
    err = rel_err(got, ref)
    print(f"pw_dw {hw}x{hw} s{stride} deep={deep} gemm_streamk={streamk} half {half} alone: rel err {err:.3g}")
    assert err < BOUND, err
    # the control: without this half's inputs the reference itself moves by far more than the bound
    gone = reference(torch.zeros_like(x), w1, b1, wd, bd, stride)
    assert rel_err(gone, ref) > 0.05


def test_frame_pair_bits_do_not_depend_on_the_pairing_without_k_splits(lib):
    """gemm_streamk = 0: a frame gives the same bits as the first and as the second frame of its pair (four frames, then the
    last three of them: every frame changes sides), and the result still meets the bound."""
    x, w1, b1, wd, bd = operands(10, 64, 32, 4, 4242)
    full = run(lib, x, w1, b1, wd, bd, 1, 0, streamk=0)
    shifted = run(lib, x[1:], w1, b1, wd, bd, 1, 0, streamk=0)
    assert torch.equal(full[1:], shifted)
    assert rel_err(full, reference(x, w1, b1, wd, bd, 1)) < BOUND
