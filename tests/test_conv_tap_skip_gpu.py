"""-m gpu: the dense 3x3 conv with position-major rows and the tap walk of `conv_skip` (gemm.hip, CONV instances), through
casync_op_conv3x3 / casync_op_conv3x3_ex against F.conv2d in float64.  The output starts as NaN: a hole in the row -> pixel
remap shows.  conv_skip = 0 walks all nine taps in the same row order and must give the same bits."""
import pytest
import torch
import torch.nn.functional as F

from calipsync_amd import _lib
from gpu_util import dev, nhwc, ok, options, ptr, stream

pytestmark = pytest.mark.gpu

BOUND = 3e-6   # test_conv3x3_implicit_gemm holds the same kernel to it


def rel_err(got, ref):
    return float((got - ref).abs().max() / max(1e-6, float(ref.abs().max())))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


CASES = [
    # b, h, w, cin, (stride_h, stride_w), pad, cout
    (1, 16, 16, 64, (2, 2), 3, 64),      # conv5 geometry
    (2, 16, 16, 64, (2, 2), 3, 64),
    (31, 16, 16, 64, (2, 2), 3, 64),     # 31 and 33: tiles straddle positions
    (32, 16, 16, 64, (2, 2), 3, 64),
    (33, 16, 16, 64, (2, 2), 3, 64),
    (70, 16, 16, 64, (2, 2), 3, 64),     # more frames than rows of a tile
    (3, 32, 32, 32, (2, 2), 1, 64),      # conv3 geometry
    (32, 32, 32, 32, (2, 2), 1, 64),
    (3, 9, 13, 64, (1, 1), 1, 64),       # ragged, non-square
    (1, 7, 5, 32, (1, 1), 0, 128),       # nothing to skip
    (2, 16, 32, 64, (1, 2), 1, 64),      # AudioConvWenet's conv3 stride
]


@pytest.mark.parametrize("b,h,w,cin,stride,pad,cout", CASES)
def test_conv3x3_tap_skip(lib, b, h, w, cin, stride, pad, cout):
    g = torch.Generator().manual_seed(h * 31 + w + 7 * b + cin)
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    bias = torch.randn(cout, generator=g)
    ref = F.leaky_relu(F.conv2d(x.double(), wt.double(), bias.double(), stride, pad), 0.01).float()
    ho, wo = ref.shape[2], ref.shape[3]
    xd, bd = nhwc(x), bias.to(dev())
    wp = wt.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous().to(dev())
    outs = {}
    for skip in (0, 1):
        out = torch.full((b, ho, wo, cout), float("nan"), device=dev())
        with options(conv_skip=skip):
            if stride[0] == stride[1]:
                ok(lib.casync_op_conv3x3(ptr(xd), ptr(wp), ptr(bd), ptr(out), b, h, w, cin, cout, stride[0], pad, 1, stream()))
            else:
                ok(lib.casync_op_conv3x3_ex(ptr(xd), ptr(wp), ptr(bd), ptr(out), b, h, w, cin, cout, stride[0], stride[1], pad, 1,
                                            stream()))
        outs[skip] = out.cpu()
    for skip, o in outs.items():
        assert not torch.isnan(o).any(), f"conv_skip={skip}: pixels nobody wrote"                      # (iii)
        err = rel_err(o.permute(0, 3, 1, 2), ref)
        print(f"conv3x3 b={b} {h}x{w} cin={cin} stride={stride} pad={pad} cout={cout} conv_skip={skip}: rel err {err:.3g}")
        assert err < BOUND, (skip, err)                                                                # (i)
    assert torch.equal(outs[0], outs[1])                                                               # (ii)
    if (h, w, stride, pad) == (16, 16, (2, 2), 3):                                                     # (iv)
        # output row 0 and column 0 see only padding: exactly LeakyReLU(bias), 19 positions
        o = outs[1]
        edge = torch.cat([o[:, 0, :, :], o[:, 1:, 0, :]], 1)
        assert edge.shape[1] == 19
        assert torch.equal(edge, F.leaky_relu(bias, 0.01).expand_as(edge))
