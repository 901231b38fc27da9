"""-m gpu: the fp32 expand + depthwise kernels (pw_dw.hip) give the BITS of the commit recorded in tests/golden/pw_dw_bits.json.

The file holds, per case, the SHA-256 of the output bytes and the name of the kernel that ran, written by
tools/record_pw_dw_bits.py from a library built from the commit BEFORE the index arithmetic of the epilogues was reworked
(`parent_commit` in the file).  That rework may only change how indices, addresses and constant taps are obtained: no
floating-point operation may change, move or re-associate, so every case has to reproduce the recorded hash.  The hashes are
that commit's, never the head's: a mismatch means the head is wrong.

Every case goes through casync_op_pw_dw (one through casync_op_pw_dw_rect) with operands that are column slices of wider
buffers (lda > cin, ldd > cexp, ld_ups > cexp, non-zero column offsets -- the A and D address paths are what the rework
touches), the output prefilled with NaN, and also holds the float64 bound of test_pw_dw_fused (3e-6 of the largest output)."""
import contextlib
import hashlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

from calipsync_amd import _lib
from gpu_util import dev, launched, ok, options, stream

pytestmark = pytest.mark.gpu

BOUND = 3e-6   # test_pw_dw_fused / test_up_block_expand_with_commuted_upsample
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pw_dw_bits.json")

# id: (h, w, stride, frames, cin, cexp, options, upsampled addend, the instance that must run)
# cexp = 64: two 32-channel tiles.  The 10x10 pair kernel with 3 frames: the last pair holds one frame, its shared pixel tile is
# wholly invalid; 40x40 whole frames: every strip, the zero rows above and below the frame included.
CASES = {
    "10_pair_3f_streamk1": (10, 10, 1, 3, 64, 64, dict(fuse_dw_deep=0, gemm_streamk=1), False, "pw_dw_kernel<10, 2, 32, 16, 1, 2>"),
    "10_pair_3f_streamk0": (10, 10, 1, 3, 64, 64, dict(fuse_dw_deep=0, gemm_streamk=0), False, "pw_dw_kernel<10, 2, 32, 16, 1, 2>"),
    "10_pair_12f": (10, 10, 1, 12, 32, 64, {}, False, "pw_dw_kernel<10, 2, 32, 16, 1, 2>"),
    "10_deep_2f": (10, 10, 1, 2, 64, 64, dict(fuse_dw_deep=100), False, "pw_dw_kernel<10, 1, 32, 32, 1, 4>"),
    "16_1f": (16, 16, 1, 1, 32, 64, {}, False, "pw_dw_kernel<16, 1, 32, 16, 1, 2>"),
    "16_deep_3f": (16, 16, 1, 3, 64, 64, dict(fuse_dw_deep=100), False, "pw_dw_kernel<16, 1, 32, 32, 1, 3>"),
    "20_s1_2f": (20, 20, 1, 2, 64, 64, {}, False, "pw_dw_kernel<20, 1, 32, 16, 1, 2>"),
    "20_s2_2f": (20, 20, 2, 2, 32, 64, {}, False, "pw_dw_kernel<20, 1, 32, 16, 2, 2>"),
    "20_ups_3f": (20, 20, 1, 3, 32, 64, {}, True, "pw_dw_kernel<20, 1, 32, 16, 1, 2>"),
    "40_s1_2f": (40, 40, 1, 2, 32, 64, {}, False, "pw_dw_strip_kernel<40, 8, 1, 32, 16>"),
    "40_s2_1f": (40, 40, 2, 1, 64, 64, {}, False, "pw_dw_strip_kernel<40, 4, 2, 32, 16>"),
    "40_ups_1f": (40, 40, 1, 1, 32, 64, {}, True, "pw_dw_strip_kernel<40, 8, 1, 32, 16>"),
    "rect_16x32_1f": (16, 32, 1, 1, 256, 64, {}, False, "pw_dw_rect_kernel<16, 32, 32, 16>"),
}


def rel_err(got, ref):
    return float((got - ref).abs().max() / max(1e-6, float(ref.abs().max())))


def run_case(lib, name):
    """One launch of case `name` -> (the [frames, ho, wo, cexp] output slice on the CPU, the float64 reference in the same
    layout, the set of kernels that ran).  Asserts that nothing outside the output slice was written."""
    h, w, stride, frames, cin, cexp, opts, ups, _ = CASES[name]
    g = torch.Generator().manual_seed(sum(name.encode()) * 131 + frames)
    x = torch.randn(frames, cin, h, w, generator=g)
    w1 = torch.randn(cexp, cin, generator=g) / cin ** 0.5
    b1 = torch.randn(cexp, generator=g) * 0.3
    wd = torch.randn(cexp, 1, 3, 3, generator=g) / 3
    bd = torch.randn(cexp, generator=g) * 0.3
    g_lo = torch.randn(frames, cexp, h // 2, w // 2, generator=g) if ups else None
    pre = F.conv2d(x.double(), w1.double()[:, :, None, None], b1.double())
    if ups:
        pre = pre + F.interpolate(g_lo.double(), scale_factor=2, mode="bilinear", align_corners=True)
    ref = F.leaky_relu(F.conv2d(F.leaky_relu(pre, 0.01), wd.double(), bd.double(), stride, 1, 1, cexp), 0.01).float()
    ho, wo = ref.shape[2], ref.shape[3]
    lda, ldd, ldg = cin + 32, cexp + 16, cexp + 48
    xin = torch.full((frames, h, w, lda), 5.0)
    xin[..., 32:] = x.permute(0, 2, 3, 1)
    xin = xin.to(dev())
    gin = None
    if ups:
        gin = torch.full((frames, h // 2, w // 2, ldg), 9.0)
        gin[..., 16:16 + cexp] = g_lo.permute(0, 2, 3, 1)
        gin = gin.to(dev())
    out = torch.full((frames, ho, wo, ldd), float("nan"), device=dev())
    wdp = wd.reshape(cexp, 9).T.contiguous().to(dev())          # tap-major [9][C]
    w1d, b1d, bdd = w1.to(dev()), b1.to(dev()), bd.to(dev())
    with contextlib.ExitStack() as stack:
        if opts:
            stack.enter_context(options(**opts))
        names = stack.enter_context(launched())
        if h != w:
            ok(lib.casync_op_pw_dw_rect(xin.data_ptr() + 32 * 4, lda, w1d.data_ptr(), b1d.data_ptr(), wdp.data_ptr(), bdd.data_ptr(),
                                        out.data_ptr() + 16 * 4, ldd, frames, h, w, cin, cexp, stream()))
        else:
            ok(lib.casync_op_pw_dw(xin.data_ptr() + 32 * 4, lda, w1d.data_ptr(), b1d.data_ptr(), wdp.data_ptr(), bdd.data_ptr(),
                                   out.data_ptr() + 16 * 4, ldd, frames, h, stride, cin, cexp,
                                   gin.data_ptr() + 16 * 4 if ups else 0, ldg if ups else 0, stream()))
    o = out.cpu()
    assert torch.isnan(o[..., :16]).all(), "columns beside the output slice were written"
    return o[..., 16:].contiguous(), ref.permute(0, 2, 3, 1), names


def digest(t):
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_pw_dw_bits(lib, golden, name):
    got, ref, names = run_case(lib, name)
    assert not torch.isnan(got).any()
    err = rel_err(got, ref)
    print(f"pw_dw bits {name}: rel err {err:.3g}, kernels {sorted(names)}")
    assert err < BOUND, err
    want = golden["cases"][name]
    assert CASES[name][8] == want["kernel"]
    assert names == {want["kernel"]}, names
    assert digest(got) == want["sha256"], f"{name}: output bits differ from commit {golden['parent_commit'][:12]}"
