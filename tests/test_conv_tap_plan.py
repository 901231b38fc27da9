"""What the dense 3x3 conv walks (casync_conv3x3_plan, host only): its GEMM rows are position-major -- output positions sorted by
(valid-tap mask, position), frames innermost -- and a 64-row tile walks the union of its rows' taps.  The count here is made
independently in numpy from that definition."""
import ctypes as C

import numpy as np
import pytest

from calipsync_amd import _lib

BM = 64                          # rows of an M-tile (the 64x64 ring tile every case here takes)
CONV5 = (16, 16, 2, 2, 3)        # h, w, stride_h, stride_w, pad: 16x16 -> 10x10
CONV3 = (32, 32, 2, 2, 1)        # 32x32 -> 16x16


def masks(h, w, sh, sw, pad):
    """valid-tap mask (bit ky * 3 + kx) of every output position, row-major"""
    ho, wo = (h + 2 * pad - 3) // sh + 1, (w + 2 * pad - 3) // sw + 1
    oy, ox = np.divmod(np.arange(ho * wo), wo)
    m = np.zeros(ho * wo, dtype=np.int64)
    for t in range(9):
        iy, ix = oy * sh - pad + t // 3, ox * sw - pad + t % 3
        m |= ((iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)).astype(np.int64) << t
    return m


def popcount(x):
    return bin(int(x)).count("1")


def numpy_share(batch, geom):
    m = np.sort(masks(*geom), kind="stable")                # (mask, position) order
    rows = np.repeat(m, batch)                              # frame innermost
    tiles = [rows[i:i + BM] for i in range(0, len(rows), BM)]
    return sum(popcount(np.bitwise_or.reduce(t)) for t in tiles), 9 * len(tiles)


def exact_share(geom):
    m = masks(*geom)
    return sum(popcount(x) for x in m) / (9.0 * len(m))


def plan(batch, geom, cin, cout):
    h, w, sh, sw, pad = geom
    full, run = C.c_int64(), C.c_int64()
    _lib.check(_lib.load().casync_conv3x3_plan(batch, h, w, cin, cout, sh, sw, pad, C.byref(full), C.byref(run)), "casync_conv3x3_plan")
    return run.value, full.value


def test_conv5_exact_share_is_64_percent():
    m = masks(*CONV5)
    assert exact_share(CONV5) == pytest.approx(0.64)
    assert int((m == 0).sum()) == 19                        # output row 0 and column 0 read only padding


@pytest.mark.parametrize("batch", [1, 2, 8, 31, 32, 33, 64])
def test_conv5_plan_matches_numpy(batch):
    n_nt = 512 // 64
    run, full = plan(batch, CONV5, 256, 512)
    want_run, want_full = numpy_share(batch, CONV5)
    assert (run, full) == (want_run * n_nt, want_full * n_nt)
    assert run / full >= exact_share(CONV5) - 1e-12         # never below what the image needs
    if batch == 32:
        assert run / full <= 0.66


def test_conv3_plan():
    for batch in (3, 32):
        run, full = plan(batch, CONV3, 128, 256)
        want_run, want_full = numpy_share(batch, CONV3)
        assert run * want_full == want_run * full
        assert run / full >= 0.95


def test_pad0_has_nothing_to_skip():
    run, full = plan(1, (7, 5, 1, 1, 0), 32, 128)
    assert run == full > 0


def test_conv_skip_off_walks_all_nine():
    old = _lib.get_option("conv_skip")
    _lib.set_option("conv_skip", 0)
    try:
        run, full = plan(32, CONV5, 256, 512)
    finally:
        _lib.set_option("conv_skip", old)
    assert run == full


def test_plan_rejects_bad_geometry():
    full, run = C.c_int64(), C.c_int64()
    lib = _lib.load()
    assert lib.casync_conv3x3_plan(1, 1, 1, 32, 64, 1, 1, 0, C.byref(full), C.byref(run)) != 0     # no 3x3 window fits
    assert lib.casync_conv3x3_plan(1, 16, 16, 30, 64, 1, 1, 1, C.byref(full), C.byref(run)) != 0   # cin not a k-tile multiple
