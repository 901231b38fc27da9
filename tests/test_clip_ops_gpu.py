"""-m gpu: the two clip operators where a frame's base lies beyond 2^31 and 2^32 bytes.  frames is 22 x 8192 x 8192 x 3 uint8
(4.4 GB, uninitialised but for the three frames used): frame 11 starts at 2.2e9 bytes (> 2^31); frame 21 starts at 4.23e9 and
its rows from 2731 on lie beyond 2^32, so its box starts at row 3000.  compose also writes 22 output frames, so that the base of
out[b] passes both marks.  Everything is compared on the device with torch indexing; nothing of this size is downloaded."""
import numpy as np
import pytest
import torch

from calipsync_amd import _lib

pytestmark = pytest.mark.gpu

N, SIDE = 22, 8192
FRAME = SIDE * SIDE * 3
USED = (0, 11, 21)
BOXES = [(21, 3000, 1001, 701, 333, 1), (11, 5, 7, 600, 601, 1), (0, 8000, 8000, 192, 192, 1)]      # frame, y0, x0, h, w, valid


@pytest.fixture(scope="module")
def frames():
    assert 11 * FRAME > 2 ** 31 and 21 * FRAME + 3000 * SIDE * 3 > 2 ** 32 and N * FRAME < 2 ** 33
    f = torch.empty((N, SIDE, SIDE, 3), dtype=torch.uint8, device="cuda:0")
    g = torch.Generator(device="cuda:0")
    g.manual_seed(2231)
    for i in USED:
        f[i] = torch.randint(0, 256, (SIDE, SIDE, 3), dtype=torch.uint8, device="cuda:0", generator=g)
    torch.cuda.synchronize()
    assert not torch.equal(f[0, :64], f[11, :64]) and not torch.equal(f[11, :64], f[21, :64])
    yield f
    del f
    torch.cuda.empty_cache()


def _records():
    rec = np.zeros((len(BOXES), 8), dtype=np.int32)
    off = 0
    for i, (f, y0, x0, h, w, valid) in enumerate(BOXES):
        off += 3 + 5 * i
        rec[i] = (f, y0, x0, h, w, valid, off, 0)
        off += h * w * 3
    return rec, off + 9


def test_gather_reads_frames_beyond_2_31_and_2_32_bytes(frames):
    rec, nbytes = _records()
    regions = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda:0")
    _lib.check(_lib.load().casync_op_clip_gather(frames.data_ptr(), N, SIDE, SIDE, rec.ctypes.data, len(rec), regions.data_ptr(), nbytes,
                                                 torch.cuda.current_stream().cuda_stream), "casync_op_clip_gather")
    want = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda:0")
    for f, y0, x0, h, w, _, off, _ in rec.tolist():
        want[off:off + h * w * 3] = frames[f, y0:y0 + h, x0:x0 + w].reshape(-1)
    differing = int((regions != want).sum())
    print(f"gather of frames {[r[0] for r in BOXES]}: {differing} of {nbytes} bytes differ")
    assert differing == 0


def test_compose_reads_and_writes_beyond_2_31_and_2_32_bytes(frames):
    rec, nbytes = _records()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(77)
    out_regions = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda:0", generator=g)
    out = torch.empty((3, SIDE, SIDE, 3), dtype=torch.uint8, device="cuda:0")
    lib = _lib.load()
    _lib.check(lib.casync_op_clip_compose(frames.data_ptr(), N, SIDE, SIDE, rec.ctypes.data, len(rec), out_regions.data_ptr(), nbytes,
                                          out.data_ptr(), torch.cuda.current_stream().cuda_stream), "casync_op_clip_compose")
    for b, (f, y0, x0, h, w, _, off, _) in enumerate(rec.tolist()):
        want = frames[f].clone()
        want[y0:y0 + h, x0:x0 + w] = out_regions[off:off + h * w * 3].view(h, w, 3)
        differing = int((out[b] != want).sum())
        print(f"compose of frame {f}: {differing} of {FRAME} bytes differ")
        assert differing == 0
        assert not torch.equal(out[b, y0:y0 + h, x0:x0 + w], frames[f, y0:y0 + h, x0:x0 + w])
        del want
    del out
    # the plain fetch of 22 frames: out[11] starts beyond 2^31, out[21] runs beyond 2^32
    order = [0] * N
    order[11], order[21], order[10], order[20] = 21, 11, 11, 21
    plain = np.zeros((N, 8), dtype=np.int32)
    plain[:, 0] = order
    out = torch.empty((N, SIDE, SIDE, 3), dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.casync_op_clip_compose(frames.data_ptr(), N, SIDE, SIDE, plain.ctypes.data, N, None, 0, out.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "casync_op_clip_compose")
    for b in (0, 10, 11, 12, 20, 21):
        assert torch.equal(out[b], frames[order[b]]), b
    del out
    torch.cuda.empty_cache()
