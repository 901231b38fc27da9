"""Seeded frames, records and numpy expectations for the two operators of csrc/clip_ops.hip (casync_op_clip_gather,
casync_op_clip_compose).  The reference is numpy slicing; every comparison is exact: the error is the number of differing
bytes of the whole output buffer, the gaps between regions included, and inf where a fence around it changed.  Nothing here
touches a GPU at import."""
import ctypes
import functools

import numpy as np

N_FRAMES = 3
# (1,1); two sizes whose H*W*3 is no multiple of 16 (105, 3069) and two whose is (768, 9216)
SIZES = [(1, 1), (5, 7), (33, 31), (16, 16), (64, 48)]
REAL = (1080, 1920)
FILL = 0x5A
FENCE = 64              # bytes before and after an output


def _boxes(H, W):
    """(frame, y0, x0, h, w, valid) of one batch: invalid records first and last, the whole frame, the two corner pixels, the
    last column, the last row, an interior box with odd x0 and odd w; frame 1 three times with different boxes, frames
    descending (2, 1 and 1, 0)."""
    if (H, W) == (1, 1):
        return [(0, 0, 0, 1, 1, 0), (2, 0, 0, 1, 1, 1), (1, 0, 0, 1, 1, 1), (0, 0, 0, 1, 1, 0)]
    if (H, W) == REAL:
        return [(1, 233, 611, 700, 700, 1), (0, 5, 7, 3, 2, 0)]
    x0 = 1 if W < 16 else 5
    w = (W - x0 - 1) | 1
    if x0 + w > W - 1:
        w -= 2
    assert x0 % 2 == 1 and w % 2 == 1 and w >= 1 and x0 + w < W and H >= 3
    return [(0, 0, 0, H, W, 0),
            (2, 0, 0, H, W, 1),
            (1, 0, 0, 1, 1, 1),
            (1, H - 1, W - 1, 1, 1, 1),
            (2, 0, W - 1, H, 1, 1),
            (1, H - 1, 0, 1, W, 1),
            (0, 1, x0, H - 2, w, 1),
            (2, H - 1, 0, 1, 1, 0)]


class Case:
    """Inputs and expectations of one size, computed once and never changed."""

    def __init__(self, H, W, repeat):
        rng = np.random.default_rng([H, W, repeat])
        self.H, self.W = H, W
        n = 2 if (H, W) == REAL else N_FRAMES
        self.frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        boxes = _boxes(H, W) * repeat
        self.batch = len(boxes)
        self.rec = np.zeros((self.batch, 8), dtype=np.int32)
        off = 0
        for i, (f, y0, x0, h, w, valid) in enumerate(boxes):
            off += 1 + (7 * i) % 15                                   # a gap of 1..15 bytes before every region
            self.rec[i] = (f, y0, x0, h, w, valid, off, 0)
            off += h * w * 3
        self.regions_bytes = off + 3
        # gather: every record's box, whatever valid says
        self.want_regions = np.full(self.regions_bytes, FILL, dtype=np.uint8)
        for f, y0, x0, h, w, _, o, _ in self.rec:
            self.want_regions[o:o + h * w * 3] = self.frames[f, y0:y0 + h, x0:x0 + w].reshape(-1)
        # compose: the blended regions are other bytes than the frames'
        self.out_regions = rng.integers(0, 256, self.regions_bytes, dtype=np.uint8)
        self.want_out = np.stack([self.frames[r[0]] for r in self.rec])
        for b, (f, y0, x0, h, w, valid, o, _) in enumerate(self.rec):
            if valid:
                self.want_out[b, y0:y0 + h, x0:x0 + w] = self.out_regions[o:o + h * w * 3].reshape(h, w, 3)
        self.rec_plain = self.rec.copy()                              # no valid record: the plain fetch (out_regions NULL)
        self.rec_plain[:, 5] = 0
        self.want_plain = np.stack([self.frames[r[0]] for r in self.rec])
        for a in (self.frames, self.rec, self.rec_plain, self.want_regions, self.out_regions, self.want_out, self.want_plain):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(H, W, repeat=1):
    return Case(H, W, repeat)


@functools.lru_cache(maxsize=None)
def _device_frames(H, W, repeat):
    import torch
    return torch.from_numpy(case(H, W, repeat).frames.copy()).to("cuda:0")


def _fenced(nbytes):
    import torch
    buf = torch.full((nbytes + 2 * FENCE,), FILL, dtype=torch.uint8, device="cuda:0")
    return buf, buf[FENCE:FENCE + nbytes]


def _differences(buf, nbytes, want):
    """bytes of the output that differ from the expectation; inf if a fence changed"""
    got = buf.cpu().numpy()
    if (got[:FENCE] != FILL).any() or (got[FENCE + nbytes:] != FILL).any():
        return float("inf")
    return float(np.count_nonzero(got[FENCE:FENCE + nbytes] != want.reshape(-1)))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def run_gather(H, W, repeat=1):
    """-> the number of differing bytes of `regions` (gaps and fences included)"""
    import torch
    from calipsync_amd import _lib
    c = case(H, W, repeat)
    frames = _device_frames(H, W, repeat)
    buf, mid = _fenced(c.regions_bytes)
    rec = np.ascontiguousarray(c.rec)
    _lib.check(_lib.load().casync_op_clip_gather(frames.data_ptr(), frames.shape[0], H, W, rec.ctypes.data, c.batch, mid.data_ptr(),
                                                 c.regions_bytes, _stream()), "casync_op_clip_gather")
    torch.cuda.synchronize()
    return _differences(buf, c.regions_bytes, c.want_regions)


def run_compose(H, W, repeat=1, plain=False):
    """-> the number of differing bytes of `out`; plain: no valid record and out_regions NULL"""
    import torch
    from calipsync_amd import _lib
    c = case(H, W, repeat)
    frames = _device_frames(H, W, repeat)
    nbytes = c.batch * H * W * 3
    buf, mid = _fenced(nbytes)
    rec = np.ascontiguousarray(c.rec_plain if plain else c.rec)
    regions = None if plain else torch.from_numpy(c.out_regions.copy()).to("cuda:0")
    _lib.check(_lib.load().casync_op_clip_compose(frames.data_ptr(), frames.shape[0], H, W, rec.ctypes.data, c.batch,
                                                  None if plain else regions.data_ptr(), 0 if plain else c.regions_bytes, mid.data_ptr(),
                                                  _stream()), "casync_op_clip_compose")
    torch.cuda.synchronize()
    return _differences(buf, nbytes, c.want_plain if plain else c.want_out)


def host_buffer(nbytes=4096):
    """a host buffer standing in for device pointers in the argument checks: a refused call never touches it"""
    buf = (ctypes.c_uint8 * nbytes)()
    ctypes.memset(buf, FILL, nbytes)
    return buf
