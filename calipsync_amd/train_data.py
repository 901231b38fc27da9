"""The trainer's batches, built on the device from a clip that is resident there (csrc/train_ops.hip).

The reference's ``MyDataset.__getitem__`` (dataset/dataset.py:136-178) reads two full frames and two landmark files per sample,
resizes two crops and slices an audio window, in DataLoader workers, for every sample of every epoch.  Here the clip is decoded
ONCE (``ResidentClip``), its dataset boxes are computed ONCE, and a batch is one kernel over the stored frames plus the window
gather the inference path already has:

    clip = clip_from_dataset_dir(dataset_dir)                       # full_body_img/{i}.jpg + landmarks/{i}.lms
    loader = TrainingBatches(clip, np.load(dataset_dir + "/aud_hu.npy"), batch_size=16)
    for img_concat, img_real, audio_feat in loader:                 # float32, on the device
        ...

which replaces ``DataLoader(MyDataset(dataset_dir, "hubert"), batch_size=16, shuffle=True, num_workers=4)`` in the reference's
training loop (its ``.cuda()`` calls become no-ops).  The training loop itself stays torch.  There is no fallback: without the
library's kernel a batch raises."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, frame_loop
from .resident_clip import UPLOAD_CHUNK, ResidentClip, _Chunks

REC_WORDS = 12           # t, y0, x0, h, w, r, ry0, rx0, rh, rw, 0, 0  (include/casync_train.h)


# ---------------------------------------------------------------------------------------------------------------
# host rules (dataset/dataset.py:39-56, 73-89, 136-146)
# ---------------------------------------------------------------------------------------------------------------
def read_lms(path: str) -> np.ndarray:
    """One ``.lms`` file as the reference parses it (dataset.py:75-82): every line split at single spaces, the words taken as
    float32, the whole cast to int32 (towards zero) -> [n_points, 2] int32.  ``np.savetxt(fmt='%d')`` files and float text alike."""
    with open(path, "r") as f:
        rows = [np.array(line.split(" "), dtype=np.float32) for line in f.read().splitlines()]
    return np.array(rows, dtype=np.int32)


def dataset_crop_box(lms, height: int, width: int) -> Optional[Tuple[int, int, int, int]]:
    """The region ``img[ymin:ymax, xmin:xmax]`` of dataset.py:83-90 as (y0, x0, h, w), cut to the ``height`` x ``width`` frame
    the way numpy slicing cuts it; None where the frame is unusable (a negative start wraps around in numpy, an empty region
    fails inside cv2.resize).  ``lms`` float landmarks go through float32 to int32 like the file's text; there are NO clamps or
    shifts (``frame_loop.crop_box``, the inference rule, has both): a square that runs past the bottom or the right edge is
    cut there, and the non-square region is resized to 168 x 168 like any other."""
    l = np.asarray(lms)
    if l.dtype.kind == "f":
        l = l.astype(np.float32)
    l = l.astype(np.int32)
    xmin, ymin, xmax = int(l[1][0]), int(l[52][1]), int(l[31][0])
    side = xmax - xmin
    if xmin < 0 or ymin < 0 or side < 1 or xmin >= int(width) or ymin >= int(height):
        return None
    return ymin, xmin, min(ymin + side, int(height)) - ymin, min(xmax, int(width)) - xmin


def window_rows(n_steps: int, idx: int) -> int:
    """Rows of ``MyDataset.get_audio_features(features, idx)`` for ``n_steps`` feature steps (dataset.py:39-56): 16 wherever the
    reference's ``reshape(32, 32, 32)`` works.  The pads are ``zeros_like`` of a slice of what is there, so they are short
    where the clip is (the closed form of ``frame_loop.audio_windows_host``)."""
    left0, right0 = idx - 8, idx + 8
    pad_left, pad_right = max(0, -left0), max(0, right0 - n_steps)
    left, right = max(left0, 0), min(right0, n_steps)
    n0 = max(0, min(right, n_steps) - min(left, n_steps))
    pl = min(pad_left, n0)
    return n0 + pl + min(pad_right, n0 + pl)


class TrainSampler:
    """Which items make up the batches of an epoch (host only).  ``n_items = T - 1`` items (dataset.py:37); item ``idx`` shows
    frame ``t = min(idx, n_img - 1)`` (:137) against the reference item ``ex``, uniform over ``range(n_items)`` without ``t``
    (:142-143; the reference excludes the index it has just clamped), shown as frame ``min(ex, n_img - 1)`` (:144).

    The ORDER is this class's own: each epoch is a new permutation (``shuffle``) and a new draw of ``ex`` from
    ``numpy.random.default_rng(seed)``, so the same seed gives the same epochs.  The reference's order depends on the global
    RNG state of torch and numpy across its worker processes and is not reproducible."""

    def __init__(self, n_img: int, n_items: int, batch_size: int = 16, shuffle: bool = True, drop_last: bool = False, seed=None):
        if n_img < 1:
            raise ValueError("TrainSampler: no frames")
        if n_items < 2:
            raise ValueError(f"TrainSampler: {n_items} item(s); a reference frame needs a second one (T - 1 >= 2)")
        if int(batch_size) < 1:
            raise ValueError(f"TrainSampler: batch_size {batch_size}")
        self.n_img, self.n_items, self.batch_size = int(n_img), int(n_items), int(batch_size)
        self.shuffle, self.drop_last = bool(shuffle), bool(drop_last)
        self._rng = np.random.default_rng(seed)

    def __len__(self) -> int:
        full, rest = divmod(self.n_items, self.batch_size)
        return full if self.drop_last or not rest else full + 1

    def frame_of(self, items) -> np.ndarray:
        return np.minimum(np.asarray(items, dtype=np.int64), self.n_img - 1)

    def epoch(self):
        """[(items, reference items)] of one epoch, int64 arrays per batch"""
        order = self._rng.permutation(self.n_items) if self.shuffle else np.arange(self.n_items)
        k = self._rng.integers(0, self.n_items - 1, size=self.n_items)
        ex = k + (k >= self.frame_of(order))                     # uniform over range(n_items) without t
        stop = len(self) * self.batch_size
        return [(order[i:i + self.batch_size], ex[i:i + self.batch_size]) for i in range(0, min(stop, self.n_items), self.batch_size)]


# ---------------------------------------------------------------------------------------------------------------
# the device call
# ---------------------------------------------------------------------------------------------------------------
def train_batch(frames_dev: torch.Tensor, records) -> Tuple[torch.Tensor, torch.Tensor]:
    """``casync_op_train_batch``: ``frames_dev`` uint8 [N,H,W,3] on a ROCm device (a clip's store), ``records`` [B,12] int32 on
    the host = {t, y0, x0, h, w, r, ry0, rx0, rh, rw, 0, 0}, the boxes ``dataset_crop_box``'s -> (img_concat [B,6,160,160],
    img_real [B,3,160,160]) float32 on the device.  On torch's current stream, from torch's allocator, no synchronisation."""
    if not isinstance(frames_dev, torch.Tensor) or frames_dev.dtype != torch.uint8 or frames_dev.dim() != 4 or frames_dev.shape[3] != 3:
        raise RuntimeError("train_batch: frames must be a uint8 [N,H,W,3] tensor")
    if frames_dev.device.type != "cuda":
        raise RuntimeError("train_batch: frames must be on a ROCm device (no CPU fallback)")
    if not frames_dev.is_contiguous():
        raise RuntimeError("train_batch: frames must be contiguous")
    rec = np.ascontiguousarray(records, dtype=np.int32)
    if rec.ndim != 2 or rec.shape[1] != REC_WORDS:
        raise ValueError(f"train_batch: records {rec.shape}, expected [B,{REC_WORDS}]")
    dev, b = frames_dev.device, rec.shape[0]
    n, h, w = (int(v) for v in frames_dev.shape[:3])
    with torch.cuda.device(dev):
        img_concat = torch.empty((b, 6, 160, 160), dtype=torch.float32, device=dev)
        img_real = torch.empty((b, 3, 160, 160), dtype=torch.float32, device=dev)
        if b:
            _lib.check(_lib.load().casync_op_train_batch(frames_dev.data_ptr(), n, h, w, rec.ctypes.data, b, img_concat.data_ptr(),
                                                         img_real.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                       "casync_op_train_batch")                 # the records are read before the call returns
    return img_concat, img_real


def clip_from_dataset_dir(dataset_dir: str, device="cuda:0", decode: str = "host", io_workers: int = 8) -> ResidentClip:
    """What the reference's data preparation writes, ``full_body_img/{i}.jpg`` and ``landmarks/{i}.lms`` for i = 0 .. n-1
    (dataset.py:20-25), as a clip on the device, every file read once with the loaders of ``ResidentClip.from_data_dir``.
    ``decode="device"``: the files go up as bytes and ``jpeg.decode_jpeg_device`` decodes them into the clip's storage; the
    frames are the same bytes as with ``"host"`` wherever the host decoder is libjpeg's default path."""
    from .frame_synth import _imread
    if decode not in ("host", "device"):
        raise ValueError(f"clip_from_dataset_dir: decode {decode!r} is neither 'host' nor 'device'")
    img_dir, lms_dir = os.path.join(dataset_dir, "full_body_img"), os.path.join(dataset_dir, "landmarks")
    n = len(os.listdir(img_dir))                                   # as the reference counts (dataset.py:20)
    if n < 1:
        raise ValueError(f"clip_from_dataset_dir: no frames in {img_dir}")
    landmarks = [None] * n

    def load(i):
        path = os.path.join(img_dir, f"{i}.jpg")
        if decode == "device":
            with open(path, "rb") as f:
                img = f.read()
        else:
            img = _imread(path)
            if img is None:
                raise ValueError(f"clip_from_dataset_dir: cannot read {path}")
        landmarks[i] = read_lms(os.path.join(lms_dir, f"{i}.lms"))
        return img

    with ThreadPoolExecutor(max_workers=max(1, int(io_workers))) as pool:
        chunks = (list(pool.map(load, range(i, min(i + UPLOAD_CHUNK, n)))) for i in range(0, n, UPLOAD_CHUNK))
        if decode == "device":
            return ResidentClip(ResidentClip._decode_chunks(n, chunks, torch.device(device), img_dir), landmarks, None, device)
        return ResidentClip(_Chunks(n, chunks), landmarks, None, device)


class TrainingBatches:
    """The reference's ``DataLoader(MyDataset(dir, "hubert"), batch_size, shuffle, drop_last)`` over a resident clip: iterating
    yields ``(img_concat [B,6,160,160], img_real [B,3,160,160], audio_feat [B,32,32,32])``, float32, on the clip's device, on
    torch's current stream and without a synchronisation.  ``features``: the clip's ``aud_hu.npy``, [T,2,1024] as a numpy array
    or a float32 device tensor, uploaded once.  ``len()`` is the DataLoader's for ``T - 1`` items.

    The order of the samples is ``TrainSampler``'s, this class's own: a new permutation and a new draw of reference frames per
    epoch from ``numpy.random.default_rng(seed)``.  The reference's order depends on global RNG state across worker processes
    and is not reproducible; what a sample IS (frames, boxes, pixels, window) is the reference's.

    ValueError at construction, before anything is sent to the device: a frame the epoch reaches whose box is unusable
    (``dataset_crop_box``), an item whose audio window has fewer than 16 rows (the reference's ``reshape`` raises), fewer than
    two items, a clip that dropped frames (``from_frames`` / ``from_video`` without a face somewhere: the audio rows would no
    longer line up with the stored frames).  ``mode="wenet"`` raises NotImplementedError."""

    def __init__(self, clip: ResidentClip, features, batch_size: int = 16, shuffle: bool = True, drop_last: bool = False, seed=None,
                 mode: str = "hubert"):
        if mode == "wenet":
            raise NotImplementedError("TrainingBatches: mode='wenet' windows ([256,16,32]) are not built here")
        if mode != "hubert":
            raise ValueError(f"TrainingBatches: mode {mode!r}")
        shape = tuple(features.shape)
        if len(shape) != 3 or shape[1:] != (2, 1024):
            raise ValueError(f"TrainingBatches: features {shape}, expected [T,2,1024]")
        n_img, steps = len(clip), shape[0]
        kept = clip.source_index
        if kept is not None and [int(i) for i in kept] != list(range(n_img)):
            raise ValueError("TrainingBatches: the clip dropped frames (source_index is not 0 .. n-1): feature row i would no longer "
                             "belong to stored frame i")
        self.sampler = TrainSampler(n_img, steps - 1, batch_size, shuffle, drop_last, seed)
        reach = min(steps - 1, n_img)                              # frames min(idx, n_img - 1) of idx in range(T - 1)
        boxes = [dataset_crop_box(clip.landmarks[i], clip.H, clip.W) for i in range(reach)]
        bad = [i for i, b in enumerate(boxes) if b is None]
        if bad:
            raise ValueError(f"TrainingBatches: no usable region (xmin, ymin >= 0 inside the {clip.H} x {clip.W} frame, width >= 1) in "
                             f"frame(s) {bad[:20]}{' ...' if len(bad) > 20 else ''}")
        short = [i for i in range(reach) if window_rows(steps, i) != 16]
        if short:
            raise ValueError(f"TrainingBatches: the audio window of item(s) {short[:20]}{' ...' if len(short) > 20 else ''} has fewer "
                             f"than 16 rows with {steps} feature steps")
        self.clip, self.steps = clip, steps
        self.boxes = np.asarray(boxes, dtype=np.int32).reshape(reach, 4)
        self._inflight: list = []                                  # (event, pinned index block) the GPU may still be reading
        if isinstance(features, torch.Tensor):
            if features.dtype != torch.float32:
                raise ValueError(f"TrainingBatches: features {features.dtype}, expected float32")
            self.features = features.to(clip.device).contiguous()
        else:
            self.features = torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32)).to(clip.device)

    def __len__(self) -> int:
        return len(self.sampler)

    def __iter__(self):
        for items, refs in self.sampler.epoch():
            yield self.batch_for(items, refs)

    def _reap(self) -> None:
        busy = []
        for done, block in self._inflight:
            if done.query():
                frame_loop._release_pinned(block)
            else:
                busy.append((done, block))
        self._inflight = busy

    def batch_for(self, indices, ref_indices):
        """One batch from given items and reference items (both in ``range(T - 1)``, equally many): item ``idx`` shows frame
        ``t = min(idx, n_img - 1)`` and the audio window at ``t`` (the reference clamps ``idx`` itself, dataset.py:137, before
        it takes the window at :172), its reference item ``ex`` frame ``min(ex, n_img - 1)``."""
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        ex = np.asarray(list(ref_indices), dtype=np.int64).reshape(-1)
        if idx.shape != ex.shape:
            raise ValueError(f"TrainingBatches.batch_for: {idx.size} items, {ex.size} reference items")
        n_items = self.sampler.n_items
        if idx.size and (min(idx.min(), ex.min()) < 0 or max(idx.max(), ex.max()) >= n_items):
            raise IndexError(f"TrainingBatches.batch_for: items outside [0, {n_items})")
        if self.clip.frames is None:
            raise RuntimeError("TrainingBatches: the clip is closed")
        t, r = self.sampler.frame_of(idx), self.sampler.frame_of(ex)
        rec = np.zeros((idx.size, REC_WORDS), dtype=np.int32)
        rec[:, 0], rec[:, 1:5], rec[:, 5], rec[:, 6:10] = t, self.boxes[t], r, self.boxes[r]
        dev = self.clip.device
        img_concat, img_real = train_batch(self.clip.frames, rec)
        if not idx.size:
            return img_concat, img_real, torch.empty((0, 32, 32, 32), dtype=torch.float32, device=dev)
        self._reap()
        stage = frame_loop._acquire_pinned(4 * idx.size)           # the window indices go up without a wait
        try:
            stage.numpy()[:4 * idx.size] = t.astype(np.int32).view(np.uint8)
            with torch.cuda.device(dev):
                idx_dev = torch.empty(idx.size, dtype=torch.int32, device=dev)
                idx_dev.view(torch.uint8).copy_(stage[:4 * idx.size], non_blocking=True)
                audio_feat = frame_loop.audio_windows_device(self.features, idx_dev)
                done = torch.cuda.Event()
                done.record(torch.cuda.current_stream(dev))
        except Exception:
            torch.cuda.synchronize(dev)
            frame_loop._release_pinned(stage)
            raise
        self._inflight.append((done, stage))
        return img_concat, img_real, audio_feat
