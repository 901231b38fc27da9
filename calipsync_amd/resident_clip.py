"""A clip resident on the device for the frame loop (csrc/clip_ops.hip).

``frame_loop.submit_batch_device`` pulls every frame of every batch through the host: it slices the crop regions into a
pinned buffer, copies each frame (the reference returns new frames) and pastes the blended regions back.  The ping-pong
walk revisits the same few hundred stored frames for as long as there is audio, so here the clip is uploaded ONCE, its
crop geometry is computed ONCE, and a batch sends a few KB of records up:

    clip = ResidentClip(frames, landmarks, masks)              # or .from_data_dir(...) / .from_frames(...)
    pending = clip.submit(net, indices, features=features_dev, frame_indices=[...])
    frames = pending.result()               # B new [H,W,3] uint8 arrays, ONE download
    frames_dev = pending.result_device()    # or the [B,H,W,3] uint8 device tensor, no download
    files = pending.result_jpeg(95)         # or B JPEG files encoded on the device (jpeg.py); submit with download=False

``casync_op_clip_gather`` cuts the crop boxes out of the resident frames into the packed ``regions`` layout,
``frame_loop.regions_through_net`` (the tail ``submit_batch_device`` runs too) blends them, ``casync_op_clip_compose``
writes whole frames: stored frame + blended box.  The pixels are those of the host-staged path byte for byte
(tests/test_resident_clip_gpu.py).  There is no fallback: a clip that does not fit raises."""
from __future__ import annotations

import os
import threading
import weakref
from concurrent.futures import ThreadPoolExecutor
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib, frame_loop

REC_WORDS = 8            # frame, y0, x0, h, w, valid, region byte offset, 0
UPLOAD_CHUNK = 64        # frames per pinned upload of a host clip
_CLIP_CAP = int(os.environ.get("CASYNC_RESIDENT_CLIP_MB", "16384")) << 20
# Page-locked bytes handed out as frames (PendingClipBatch.result) and not yet returned.  A consumer that holds every frame of
# a clip (VideoStreamManager.process_single_file) would otherwise pin the whole output: over the cap a batch is copied into
# pageable arrays and its block goes back at once.
_PINNED_VIEW_CAP = int(os.environ.get("CASYNC_RESIDENT_PINNED_MB", "2048")) << 20
_OUT_LOCK = threading.RLock()
_OUTSTANDING = 0


class ClipGeometry(NamedTuple):
    """Per stored frame: ``box`` [N,5] int64 = (ymin, ymax, xmin, xmax, width) of ``frame_loop.crop_box``, ``valid`` [N],
    ``pts`` [N,33,2] int32 (zeros where the box is empty), ``empty`` [N] bool."""
    box: np.ndarray
    valid: np.ndarray
    pts: np.ndarray
    empty: np.ndarray


def clip_geometry(landmarks: Sequence, H: int, W: int) -> ClipGeometry:
    """The host geometry of a clip's stored frames, once (``frame_loop.frame_geometry`` per frame: infer_api.py:206-231,
    281-289)."""
    n = len(landmarks)
    box = np.zeros((n, 5), dtype=np.int64)
    valid = np.zeros(n, dtype=np.int32)
    pts = np.zeros((n, 33, 2), dtype=np.int32)
    empty = np.zeros(n, dtype=bool)
    for i, lms in enumerate(landmarks):
        box[i], fp, valid[i] = frame_loop.frame_geometry(lms, H, W)
        if fp is None:
            empty[i] = True
        else:
            pts[i] = fp
    return ClipGeometry(box, valid, pts, empty)


def outstanding_pinned_bytes() -> int:
    """Page-locked bytes that live frames of ``PendingClipBatch.result`` still view (tests, diagnostics)."""
    with _OUT_LOCK:
        return _OUTSTANDING


def _returned(block, nbytes: int) -> None:
    global _OUTSTANDING
    with _OUT_LOCK:
        _OUTSTANDING -= nbytes
    frame_loop._release_pinned(block)


def _hand_out(block, batch: int, H: int, W: int) -> List[np.ndarray]:
    """``block``: a pinned uint8 buffer whose first batch * H * W * 3 bytes are the downloaded frames -> batch [H,W,3] arrays.
    Under the cap they are views of the block, which returns to ``frame_loop``'s pool when the last of them (or of their own
    views) is gone; over it they are pageable copies and the block returns now."""
    global _OUTSTANDING
    frame = H * W * 3
    arr = block.numpy()
    with _OUT_LOCK:
        pinned = _OUTSTANDING + block.numel() <= _PINNED_VIEW_CAP
        if pinned:
            _OUTSTANDING += block.numel()
    if not pinned:
        pool = frame_loop._host_pool()
        frames = [f.result() for f in [pool.submit(np.copy, arr[i * frame:(i + 1) * frame].reshape(H, W, 3)) for i in range(batch)]]
        frame_loop._release_pinned(block)
        return frames
    weakref.finalize(arr, _returned, block, block.numel())       # every view below has `arr` as its base
    return [arr[i * frame:(i + 1) * frame].reshape(H, W, 3) for i in range(batch)]


class PendingClipBatch:
    """A batch of ``ResidentClip.submit`` / ``fetch`` whose device work (and download, where one was asked for) is enqueued."""

    def __init__(self, out: torch.Tensor, host, done):
        self._out, self._host, self._done = out, host, done
        self._frames = None

    def result_device(self) -> torch.Tensor:
        """The finished frames [B,H,W,3] uint8 on the device, ordered on the stream they were submitted on; nothing is
        downloaded and nothing waits."""
        return self._out

    def _download(self) -> None:
        dev = self._out.device
        with torch.cuda.device(dev):
            self._host = frame_loop._acquire_pinned(max(self._out.numel(), 1))
            self._host[:self._out.numel()].copy_(self._out.view(-1), non_blocking=True)
            self._done = torch.cuda.Event()
            self._done.record(torch.cuda.current_stream(dev))

    def result(self) -> List[np.ndarray]:
        """B new [H,W,3] uint8 arrays after ONE download into a pinned block (see ``_hand_out`` for who owns it)."""
        if self._frames is None:
            if self._host is None:
                self._download()
            self._done.synchronize()
            b, h, w = self._out.shape[:3]
            host, self._host = self._host, None
            self._frames = _hand_out(host, b, h, w)
        return self._frames

    def result_jpeg(self, quality: int = 95, subsampling="4:4:4") -> List[bytes]:
        """The finished frames as B complete baseline JPEG files (4:4:4 and one restart interval per block row, or with
        ``subsampling="4:2:0"`` libjpeg's default chroma subsampling and one per MCU row), encoded on the device where
        ``result_device()`` lies (``jpeg.encode_jpeg_device``, on torch's current stream): what crosses to the host is the
        compressed bytes.  The raw download is not run; when this is the only result wanted, submit with ``download=False``."""
        from . import jpeg
        return jpeg.encode_jpeg_device(self._out, quality, subsampling=subsampling)


class _Chunks:
    """n equal-sized host frames that arrive in lists of at most UPLOAD_CHUNK (a directory being decoded)."""

    def __init__(self, n: int, chunks):
        self.n, self.chunks = n, chunks


def _mixed(shapes) -> ValueError:
    return ValueError(f"ResidentClip: needs uint8 frames of one size [H,W,3], got {sorted(set(shapes))}; frames of mixed sizes go "
                      "through frame_loop.submit_batch_device (FrameSynthesizer(resident=False))")


class ResidentClip:
    """The stored frames of a clip on the device (uint8 [N,H,W,3], BGR as stored), with their landmarks, crop geometry and
    masks.  ``frames``: equal-sized uint8 [H,W,3] arrays, or a uint8 [N,H,W,3] tensor (a device tensor is taken as it is);
    ``landmarks``: per frame [>=53, 2] (``np.loadtxt`` of a positions file, or int32); ``masks``: per frame None, uint8 or
    float32 of any 2-D size, each uploaded once to an allocation of its own."""

    def __init__(self, frames, landmarks, masks=None, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ResidentClip needs a ROCm device (no CPU fallback)")
        self.source_index = None
        self.audio, self.fps = None, None       # from_video: the file's PCM sound track (pcm, rate, width) and its frame rate
        self._inflight: list = []            # (event, pinned record block) of batches the GPU may still be reading
        if isinstance(frames, torch.Tensor) and (frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3):
            raise ValueError(f"ResidentClip: frames {tuple(frames.shape)} {frames.dtype}, expected uint8 [N,H,W,3]")
        if isinstance(frames, torch.Tensor) and not frames.is_cuda:
            frames = list(frames.numpy())                                 # a host tensor goes up like host frames
        if isinstance(frames, torch.Tensor):
            n, shape = int(frames.shape[0]), tuple(int(v) for v in frames.shape[1:])
            self._check_size(n, shape)
            self.frames = frames.to(self.device).contiguous()
        else:
            if not isinstance(frames, _Chunks):
                host = [np.asarray(f) for f in frames]
                frames = _Chunks(len(host), (host[i:i + UPLOAD_CHUNK] for i in range(0, len(host), UPLOAD_CHUNK)))
            self.frames = self._upload(frames)
        n, self.H, self.W = (int(v) for v in self.frames.shape[:3])
        if n < 1:
            raise ValueError("ResidentClip: no frames")
        landmarks = list(landmarks)
        if len(landmarks) != n:
            raise ValueError(f"ResidentClip: {n} frames, {len(landmarks)} landmark sets")
        self.landmarks = [np.asarray(l) for l in landmarks]
        if any(l.ndim != 2 or l.shape[0] < 53 or l.shape[1] != 2 for l in self.landmarks):
            raise ValueError("ResidentClip: landmarks must be [>=53, 2] per frame")
        self.geometry = clip_geometry(self.landmarks, self.H, self.W)
        box = self.geometry.box
        self._h, self._w = box[:, 1] - box[:, 0], box[:, 3] - box[:, 2]
        # geometry words 7..11 per stored frame: kind, height, width and device address of its mask
        self._mask_words = np.zeros((n, 5), dtype=np.int32)
        self._mask_words[:, 0] = -1
        self._masks: list = []
        masks = [None] * n if masks is None else list(masks)
        if len(masks) != n:
            raise ValueError(f"ResidentClip: {n} frames, {len(masks)} masks")
        with torch.cuda.device(self.device):
            for i, m in enumerate(masks):
                if m is None:
                    continue
                kind = frame_loop._mask_kind(m)
                d = torch.from_numpy(np.ascontiguousarray(m, dtype=np.uint8 if kind else np.float32)).to(self.device)
                self._masks.append(d)
                self._mask_words[i] = (kind, m.shape[0], m.shape[1]) + frame_loop._split64(d.data_ptr())

    # ------------------------------------------------------------------ construction
    @staticmethod
    def _check_size(n: int, shape) -> None:
        nbytes = n * int(np.prod(shape))
        if nbytes > _CLIP_CAP:
            raise ValueError(f"ResidentClip: {n} frames of {tuple(shape)} are {nbytes >> 20} MiB, above CASYNC_RESIDENT_CLIP_MB = "
                             f"{_CLIP_CAP >> 20}; use FrameSynthesizer(resident=False) (there is no partial residency)")

    def _upload(self, src: _Chunks) -> torch.Tensor:
        """Host frames -> the device tensor, UPLOAD_CHUNK frames at a time through one reused pinned buffer."""
        dev_frames = stage = copied = None
        at = 0
        try:
            for chunk in src.chunks:
                if not chunk:
                    continue
                shapes = [(f.shape, str(f.dtype)) for f in chunk]
                if dev_frames is None:
                    shape = chunk[0].shape
                if len(shape) != 3 or shape[2] != 3 or any(s != (shape, "uint8") for s in shapes):
                    raise _mixed(shapes + [(shape, "uint8")] * (dev_frames is not None))
                if dev_frames is None:
                    self._check_size(src.n, shape)                       # before anything is allocated
                    frame_bytes = int(np.prod(shape))
                    stage = frame_loop._acquire_pinned(min(src.n, UPLOAD_CHUNK) * frame_bytes)
                    with torch.cuda.device(self.device):
                        dev_frames = torch.empty((src.n,) + tuple(shape), dtype=torch.uint8, device=self.device)
                if len(chunk) > UPLOAD_CHUNK or at + len(chunk) > src.n:
                    raise ValueError("ResidentClip: more frames than announced")
                if copied is not None:
                    copied.synchronize()                                  # the buffer is not written before its last copy is done
                view = stage[:len(chunk) * frame_bytes].view(len(chunk), *shape)
                np.stack(chunk, out=view.numpy())
                with torch.cuda.device(self.device):
                    dev_frames[at:at + len(chunk)].copy_(view, non_blocking=True)
                    copied = torch.cuda.Event()
                    copied.record(torch.cuda.current_stream(self.device))
                at += len(chunk)
            if dev_frames is None or at != src.n:
                raise ValueError(f"ResidentClip: {at} frames arrived, {src.n} were announced")
            return dev_frames
        finally:
            if copied is not None:
                copied.synchronize()
            if stage is not None:
                frame_loop._release_pinned(stage)

    @classmethod
    def from_data_dir(cls, data_dir: str, device="cuda:0", io_workers: int = 8, decode: str = "host") -> "ResidentClip":
        """The clip of an ``infer_data`` directory (frames/, positions/, masks/), every file read once, with the loaders and
        the .jpg / .npy rule of ``frame_synth.FrameSynthesizer``; masks stay uint8 where the file holds uint8.
        ``decode="device"``: the workers read the .jpg frames as bytes and ``jpeg.decode_jpeg_device`` decodes each list of
        ``UPLOAD_CHUNK`` files straight into the clip's storage, so that the compressed bytes cross to the device, not the
        pixels; the frames are the same bytes as with ``"host"`` wherever the host decoder is libjpeg's default path (Pillow,
        cv2).  Masks, .npy frames and files outside the decoder's subset take the host path."""
        from .frame_synth import _imread
        if decode not in ("host", "device"):
            raise ValueError(f"ResidentClip.from_data_dir: decode {decode!r} is neither 'host' nor 'device'")
        frames_dir, positions_dir, masks_dir = (os.path.join(data_dir, d) for d in ("frames", "positions", "masks"))
        names = os.listdir(frames_dir)
        ext = ".jpg" if any(f.endswith(".jpg") for f in names) else ".npy"
        n = len([f for f in names if f.endswith(ext)])
        if n < 1:
            raise ValueError(f"ResidentClip: no frames in {frames_dir}")
        landmarks, masks = [None] * n, [None] * n

        as_bytes = decode == "device" and ext == ".jpg"

        def load(i):
            stem = f"{i:06d}"
            if as_bytes:
                with open(os.path.join(frames_dir, stem + ext), "rb") as f:
                    img = f.read()
            else:
                img = _imread(os.path.join(frames_dir, stem + ext))
            if img is None:
                raise ValueError(f"ResidentClip: cannot read {os.path.join(frames_dir, stem + ext)}")
            landmarks[i] = np.loadtxt(os.path.join(positions_dir, stem + ".txt"))
            path = next((p for p in (os.path.join(masks_dir, stem + e) for e in (".jpg", ".npy")) if os.path.exists(p)), None)
            mask = _imread(path, gray=True) if path else None
            if mask is not None and mask.dtype != np.uint8:
                mask = mask.astype(np.float32) / 255.0                    # as FrameSynthesizer._load_single_frame
            masks[i] = mask
            return img

        with ThreadPoolExecutor(max_workers=max(1, int(io_workers))) as pool:
            chunks = (list(pool.map(load, range(i, min(i + UPLOAD_CHUNK, n)))) for i in range(0, n, UPLOAD_CHUNK))
            if as_bytes:
                return cls(cls._decode_chunks(n, chunks, torch.device(device), frames_dir), landmarks, masks, device)
            return cls(_Chunks(n, chunks), landmarks, masks, device)      # the two lists fill while the frames go up

    @classmethod
    def _decode_chunks(cls, n: int, chunks, device, frames_dir: str) -> torch.Tensor:
        """Lists of JPEG files -> the device tensor [n,H,W,3], each list decoded on the device into its place"""
        from . import jpeg
        frames, at = None, 0
        for files in chunks:
            try:
                if frames is None:
                    try:
                        info = jpeg.parse_jpeg(files[0])                     # its size is the clip's
                        shape = (info.H, info.W, 3)
                    except jpeg.JpegUnsupported:
                        shape = tuple(jpeg.decode_jpeg_device(files[:1], device=device).shape[1:])
                    cls._check_size(n, shape)                                # before the clip is allocated
                    with torch.cuda.device(device):
                        frames = torch.empty((n,) + shape, dtype=torch.uint8, device=device)
                jpeg.decode_jpeg_device(files, out=frames[at:at + len(files)])
            except jpeg.JpegUnreadable as exc:
                raise ValueError(f"ResidentClip: cannot read {os.path.join(frames_dir, f'{at + exc.index:06d}.jpg')}") from exc
            except ValueError as exc:
                if isinstance(exc, (jpeg.JpegUnsupported, jpeg.JpegCorrupt)):
                    raise
                raise _mixed([str(exc)]) from exc
            at += len(files)
        return frames

    @classmethod
    def from_frames(cls, frames_bgr, landmark_detector, boxes=None, chunk: int = 32, masks=None) -> "ResidentClip":
        """Frames to a clip without a directory in between (what step 3's ``VideoPreprocessor.process_frames_batch`` writes to
        disk): ``chunk`` frames at a time go to the device, ``landmark_detector.detect_landmarks_device`` sees their RGB view
        and the first face of a frame gives its landmarks; frames without a face are left out (``source_index`` names the
        kept ones).  ``boxes``: per frame its (x, y, w, h) boxes instead of the detector's."""
        from . import face_ops
        dev = landmark_detector.pfld_backbone.device
        is_tensor = isinstance(frames_bgr, torch.Tensor)
        n_in = int(frames_bgr.shape[0]) if is_tensor else len(frames_bgr)
        if n_in < 1:
            raise ValueError("ResidentClip.from_frames: no frames")
        shape = tuple(int(v) for v in frames_bgr.shape[1:]) if is_tensor else tuple(np.asarray(frames_bgr[0]).shape)
        parts = (frames_bgr[at:at + chunk] for at in range(0, n_in, chunk))
        return cls._from_parts(parts, n_in, shape, landmark_detector, boxes, chunk, masks, "ResidentClip.from_frames")

    @classmethod
    def _from_parts(cls, parts, n_in: int, shape, landmark_detector, boxes, chunk: int, masks, who: str) -> "ResidentClip":
        """from_frames on frames that arrive ``chunk`` at a time (host frames, or uint8 [n,H,W,3] tensors already on the device)"""
        from . import face_ops
        dev = landmark_detector.pfld_backbone.device
        cls._check_size(n_in, shape)
        stager = face_ops.FrameStager(dev)
        kept, landmarks, store = [], [], None
        for at, frames in zip(range(0, n_in, chunk), parts):
            part = stager.upload(frames, who, "frame_loop.submit_batch_device")
            if store is None:
                store = torch.empty((n_in,) + tuple(part.shape[1:]), dtype=torch.uint8, device=part.device)
            found = landmark_detector.detect_landmarks_device(part.flip(-1).contiguous(),
                                                              boxes=None if boxes is None else list(boxes[at:at + chunk]))
            keep = [i for i, faces in enumerate(found) if faces]
            if keep:
                store[len(kept):len(kept) + len(keep)] = part[torch.as_tensor(keep, device=part.device)]
            kept += [at + i for i in keep]
            landmarks += [found[i][0] for i in keep]
        if not kept:
            raise ValueError(f"{who}: no face in any frame")
        clip = cls(store[:len(kept)], landmarks, None if masks is None else [masks[i] for i in kept], dev)
        clip.source_index = kept
        return clip

    @classmethod
    def from_video(cls, path: str, landmark_detector, *, chunk: int = 32, decode: str = "device", boxes=None, masks=None) -> "ResidentClip":
        """A Motion-JPEG AVI file to a clip (``mjpeg_avi.read_avi``): ``chunk`` frames at a time are decoded and go the way of
        ``from_frames`` (landmarks from ``landmark_detector``, or from ``boxes``; frames without a face are left out and
        ``source_index`` names the kept ones).  ``decode="device"``: ``jpeg.decode_jpeg_device(subset="mjpeg")`` decodes the
        files where the clip lives, so that the compressed bytes cross to the device, not the pixels (4:4:4, 4:2:2, 4:2:0 and
        grayscale frames, with or without their Huffman tables; any other JPEG is decoded by Pillow and uploaded);
        ``decode="host"``: Pillow decodes every frame.  Both give the same bytes.  ``clip.audio`` holds the file's PCM sound
        track as ``audio.read_pcm_wav`` would return it, or None; ``clip.fps`` its frame rate."""
        from . import jpeg, mjpeg_avi
        if decode not in ("host", "device"):
            raise ValueError(f"ResidentClip.from_video: decode {decode!r} is neither 'host' nor 'device'")
        if int(chunk) < 1:
            raise ValueError(f"ResidentClip.from_video: chunk {chunk}")
        avi = mjpeg_avi.read_avi(path)
        dev = landmark_detector.pfld_backbone.device
        files, n_in = avi.frames, len(avi.frames)

        def parts():
            for at in range(0, n_in, chunk):
                try:
                    if decode == "device":
                        yield jpeg.decode_jpeg_device(files[at:at + chunk], device=dev, subset="mjpeg")
                    else:
                        yield [jpeg._decode_pillow(f) for f in files[at:at + chunk]]
                except jpeg.JpegUnreadable as exc:
                    raise ValueError(f"ResidentClip.from_video: cannot read frame {at + exc.index} of {path}") from exc
                except OSError as exc:
                    raise ValueError(f"ResidentClip.from_video: cannot read a frame in {at}..{at + chunk - 1} of {path}: {exc}") from exc

        clip = cls._from_parts(parts(), n_in, (avi.height, avi.width, 3), landmark_detector, boxes, int(chunk), masks, "ResidentClip.from_video")
        clip.audio, clip.fps = avi.audio, avi.fps
        return clip

    def __len__(self) -> int:
        return int(self.frames.shape[0])

    def close(self) -> None:
        """Give the device memory back (after the work in flight has finished)."""
        if self.frames is not None:
            torch.cuda.synchronize(self.device)
            self._reap(wait=True)
            self.frames, self._masks = None, []

    # ------------------------------------------------------------------ batches
    def _reap(self, wait: bool = False) -> None:
        """Record blocks of batches the GPU has finished go back to the pinned pool."""
        busy = []
        for done, block in self._inflight:
            if wait:
                done.synchronize()
            if wait or done.query():
                frame_loop._release_pinned(block)
            else:
                busy.append((done, block))
        self._inflight = busy

    def _indices(self, indices) -> np.ndarray:
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        if self.frames is None:
            raise RuntimeError("ResidentClip: closed")
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError(f"ResidentClip: indices outside [0, {len(self)})")
        return idx

    def _compose(self, rec_ptr: int, batch: int, out_regions, regions_bytes: int, download: bool) -> PendingClipBatch:
        """Enqueue compose (+ the download) on the current stream; rec_ptr: the records in host memory."""
        dev = self.device
        out = torch.empty((batch, self.H, self.W, 3), dtype=torch.uint8, device=dev)
        if batch:
            _lib.check(_lib.load().casync_op_clip_compose(
                self.frames.data_ptr(), len(self), self.H, self.W, rec_ptr, batch,
                out_regions.data_ptr() if out_regions is not None else None, regions_bytes, out.data_ptr(),
                torch.cuda.current_stream(dev).cuda_stream), "casync_op_clip_compose")
        pending = PendingClipBatch(out, None, None)
        if download:
            pending._download()
        return pending

    def fetch(self, indices, *, download: bool = True) -> PendingClipBatch:
        """The stored frames ``indices`` as a batch (compose with no valid record): pass-through mode, and what a batch that
        cannot be synthesised comes back as."""
        idx = self._indices(indices)
        rec = np.zeros((idx.size, REC_WORDS), dtype=np.int32)
        rec[:, 0] = idx
        with torch.cuda.device(self.device):
            return self._compose(rec.ctypes.data, idx.size, None, 0, download)      # records are read before the call returns

    def _batch_records(self, idx: np.ndarray):
        """The geometry records [B,12], points [B,33,2] and clip records [B,8] of a batch, from the static table (numpy only),
        and the bytes of its packed regions.  The regions are packed as ``frame_loop.submit_batch_device`` packs them."""
        geo = self.geometry
        B = idx.size
        h, w, width, valid = self._h[idx], self._w[idx], geo.box[idx, 4], geo.valid[idx].astype(np.int64)
        reg = h * w * 3
        reg_off = np.cumsum(reg) - reg
        reg_total = int(reg.sum())
        if reg_total >= 2 ** 31:
            raise ValueError("batch too large for 32-bit region offsets")
        synth = valid * width * width * 3
        geom = np.zeros((B, frame_loop.GEOM_WORDS), dtype=np.int32)
        geom[:, 0], geom[:, 1], geom[:, 2], geom[:, 3], geom[:, 4] = reg_off, h, w, width, valid
        geom[:, 5], geom[:, 6] = np.cumsum(synth) - synth, np.cumsum(h * w) - h * w
        geom[:, 7:12] = self._mask_words[idx]
        rec = np.zeros((B, REC_WORDS), dtype=np.int32)
        rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5], rec[:, 6] = idx, geo.box[idx, 0], geo.box[idx, 2], h, w, valid, reg_off
        return geom, geo.pts[idx], rec, reg_total

    def submit(self, net, indices, *, windows=None, features=None, frame_indices=None, download: bool = True) -> PendingClipBatch:
        """Enqueue the synthesis of the stored frames ``indices`` (they may repeat and descend) without waiting for the GPU:
        one small pinned upload of [geom | pts | records], gather -> ``frame_loop.regions_through_net`` -> compose.
        ``windows`` [B,32,32,32] on the device, or ``features`` [T,2,1024] on the device + ``frame_indices``, as for
        ``frame_loop.submit_batch_device``.  ``download=False`` leaves the download to a later ``result()``: a device
        consumer takes ``result_device()`` and nothing crosses to the host.  A batch that holds a frame with an empty crop
        box comes back as the stored frames (the reference's "returning the original frames")."""
        idx = self._indices(indices)
        dev = self.frames.device
        if torch.device(net._device()).type != "cuda":
            raise RuntimeError("ResidentClip.submit needs the model on a ROCm device (no CPU fallback)")
        B = idx.size
        geo = self.geometry
        if B == 0 or geo.empty[idx].any():
            if B:
                print(f"process_batch failed, returning the original frames: empty crop box in frame(s) "
                      f"{[int(i) for i in idx[geo.empty[idx]]]}")
            return self.fetch(idx, download=download)
        self._reap()
        geom, pts, rec, reg_total = self._batch_records(idx)
        al = lambda n: (n + 15) & ~15
        o_pts = al(geom.nbytes)
        o_rec = o_pts + al(pts.nbytes)
        total = o_rec + rec.nbytes
        stage = frame_loop._acquire_pinned(total)
        st = stage.numpy()
        st[:geom.nbytes] = geom.reshape(-1).view(np.uint8)
        st[o_pts:o_pts + pts.nbytes] = pts.reshape(-1).view(np.uint8)
        st[o_rec:total] = rec.reshape(-1).view(np.uint8)
        lib = _lib.load()
        try:
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                staged = torch.empty(total, dtype=torch.uint8, device=dev)
                staged.copy_(stage[:total], non_blocking=True)
                regions = torch.empty(reg_total, dtype=torch.uint8, device=dev)
                rec_ptr = stage.data_ptr() + o_rec                     # host memory: the operators read it before they return
                _lib.check(lib.casync_op_clip_gather(self.frames.data_ptr(), len(self), self.H, self.W, rec_ptr, B, regions.data_ptr(),
                                                     reg_total, stream), "casync_op_clip_gather")
                out_regions = frame_loop.regions_through_net(net, regions.data_ptr(), staged.data_ptr(), staged.data_ptr() + o_pts, geom,
                                                             reg_total, windows=windows, features=features, frame_indices=frame_indices)
                pending = self._compose(rec_ptr, B, out_regions, reg_total, download)
                done = torch.cuda.Event()
                done.record(torch.cuda.current_stream(dev))
        except Exception:
            torch.cuda.synchronize(dev)          # whatever was enqueued may still read the block
            frame_loop._release_pinned(stage)
            raise
        # the device tensors may be dropped here (torch's allocator is stream-ordered); the pinned block is the clip's until
        # the upload that reads it has passed
        self._inflight.append((done, stage))
        return pending
