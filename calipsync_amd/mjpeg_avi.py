"""Motion-JPEG AVI writer and reader without OpenCV / ffmpeg: the offline driver's fallback container, and a video source.

The reference saves its frames with ``cv2.VideoWriter(..., 'mp4v', fps, (w, h))`` and muxes the audio with the ``ffmpeg``
binary (inference.py:88-110).  Neither exists in this image; ``VideoStreamManager`` uses them when they do.  Without them
the frames used to go to a ``.npy`` file only; this module writes them as a playable video instead: every frame is
JPEG-encoded with Pillow and stored as one ``00dc`` chunk of a RIFF/AVI file ('MJPG' stream, an ``idx1`` index, fixed
frame rate).  ``write_mjpeg_avi(..., audio=)`` adds the sound track: an AVI carries uncompressed PCM, so the WAV's own bytes
go into ``01wb`` chunks interleaved with the frames, and no encoder is needed (compressed audio stays out of reach).

``read_avi(path)`` is the way back, and reads what other writers produce as well (capture cards, ``ffmpeg -c:v mjpeg``): the
JPEG data of every frame, untouched, for ``jpeg.decode_jpeg_device(subset="mjpeg")`` or any JPEG decoder, and the PCM track.
Plain RIFF/AVI only: OpenDML files above the first RIFF, other codecs and interlaced two-field MJPEG are refused by name.
Host code only: the standard library and numpy.
"""
from __future__ import annotations

import io
import os
import struct
from typing import Iterable, List, Optional

import numpy as np


def _chunk(fourcc: bytes, data: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")


def _list(kind: bytes, data: bytes) -> bytes:
    return b"LIST" + struct.pack("<I", len(data) + 4) + kind + data


def encode_jpeg(frame_bgr: np.ndarray, quality: int = 95) -> bytes:
    """One BGR uint8 HxWx3 frame (the frame loop's layout, cv2 order) as a baseline JPEG."""
    from PIL import Image
    if frame_bgr.dtype != np.uint8 or frame_bgr.ndim != 3 or frame_bgr.shape[2] != 3:
        raise ValueError(f"frames must be uint8 HxWx3 (BGR), got {frame_bgr.dtype} {frame_bgr.shape}")
    buf = io.BytesIO()
    # 4:4:4 (no chroma subsampling): the synthesised mouth region is small and colour edges matter more than file size
    Image.fromarray(np.ascontiguousarray(frame_bgr[:, :, ::-1])).save(buf, format="JPEG", quality=quality, subsampling=0)
    return buf.getvalue()


def jpeg_size(data) -> tuple:
    """(height, width) of an encoded JPEG, from its SOF0..SOF2 segment (a walk over the marker segments ahead of the scan)."""
    d = bytes(data[:2]) if len(data) >= 2 else b""
    if d != b"\xff\xd8":
        raise ValueError("an encoded frame must be a JPEG file (no SOI marker)")
    pos, n = 2, len(data)
    while pos + 4 <= n:
        if data[pos] != 0xFF:
            break
        marker, length = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        if marker in (0xC0, 0xC1, 0xC2) and pos + 9 <= n:
            return (data[pos + 5] << 8) | data[pos + 6], (data[pos + 7] << 8) | data[pos + 8]
        if marker == 0xDA:
            break
        pos += 2 + length
    raise ValueError("an encoded frame has no SOF segment ahead of its scan")


RIFF_LIMIT = (1 << 32) - (1 << 20)     # 32-bit RIFF sizes (plain AVI, no OpenDML segments): stop a MiB short of 4 GiB


def stream_rate(fps: float) -> tuple:
    """(dwRate, dwScale) of a video stream of `fps`: thousandths of a frame per second"""
    return int(round(fps * 1000)), 1000


def audio_span(k: int, rate: int, vrate: int, scale: int) -> int:
    """the first audio sample frame of video frame k: exact integer arithmetic, so non-integer frame rates do not drift"""
    return (k * rate * scale) // vrate


def _pcm_track(audio):
    """a WAV path or (pcm, rate, width) -> (the file's bytes, channels, rate, width)"""
    from . import audio as _audio
    if isinstance(audio, (str, os.PathLike)):
        audio = _audio.read_pcm_wav(os.fspath(audio))
    try:
        pcm, rate, width = audio
    except (TypeError, ValueError):
        raise ValueError("audio must be a WAV path or (pcm, rate, width) as audio.read_pcm_wav returns them") from None
    pcm = np.asarray(pcm)
    if pcm.ndim == 1:
        pcm = pcm[:, None]
    if pcm.ndim != 2 or pcm.shape[1] < 1 or pcm.shape[1] > 65535:
        raise ValueError(f"audio: PCM must be [frames, channels], got {pcm.shape}")
    if int(rate) != rate or not 1 <= int(rate) < 1 << 32:
        raise ValueError(f"audio: sample rate {rate!r}")
    raw = _audio.pcm_bytes(pcm, width).tobytes()                 # ValueError for a width outside 1..4 or samples that are no integers
    return raw, int(pcm.shape[1]), int(rate), int(width)


def write_mjpeg_avi(path: str, frames: Iterable[np.ndarray], fps: float = 25.0, quality: int = 95, audio=None) -> int:
    """Write `frames` (BGR uint8, all the same size) to `path` as Motion-JPEG AVI; returns the frame count.  An item that is
    `bytes` / `bytearray` / `memoryview` is an already encoded JPEG (``jpeg.encode_jpeg_device``): it is stored as it is, its
    size read from its SOF segment; arrays and encoded items may be mixed.

    `audio`: a WAV path, or ``(pcm, rate, width)`` as ``audio.read_pcm_wav`` returns them (integer PCM of 1, 2, 3 or 4 bytes,
    any channel count), becomes a second stream of uncompressed PCM: the samples' own bytes, nothing resampled or requantised.
    After the ``00dc`` chunk of frame k comes a ``01wb`` chunk with the sample frames ``[k * rate * scale // vrate,
    (k + 1) * rate * scale // vrate)`` (vrate / scale: the video stream's rate; no chunk where that range is empty); audio past
    the last frame goes into one last chunk, audio shorter than the video simply ends.  None writes the file without a track.

    Frames are encoded and written one at a time (one JPEG in memory, not the clip); the header fields that depend on
    the whole clip (frame count, largest chunk, RIFF / LIST sizes) are patched when the last frame is on disk.  The
    container is plain RIFF/AVI with 32-bit sizes: a clip that would pass 4 GiB (about five minutes of 1080p at this
    quality) raises ValueError at the frame that would cross the limit, and the partial file is removed -- it fails while
    encoding, not after it."""
    usec = int(round(1e6 / fps))
    rate, scale = stream_rate(fps)
    n, biggest, width, height = 0, 0, None, None
    index = []
    fh = None
    track = None if audio is None else _pcm_track(audio)
    if track:
        pcm, a_ch, a_rate, a_width = track
        align = a_ch * a_width
        a_total, a_at, a_biggest = len(pcm) // align, 0, 0
    try:
        for f in frames:
            encoded = isinstance(f, (bytes, bytearray, memoryview))
            size = jpeg_size(f) if encoded else tuple(f.shape[:2])
            if width is None:
                height, width = size
                fh = open(path, "wb")
                # header with the clip-dependent fields zeroed: patched below (positions recorded as they are written)
                avih = struct.pack("<14I", usec, 0, 0, 0x10, 0, 0, 1, 0, width, height, 0, 0, 0, 0)   # 0x10 = AVIF_HASINDEX
                strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, scale, rate, 0, 0, 0, 0xFFFFFFFF, 0, 0, 0, width, height)
                strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
                strls = _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf))
                if track:                                            # the video strl stays first: its patch positions hold
                    avih = struct.pack("<14I", usec, 0, 0, 0x110, 0, 0, 2, 0, width, height, 0, 0, 0, 0)   # | AVIF_ISINTERLEAVED
                    astrh = b"auds" + bytes(4) + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, 1, a_rate, 0, a_total, 0, 0xFFFFFFFF, align, 0, 0, 0, 0)
                    astrf = struct.pack("<HHIIHH", 1, a_ch, a_rate, a_rate * align, align, 8 * a_width)    # PCM WAVEFORMAT
                    strls += _list(b"strl", _chunk(b"strh", astrh) + _chunk(b"strf", astrf))
                hdrl = _list(b"hdrl", _chunk(b"avih", avih) + strls)
                fh.write(b"RIFF" + struct.pack("<I", 0) + b"AVI " + hdrl)
                movi_at = fh.tell()
                fh.write(b"LIST" + struct.pack("<I", 0) + b"movi")
                off = 4                                              # idx1 offsets count from the 'movi' fourcc
            elif size != (height, width):
                raise ValueError("all frames of a video must have the same size")
            j = bytes(f) if encoded else encode_jpeg(f, quality)
            chunk = _chunk(b"00dc", j)
            sound = b""
            if track:
                a_end = min(audio_span(n + 1, a_rate, rate, scale), a_total)
                if a_end > a_at:
                    sound = _chunk(b"01wb", pcm[a_at * align:a_end * align])
            if fh.tell() + len(chunk) + len(sound) + 16 * (len(index) + 1 + bool(sound)) + 8 > RIFF_LIMIT:
                raise ValueError(f"{path}: the clip passes the 4 GiB limit of a plain AVI file at frame {n} "
                                 f"({fh.tell() / 2 ** 30:.2f} GiB written): write it in shorter segments")
            fh.write(chunk)
            index.append((b"00dc", off, len(j)))
            off += len(chunk)
            if sound:
                fh.write(sound)
                index.append((b"01wb", off, (a_end - a_at) * align))
                off += len(sound)
                a_biggest = max(a_biggest, (a_end - a_at) * align)
                a_at = a_end
            biggest = max(biggest, len(j))
            n += 1
        if n == 0:
            raise ValueError("no video frame was generated")
        if track and a_at < a_total:                                 # audio longer than the video: one last chunk
            sound = _chunk(b"01wb", pcm[a_at * align:a_total * align])
            if fh.tell() + len(sound) + 16 * (len(index) + 1) + 8 > RIFF_LIMIT:
                raise ValueError(f"{path}: the clip passes the 4 GiB limit of a plain AVI file at the audio behind frame {n - 1} "
                                 f"({fh.tell() / 2 ** 30:.2f} GiB written): write it in shorter segments")
            fh.write(sound)
            index.append((b"01wb", off, (a_total - a_at) * align))
            a_biggest = max(a_biggest, (a_total - a_at) * align)
        movi_size = fh.tell() - movi_at - 8
        fh.write(_chunk(b"idx1", b"".join(cc + struct.pack("<III", 0x10, o, ln) for cc, o, ln in index)))   # 0x10 = AVIIF_KEYFRAME
        riff_size = fh.tell() - 8
        # patches: RIFF size; avih (at 32): dwMaxBytesPerSec (+4), dwTotalFrames (+16), dwSuggestedBufferSize (+28);
        # strh (at 108): dwLength (+32), dwSuggestedBufferSize (+36); the movi LIST size
        patches = [(4, riff_size), (32 + 4, int(biggest * fps) + (a_rate * align if track else 0)), (32 + 16, n), (32 + 28, biggest),
                   (108 + 32, n), (108 + 36, biggest), (movi_at + 4, movi_size)]
        if track:       # the audio strh (at 232, behind the video strl): dwSuggestedBufferSize (+36); avih's byte rate above counts the samples
            patches.append((232 + 36, a_biggest))
        for pos, value in patches:
            fh.seek(pos)
            fh.write(struct.pack("<I", value))
        fh.close()
        fh = None
        return n
    finally:
        if fh is not None:              # an error part-way: no half-written file is left behind
            fh.close()
            try:
                os.remove(path)
            except OSError:
                pass


def read_mjpeg_avi(path: str):
    """(fps, [BGR frames]) of a file written by `write_mjpeg_avi` (tests; a minimal RIFF walk, not a general AVI reader)."""
    from PIL import Image
    data = open(path, "rb").read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError("not a RIFF/AVI file")
    fps, frames = None, []

    def walk(lo: int, hi: int) -> None:
        nonlocal fps
        pos = lo
        while pos + 8 <= hi:
            cc, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
            body = pos + 8
            if cc == b"LIST":
                walk(body + 4, body + size)
            elif cc == b"strh":
                scale, rate = struct.unpack("<II", data[body + 20:body + 28])
                fps = rate / scale
            elif cc == b"00dc":
                im = Image.open(io.BytesIO(data[body:body + size])).convert("RGB")
                frames.append(np.ascontiguousarray(np.asarray(im)[:, :, ::-1]))
            pos = body + size + (size & 1)

    walk(12, len(data))
    return fps, frames


class AviClip:
    """What read_avi reads.  fps = rate / scale of the video stream (both kept); width, height; frames: the JPEG data of every
    video frame in order (memoryviews of the file's bytes; a dropped frame repeats the one before it); audio: None, or (pcm
    [n, C], rate, width) in the form audio.read_pcm_wav returns; notes: what was skipped or stood in, in words."""
    __slots__ = ("fps", "rate", "scale", "width", "height", "frames", "audio", "notes")

    def __len__(self) -> int:
        return len(self.frames)


def _u32(data, pos: int) -> int:
    return struct.unpack_from("<I", data, pos)[0]


def _chunks(data, lo: int, hi: int):
    """(fourcc, body start, size) of the chunks in data[lo:hi], one after the other, until one does not fit"""
    pos = lo
    while pos + 8 <= hi:
        size = _u32(data, pos + 4)
        if pos + 8 + size > hi:
            return
        yield bytes(data[pos:pos + 4]), pos + 8, size
        pos += 8 + size + (size & 1)


def read_avi(path: str, audio: str = "auto") -> AviClip:
    """A Motion-JPEG AVI file -> AviClip: the frames' JPEG data as it lies in the file and the PCM sound track, if any.

    The ``movi`` list is walked chunk by chunk and ``idx1`` is ignored, so the reader copes with ``LIST rec `` groups, ``JUNK``
    anywhere, odd-sized chunks, either stream order (the stream numbers come from the order of the ``strl`` lists), a zero-length
    video chunk (a dropped frame: the previous frame stands in; a zero-length first frame is an error) and a file cut off
    mid-recording (no ``idx1``, sizes that run past the end: every whole chunk is read, the incomplete one is dropped).

    ValueError, naming the cause, for a video stream that is not ``MJPG``, an OpenDML file (``RIFF AVIX``), a frame whose JPEG
    size is not the stream's (interlaced two-field MJPEG looks like that) and, under ``audio="require"``, a sound track that is
    missing or not PCM; under the default ``audio="auto"`` such a track gives ``audio=None`` and a line in ``notes``."""
    if audio not in ("auto", "require"):
        raise ValueError(f"read_avi: audio {audio!r} is neither 'auto' nor 'require'")
    with open(path, "rb") as f:
        data = memoryview(f.read())
    n = len(data)
    if n < 12 or data[:4] != b"RIFF" or bytes(data[8:12]) not in (b"AVI ", b"AVIX"):
        raise ValueError(f"{path}: not a RIFF/AVI file")
    if data[8:12] == b"AVIX":
        raise ValueError(f"{path}: an OpenDML continuation (RIFF AVIX) without its first RIFF")
    first_end = 8 + _u32(data, 4)
    first_end += first_end & 1
    if first_end + 12 <= n and data[first_end:first_end + 4] == b"RIFF" and data[first_end + 8:first_end + 12] == b"AVIX":
        raise ValueError(f"{path}: an OpenDML file (RIFF AVIX segments behind the first RIFF): only plain AVI is read")
    end = first_end if 24 <= first_end <= n else n               # a recorder that never patched its sizes: to the end of the file
    clip = AviClip()
    clip.notes, clip.audio = [], None
    streams, movi = [], None                                     # [(fccType, strh body, strf body)] in strl order
    pos = 12
    while pos + 12 <= end:                                       # top level of the RIFF; a movi list may run past the end
        cc, size = bytes(data[pos:pos + 4]), _u32(data, pos + 4)
        if cc == b"LIST" and data[pos + 8:pos + 12] == b"movi":
            movi = (pos + 12, n if size < 4 or pos + 8 + size > n else pos + 8 + size)
            break
        if cc == b"LIST" and data[pos + 8:pos + 12] == b"hdrl":
            for c2, b2, s2 in _chunks(data, pos + 12, min(pos + 8 + size, n)):
                if c2 == b"LIST" and data[b2:b2 + 4] == b"strl":
                    parts = {c3: (b3, s3) for c3, b3, s3 in _chunks(data, b2 + 4, b2 + s2)}
                    if b"strh" not in parts or b"strf" not in parts or parts[b"strh"][1] < 48:
                        raise ValueError(f"{path}: stream {len(streams)} has no strh / strf")
                    streams.append((bytes(data[parts[b"strh"][0]:][:4]), parts[b"strh"], parts[b"strf"], b"indx" in parts))
        pos += 8 + size + (size & 1)
    if movi is None:
        raise ValueError(f"{path}: no movi list")
    video = next((i for i, s in enumerate(streams) if s[0] == b"vids"), None)
    sound = next((i for i, s in enumerate(streams) if s[0] == b"auds"), None)
    if video is None:
        raise ValueError(f"{path}: no video stream")
    _, (h_at, _), (f_at, f_size), _ = streams[video]
    clip.scale, clip.rate = struct.unpack_from("<II", data, h_at + 20)
    if f_size < 20 or not clip.scale or not clip.rate:
        raise ValueError(f"{path}: the video stream has no format or no rate")
    clip.fps = clip.rate / clip.scale
    clip.width, height = struct.unpack_from("<ii", data, f_at + 4)
    clip.height = abs(height)
    fourcc = bytes(data[f_at + 16:f_at + 20])
    if fourcc.upper() != b"MJPG":
        raise ValueError(f"{path}: the video stream is {fourcc.decode('latin-1')!r}, not Motion-JPEG ('MJPG')")
    fmt = None
    if sound is not None:
        _, _, (a_at, a_size), _ = streams[sound]
        tag, ch, a_rate, _, align, bits = struct.unpack_from("<HHIIHH", data, a_at) if a_size >= 16 else (0, 0, 0, 0, 0, 0)
        if tag != 1 or bits % 8 or not 1 <= bits // 8 <= 4 or ch < 1 or align != ch * (bits // 8):
            what = f"{path}: the audio stream is not PCM (wFormatTag {tag:#x}, {bits} bits): only uncompressed PCM is read"
            if audio == "require":
                raise ValueError(what)
            clip.notes.append(what + "; audio=None")
        else:
            fmt = (ch, a_rate, bits // 8)
    elif audio == "require":
        raise ValueError(f"{path}: no audio stream")
    if len(streams) > 1 + (sound is not None):
        clip.notes.append(f"{len(streams)} streams: only the first video and the first audio stream are read")
    frames: List = []
    pcm: List = []
    pos, hi = movi
    while pos + 8 <= hi:
        cc, size = bytes(data[pos:pos + 4]), _u32(data, pos + 4)
        if cc == b"LIST":                                        # 'rec ' groups: their chunks are read in place
            pos += 12
            continue
        if pos + 8 + size > n:                                   # cut off inside this chunk
            clip.notes.append(f"the file ends inside a chunk at byte {pos}: {len(frames)} whole frames were read")
            break
        if pos + 8 + size > hi:
            break
        number = int(cc[:2], 16) if cc[:2].isalnum() and all(c in b"0123456789abcdefABCDEF" for c in cc[:2]) else -1
        if number == video and cc[2:] in (b"dc", b"db"):
            if size == 0:
                if not frames:
                    raise ValueError(f"{path}: frame 0 is empty (a dropped frame with no frame before it)")
                frames.append(frames[-1])
                clip.notes.append(f"frame {len(frames) - 1} was dropped by the writer: frame {len(frames) - 2} stands in")
            else:
                frames.append(data[pos + 8:pos + 8 + size])
        elif number == sound and cc[2:] == b"wb" and fmt:
            pcm.append(data[pos + 8:pos + 8 + size])
        pos += 8 + size + (size & 1)
    if not frames:
        raise ValueError(f"{path}: no video frame")
    if streams[video][3] and first_end < n and bytes(data[first_end:first_end + 4]) == b"RIFF":
        raise ValueError(f"{path}: an OpenDML file (an indx super-index and data behind the first RIFF): only plain AVI is read")
    seen = {}
    for i, f in enumerate(frames):
        if id(f) in seen:
            continue
        seen[id(f)] = True
        try:
            size = jpeg_size(f)
        except ValueError as exc:
            raise ValueError(f"{path}: frame {i}: {exc}") from None
        if size != (clip.height, clip.width):
            raise ValueError(f"{path}: frame {i} is a JPEG of {size[0]} x {size[1]} (h x w), the stream says {clip.height} x {clip.width} "
                             f"(interlaced two-field Motion-JPEG is not read)")
    clip.frames = frames
    if fmt:
        from . import audio as _audio
        ch, a_rate, a_width = fmt
        raw = b"".join(pcm)
        raw = raw[:len(raw) - len(raw) % (ch * a_width)]
        clip.audio = (_audio.pcm_from_bytes(raw, ch, a_width), a_rate, a_width)
    return clip
