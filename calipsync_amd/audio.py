"""The audio front end on the device: the PCM bytes of a WAV file at any rate -> the mono 16 kHz waveform and its Wav2Vec2
normalisation (csrc/audio.hip), without ffmpeg.

* ``read_pcm_wav(path)`` reads a RIFF PCM file with the standard library: the integers as they are stored, any rate.
* ``resample_taps(rate)`` designs the polyphase filter of ``scipy.signal.resample_poly(x, up, down)`` at its defaults (a Kaiser
  windowed sinc, beta 5, 10 max(up, down) taps to either side) in float64 and rounds it once to fp32.
* ``frontend_host`` is the numpy twin of the device path (float64 sums, rounded to fp32 where the device holds fp32): its oracle.
* ``frontend_device`` uploads the bytes once and runs decode, downmix, resampling and normalisation as HIP kernels.

The arithmetic is scipy's, not ffmpeg's (swresample) or librosa's (soxr): their filters differ, and parity with them is not
pinned anywhere in this repository.  ``HubertExtractor(frontend="device")`` opts in; the default stays the ffmpeg path.
"""
from __future__ import annotations

import math
import wave as _wave
from typing import Dict, Tuple

import numpy as np

TARGET_RATE = 16000
MONO = {"mean": 0, "first": 1}      # -> the `mono` of casync_op_audio_resample
FRONTENDS = ("reference", "device")
_SCALE = {1: 128.0, 2: 32768.0, 3: 8388608.0, 4: 2147483648.0}


def check_mono(mono: str) -> int:
    """-> the kernel's number; ValueError for anything but "mean" / "first" (before any device call)."""
    if mono not in MONO:
        raise ValueError(f"mono {mono!r}; the audio front end has {sorted(MONO)}")
    return MONO[mono]


def check_frontend(frontend: str) -> str:
    """ValueError for anything but "reference" / "device" (before any device call)."""
    if frontend not in FRONTENDS:
        raise ValueError(f"audio front end {frontend!r}; there are {list(FRONTENDS)}")
    return frontend


def ratio(rate: int) -> Tuple[int, int]:
    """-> (up, down) = (16000, rate) in lowest terms."""
    rate = int(rate)
    if rate < 1:
        raise ValueError(f"sample rate {rate}")
    g = math.gcd(rate, TARGET_RATE)
    return TARGET_RATE // g, rate // g


def out_samples(n: int, rate: int) -> int:
    """Samples at 16 kHz of n samples at `rate`: ceil(n up / down)."""
    up, down = ratio(rate)
    return -((-int(n) * up) // down)


def read_pcm_wav(path: str) -> Tuple[np.ndarray, int, int]:
    """RIFF PCM WAV -> (integers [frames, C] as stored, rate, bytes per sample).  uint8 for 8-bit files (offset binary, as
    stored), int16, and int32 for 24- and 32-bit ones.  ValueError for a compressed file or another sample size."""
    with _wave.open(path, "rb") as w:
        if w.getcomptype() != "NONE":
            raise ValueError(f"{path}: compressed WAV ({w.getcomptype()}); only PCM is read")
        ch, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    try:
        return pcm_from_bytes(raw, ch, width), rate, width
    except ValueError as exc:
        raise ValueError(f"{path}: {exc}") from None


def pcm_from_bytes(raw, channels: int, width: int) -> np.ndarray:
    """Little-endian PCM bytes -> the integers [frames, C] of read_pcm_wav (the inverse of pcm_bytes): uint8 for 8-bit samples
    (offset binary, as stored), int16, and int32 for 24- and 32-bit ones.  ValueError for another sample size."""
    if width == 1:
        x = np.frombuffer(raw, np.uint8)
    elif width == 2:
        x = np.frombuffer(raw, "<i2")
    elif width == 3:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.int32)
    elif width == 4:
        x = np.frombuffer(raw, "<i4")
    else:
        raise ValueError(f"{8 * width}-bit samples")
    return x.reshape(-1, channels)


def pcm_bytes(pcm: np.ndarray, width: int) -> np.ndarray:
    """The integers of read_pcm_wav -> the file's little-endian bytes [frames * C * width] (uint8)."""
    pcm = np.asarray(pcm)
    if width not in _SCALE:
        raise ValueError(f"{8 * width}-bit samples")
    if pcm.dtype.kind not in "iu":
        raise ValueError(f"PCM samples are integers, not {pcm.dtype}")
    flat = np.ascontiguousarray(pcm).reshape(-1)
    if width == 1:
        return flat.astype(np.uint8)
    if width == 2:
        return flat.astype("<i2").view(np.uint8)
    b = flat.astype("<i4").view(np.uint8).reshape(-1, 4)
    return np.ascontiguousarray(b[:, :3]).reshape(-1) if width == 3 else b.reshape(-1)


def decode(pcm: np.ndarray, width: int) -> np.ndarray:
    """The integers of read_pcm_wav -> float64 in [-1, 1), scaled as hubert.read_wav scales them (exact)."""
    x = np.asarray(pcm).astype(np.float64)
    if width == 1:
        x = x - 128.0
    return x / _SCALE[width]


def resample_taps(rate: int, dtype=np.float32) -> np.ndarray:
    """h[m + half] = up w[m] / sum(w), w[m] = sinc(m / R) / R * kaiser(2 half + 1, 5)[m + half], R = max(up, down), half = 10 R:
    designed in float64, rounded once to `dtype`.  16 kHz has no filter: the single tap 1."""
    up, down = ratio(rate)
    if up == down:
        return np.ones(1, dtype=dtype)
    r = max(up, down)
    half = 10 * r
    m = np.arange(-half, half + 1, dtype=np.float64)
    w = np.sinc(m / r) / r * np.kaiser(2 * half + 1, 5.0)
    return (up * w / w.sum()).astype(dtype)


def resample_host(x: np.ndarray, up: int, down: int, taps: np.ndarray, ks=None) -> np.ndarray:
    """y[k] = sum_i x[i] taps[k down + half - i up] in float64, zeros outside both arrays: the formula itself, output by
    output (int64 indices).  `ks`: the outputs wanted (default all ceil(n up / down))."""
    x = np.asarray(x, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    n, half = len(x), (len(taps) - 1) // 2
    ks = np.arange(-((-n * up) // down), dtype=np.int64) if ks is None else np.asarray(ks, dtype=np.int64)
    if up == down:
        return x[ks].copy()
    span = np.arange(2 * half // up + 1, dtype=np.int64)          # the most inputs one output reaches
    out = np.zeros(len(ks), dtype=np.float64)
    for a in range(0, len(ks), 1 << 15):
        c = ks[a:a + (1 << 15)] * down
        lo = np.maximum(0, -((half - c) // up))                    # ceil((c - half) / up)
        i = lo[:, None] + span[None, :]
        t = c[:, None] + half - i * up
        ok = (i < n) & (t >= 0)
        out[a:a + len(c)] = np.where(ok, x[np.minimum(i, n - 1)] * taps[np.maximum(t, 0)], 0.0).sum(axis=1)
    return out


def downmix(x: np.ndarray, mono: str) -> np.ndarray:
    """[frames, C] float64 -> [frames]: the channel mean (summed in channel order) or channel 0."""
    check_mono(mono)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        return x
    return x[:, 0].copy() if mono == "first" else x.sum(axis=1) / x.shape[1]


def normalize_host(x: np.ndarray, exact: bool = False) -> np.ndarray:
    """(x - mean) (var + 1e-7)^-1/2 with float64 moments.  Default: the device's roundings, (x - fp32(mean)) * fp32(r) in fp32;
    exact: float64 throughout."""
    x64 = np.asarray(x, dtype=np.float64)
    mean, var = x64.mean(), x64.var()
    r = 1.0 / np.sqrt(var + 1e-7)
    if exact:
        return (x64 - mean) * r
    return (np.asarray(x, dtype=np.float32) - np.float32(mean)) * np.float32(r)


def frontend_host(pcm: np.ndarray, rate: int, width: int, mono: str = "mean", exact: bool = False):
    """The numpy twin of frontend_device -> (wave16k, normalised).  Every sum is float64; the default rounds to fp32 where the
    device holds fp32 (the decoded sample, the downmixed frame, the taps, the resampled sample, the normalised one), `exact`
    rounds nowhere and returns float64: the formula itself, scipy.signal.resample_poly's to rounding."""
    check_mono(mono)
    hold = (lambda a: a) if exact else (lambda a: np.asarray(a, dtype=np.float32).astype(np.float64))
    pcm = np.asarray(pcm)
    x = hold(decode(pcm.reshape(len(pcm), -1), width))
    x = hold(downmix(x, mono))
    up, down = ratio(rate)
    y = hold(resample_host(x, up, down, resample_taps(rate, np.float64 if exact else np.float32)))
    if exact:
        return y, normalize_host(y, exact=True)
    y = y.astype(np.float32)
    return y, normalize_host(y)


_TAPS_DEV: Dict[tuple, object] = {}      # (rate, device) -> the fp32 taps on that device


def taps_device(rate: int, device):
    """resample_taps(rate) on the device, uploaded once per rate and device."""
    import torch
    key = (int(rate), str(torch.device(device)))
    if key not in _TAPS_DEV:
        _TAPS_DEV[key] = torch.from_numpy(resample_taps(rate)).to(device)
    return _TAPS_DEV[key]


def resample_device(raw, width: int, channels: int, mono: str, up: int, down: int, taps):
    """casync_op_audio_resample on device tensors: raw uint8 [frames * channels * width], taps fp32 (None when up == down)
    -> fp32 [ceil(frames up / down)]."""
    import torch
    from . import _lib
    lib = _lib.load()
    frames = raw.numel() // (channels * width)
    n_out = -((-frames * up) // down)
    out = torch.empty(n_out, dtype=torch.float32, device=raw.device)
    strm = torch.cuda.current_stream(raw.device).cuda_stream
    _lib.check(lib.casync_op_audio_resample(raw.data_ptr(), width, channels, frames, check_mono(mono), up, down,
                                            0 if taps is None else taps.data_ptr(), 0 if taps is None else taps.numel(),
                                            out.data_ptr(), n_out, strm), "casync_op_audio_resample")
    return out


def normalize_device(x, return_moments: bool = False):
    """casync_op_audio_normalize on a device fp32 tensor [n] -> the normalised tensor (and the float64 {mean, var} tensor)."""
    import torch
    from . import _lib
    lib = _lib.load()
    x = x.contiguous()
    ws = torch.empty(lib.casync_op_audio_workspace_bytes(x.numel()) // 8, dtype=torch.float64, device=x.device)
    out = torch.empty_like(x)
    strm = torch.cuda.current_stream(x.device).cuda_stream
    _lib.check(lib.casync_op_audio_normalize(x.data_ptr(), x.numel(), ws.data_ptr(), out.data_ptr(), strm), "casync_op_audio_normalize")
    return (out, ws[:2]) if return_moments else out


def frontend_device(pcm: np.ndarray, rate: int, width: int, mono: str = "mean", device="cuda:0"):
    """The integers of read_pcm_wav -> (wave16k, normalised), fp32 tensors [ceil(frames up / down)] on `device`.  The PCM
    bytes go up once; decode, downmix, resampling and normalisation are HIP kernels (csrc/audio.hip)."""
    import torch
    check_mono(mono)
    pcm = np.asarray(pcm)
    pcm = pcm.reshape(len(pcm), -1)
    if pcm.shape[0] < 1:
        raise ValueError("the audio front end needs at least one frame")
    up, down = ratio(rate)
    raw = torch.from_numpy(pcm_bytes(pcm, width)).to(device)
    wave16k = resample_device(raw, width, pcm.shape[1], mono, up, down, None if up == down else taps_device(rate, device))
    return wave16k, normalize_device(wave16k)
