"""The ledger of calipsync_amd/lib/obj_audio/ (the audio front end, csrc/audio.hip), under the rule of tests/kernel_ledger.py:
every compiled kernel instance has op-level cases that launch it through its casync_op_* entry with the launch log on.

The bars are derived, not measured.  An error is reported as a fraction of its bar (the bar of every case is 1), inf where a
sentinel around the output changed or a value is not finite.
  resample / convert: per output |y - ref| <= (T + C + 3) 2^-24 A[k]: the forward error of a length-T fp32 dot product plus one
    rounding each for the taps, the sample conversion and the C-channel mean; T the taps an output can reach, A[k] the formula
    on absolute values: sum_i |x_i| |h|, x_i the DOWNMIXED sample (the mean of the channels, or channel 0); ref the formula in
    float64 (real taps: the float64 design; random taps: the fp32 values themselves).  One channel (or mono "first") at
    up == down is a copy of exact values: the bar is 0, the output must be equal.
    One class of input cannot meet a bar relative to |x_i| and is held to another: 32-bit samples, several channels, "mean", and
    no filter (up == down, T = 1).  Only a 32-bit sample is rounded when it becomes fp32, by up to 2^-24 of THAT sample, and the
    partial channel sums round relative to themselves; where the channels cancel, the mean is far below either, and with one tap
    nothing averages that out (the fp32 arithmetic the kernel is given reaches hundreds of times (1 + C + 3) 2^-24 |x_i| on
    random stereo input).  There the conversions, the C - 1 sums and the division are each within 2^-24 mean_c |x_c|, C + 1
    roundings in all, and the bar is (1 + C + 3) 2^-24 mean_c |x_c|.  Through a filter the same input keeps the bar above.
  normalise: against float64 on the kernel's own fp32 input, per sample 6 2^-24 (|x| + |mean|) r, r = (var + 1e-7)^-1/2: the four
    roundings of mean, difference, r and product, plus two of slack; mean and variance read back from the workspace agree with
    numpy's float64 to 1e-12 (relative to mean |x| and mean x^2); a second call returns the same bits.
Nothing here touches a GPU at import."""
from __future__ import annotations

import math

import numpy as np

from kernel_ledger import C, _done, _lib, _ok, _Run, _s, _t

OUT_PER_WG = 512          # csrc/audio.hip: outputs of one workgroup of the resample kernel
CONVERT_PER_WG = 4096     # frames of one workgroup of the convert kernel
MOMENT_SPAN = 4096        # samples of one moments block, until there are 512 of them
PAD = 64                  # sentinel floats on either side of an output
SENTINEL = -777.0
MONO = ("mean", "first")


def _rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _pcm(rng, n, channels, width):
    if width == 1:
        return rng.integers(0, 256, (n, channels), dtype=np.uint8)
    lim = 1 << (8 * width - 1)
    return rng.integers(-lim, lim, (n, channels), dtype=np.int64).astype(np.int16 if width == 2 else np.int32)


def frames_for(n_out, rate):
    """the most frames at `rate` that give n_out samples at 16 kHz"""
    up, down = _ratio(rate)
    return (n_out * down) // up


def _ratio(rate):
    g = math.gcd(rate, 16000)
    return 16000 // g, rate // g


def _ratio_error(got, ref, bar):
    d = np.abs(got.astype(np.float64) - ref)
    if not np.isfinite(got).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bar > 0, d / bar, np.where(d == 0, 0.0, np.inf))
    return float(frac.max()) if frac.size else 0.0


def _front(width, up, down, n, channels, mono, taps64, taps32, offset):
    """casync_op_audio_resample on seeded PCM at a byte offset into its buffer -> (error as a fraction of the bar, n_out)"""
    from calipsync_amd import audio
    torch = _t()
    rng = _rng("pcm", width, up, down, n, channels, mono, offset)
    pcm = _pcm(rng, n, channels, width)
    raw = audio.pcm_bytes(pcm, width)
    buf = torch.zeros(offset + raw.size + 16, dtype=torch.uint8, device="cuda:0")
    buf[offset:offset + raw.size] = torch.from_numpy(raw).to("cuda:0")
    n_out = -((-n * up) // down)
    out = torch.full((n_out + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda:0")
    taps_dev = None if taps32 is None else torch.from_numpy(taps32).to("cuda:0")
    _ok(_lib().casync_op_audio_resample(buf.data_ptr() + offset, width, channels, n, audio.MONO[mono], up, down,
                                        0 if taps_dev is None else taps_dev.data_ptr(), 0 if taps_dev is None else taps_dev.numel(),
                                        out.data_ptr() + 4 * PAD, n_out, _s()), "casync_op_audio_resample")
    got = out.cpu().numpy()
    if not (got[:PAD] == SENTINEL).all() or not (got[PAD + n_out:] == SENTINEL).all():
        return float("inf"), n_out
    x = audio.downmix(audio.decode(pcm, width), mono)
    ref = audio.resample_host(x, up, down, taps64)
    a = audio.resample_host(np.abs(x), up, down, np.abs(taps64))
    reach = (len(taps64) - 1) // up + 1
    exact = up == down and (channels == 1 or mono == "first") and width < 4
    if up == down and width == 4 and channels > 1 and mono == "mean":       # no tap averages a cancellation out: see above
        a = audio.downmix(np.abs(audio.decode(pcm, width)), mono)
    bar = np.zeros_like(a) if exact else (reach + channels + 3) * 2.0 ** -24 * a
    return _ratio_error(got[PAD:PAD + n_out], ref, bar), n_out


def resample(width, rate, n, channels=1, mono="mean", offset=0):
    """the real taps of `rate` (calipsync_amd/audio.py resample_taps): reference with the float64 design"""
    from calipsync_amd import audio
    up, down = _ratio(rate)
    with _Run(0) as r:
        err, n_out = _front(width, up, down, n, channels, mono, audio.resample_taps(rate, np.float64), audio.resample_taps(rate), offset)
    return _done(r, err, 1.0, f"{8 * width}-bit x {channels} ({mono}) {rate} Hz, {n} frames at byte {offset} -> {n_out}")


def resample_random_taps(width, up, down, n_taps, n, channels=1, mono="mean"):
    """random ASYMMETRIC taps: the real ones are symmetric, which hides a reversed tap order"""
    taps32 = _rng("taps", up, down, n_taps).standard_normal(n_taps).astype(np.float32)
    with _Run(0) as r:
        err, n_out = _front(width, up, down, n, channels, mono, taps32.astype(np.float64), taps32, 0)
    return _done(r, err, 1.0, f"{8 * width}-bit x {channels} ({mono}) {up}/{down}, {n_taps} random taps, {n} frames -> {n_out}")


def convert(width, n, channels=1, mono="mean", offset=0):
    """up == down: the decode and downmix alone, no taps"""
    with _Run(0) as r:
        err, n_out = _front(width, 1, 1, n, channels, mono, np.ones(1), None, offset)
    return _done(r, err, 1.0, f"{8 * width}-bit x {channels} ({mono}) 16000 Hz, {n} frames at byte {offset}")


def normalize(n, kind="noise", misalign=0, in_place=False):
    """casync_op_audio_normalize: the two moments kernels and the normalise kernel in one call"""
    torch = _t()
    rng = _rng("norm", n, kind)
    if kind == "noise":
        x = (0.3 * rng.standard_normal(n) + 0.05).astype(np.float32)
    elif kind == "offset":           # a DC offset far above the signal
        x = (0.75 + 1e-3 * rng.standard_normal(n)).astype(np.float32)
    else:                            # constant: variance 0
        x = np.full(n, 0.3125, dtype=np.float32)
    xd = torch.zeros(n + 4, dtype=torch.float32, device="cuda:0")
    xd[misalign:misalign + n] = torch.from_numpy(x).to("cuda:0")
    lib = _lib()
    ws = torch.zeros(lib.casync_op_audio_workspace_bytes(n) // 8, dtype=torch.float64, device="cuda:0")
    outs = []
    with _Run(0) as r:
        for _ in range(2):
            out = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda:0")
            if in_place:
                out[PAD + misalign:PAD + misalign + n] = torch.from_numpy(x).to("cuda:0")
            src = out.data_ptr() + 4 * (PAD + misalign) if in_place else xd.data_ptr() + 4 * misalign
            _ok(lib.casync_op_audio_normalize(src, n, ws.data_ptr(), out.data_ptr() + 4 * (PAD + misalign), _s()), "casync_op_audio_normalize")
            outs.append(out.cpu().numpy())
    a, b = outs
    got = a[PAD + misalign:PAD + misalign + n]
    x64 = x.astype(np.float64)
    mean, var = x64.mean(), x64.var()
    rstd = 1.0 / np.sqrt(var + 1e-7)
    err = _ratio_error(got, (x64 - mean) * rstd, 6 * 2.0 ** -24 * (np.abs(x64) + abs(mean)) * rstd)
    if not (a[:PAD + misalign] == SENTINEL).all() or not (a[PAD + misalign + n:] == SENTINEL).all():
        err = float("inf")
    if a.tobytes() != b.tobytes():                                   # bit-identical from call to call
        err = float("inf")
    m = ws[:2].cpu().numpy()
    moments = max(abs(m[0] - mean) / np.abs(x64).mean(), abs(m[1] - var) / (x64 * x64).mean()) / 1e-12
    return _done(r, max(err, moments), 1.0, f"normalise {n} samples ({kind}{', in place' if in_place else ''}) at float {misalign}")


_TWO_TILES = 2 * OUT_PER_WG + 3
# output counts around a workgroup's 512 and two tiles + 3, one frame, fewer frames than a span, upsampling (8000, 11025), 16001 Hz
# (16000 distinct phases), three channels in both modes, byte offsets that take the vector path with a head (2, 4) or leave it (1, 3)
LEDGER = {
    "wav_resample_kernel<1>": [C(resample, 1, 48000, frames_for(OUT_PER_WG + 1, 48000)), C(resample, 1, 8000, 700, 2), C(resample, 1, 44100, 1500, 3),
                               C(resample, 1, 22050, 900, 3, "first"), C(resample, 1, 24000, 777, 1, "mean", 3),
                               C(resample_random_taps, 1, 3, 7, 41, 1300, 2)],
    "wav_resample_kernel<2>": [C(resample, 2, 44100, frames_for(n_out, 44100)) for n_out in (OUT_PER_WG - 1, OUT_PER_WG, OUT_PER_WG + 1, _TWO_TILES)] +
                              [C(resample, 2, 44100, 1), C(resample, 2, 48000, 7), C(resample, 2, 44100, 30, 2), C(resample, 2, 8000, 601),
                               C(resample, 2, 11025, 803), C(resample, 2, 16001, 3000), C(resample, 2, 32000, 1001, 3),
                               C(resample, 2, 32000, 1001, 3, "first"), C(resample, 2, 24000, 2000, 2, "mean", 2), C(resample, 2, 24000, 999, 1, "mean", 1),
                               C(resample, 2, 96000, 7000, 4), C(resample_random_taps, 2, 160, 441, 8821, 3000),
                               C(resample_random_taps, 2, 7, 3, 40 + 1, 1100), C(resample_random_taps, 2, 2, 1, 1, 600)],
    "wav_resample_kernel<3>": [C(resample, 3, 44100, frames_for(_TWO_TILES, 44100)), C(resample, 3, 11025, 500, 2), C(resample, 3, 12000, 1),
                               C(resample, 3, 48000, 1600, 3), C(resample, 3, 48000, 1600, 3, "first"), C(resample, 3, 22050, 40, 1, "mean", 1),
                               C(resample_random_taps, 3, 5, 2, 101, 900, 2, "first")],
    "wav_resample_kernel<4>": [C(resample, 4, 24000, frames_for(OUT_PER_WG + 1, 24000)), C(resample, 4, 16001, 3000, 2, "first"),
                               C(resample, 4, 8000, 5), C(resample, 4, 44100, 1234, 3), C(resample, 4, 48000, 3000, 2, "mean", 4),
                               C(resample, 4, 96000, 6200, 4, "mean", 16), C(resample_random_taps, 4, 3, 4, 33, 1500, 3)],
    "wav_convert_kernel<1>": [C(convert, 1, n) for n in (1, CONVERT_PER_WG + 1)] + [C(convert, 1, 5000, 3), C(convert, 1, 4100, 2, "first", 5),
                                                                                    C(convert, 1, 9000, 16)],
    "wav_convert_kernel<2>": [C(convert, 2, n) for n in (1, 7, CONVERT_PER_WG - 1, CONVERT_PER_WG, CONVERT_PER_WG + 1, 2 * CONVERT_PER_WG + 3)] +
                             [C(convert, 2, 4099, 2), C(convert, 2, 4099, 2, "first"), C(convert, 2, 4099, 3), C(convert, 2, 4099, 3, "first"),
                              C(convert, 2, 5001, 1, "mean", 1), C(convert, 2, 5001, 1, "mean", 6), C(convert, 2, 5001, 8, "mean", 16)],
    "wav_convert_kernel<3>": [C(convert, 3, n) for n in (1, CONVERT_PER_WG + 1)] + [C(convert, 3, 4500, 3), C(convert, 3, 4500, 2, "first", 2)],
    "wav_convert_kernel<4>": [C(convert, 4, n) for n in (1, CONVERT_PER_WG + 1)] + [C(convert, 4, 4500, 2), C(convert, 4, 4500, 3, "first"),
                                                                                    C(convert, 4, 4500, 4, "mean", 4), C(convert, 4, 4500, 1, "mean", 2)],
}
# one entry, three kernels: 1 .. 3 samples (no vector), the block span and one past it, many blocks, past 512 blocks (the span
# grows), every n % 4, a misaligned buffer (the scalar path), in place, a DC offset, variance 0
_NORMALIZE = [C(normalize, n) for n in (1, 3, 4, MOMENT_SPAN, MOMENT_SPAN + 1, 3 * MOMENT_SPAN + 2, 300_007, 512 * MOMENT_SPAN + 7)] + \
             [C(normalize, 70_001, "noise", 1), C(normalize, 5, "noise", 3), C(normalize, 50_002, "noise", 0, True),
              C(normalize, 50_003, "noise", 1, True), C(normalize, 100_000, "offset"), C(normalize, 33_333, "constant")]
LEDGER["wav_moments_kernel"] = _NORMALIZE
LEDGER["wav_moments_final_kernel"] = _NORMALIZE
LEDGER["wav_normalize_kernel"] = _NORMALIZE


def cases():
    """[(kernel, index, case)] in ledger order: one GPU test each"""
    return [(name, i, c) for name, cs in LEDGER.items() for i, c in enumerate(cs)]


def launched_by(case):
    """the kernels a case is listed under: what its entry launches"""
    return {name for name, cs in LEDGER.items() if case in cs}
