"""The audio front end without a GPU: the numpy twin of csrc/audio.hip (calipsync_amd/audio.py frontend_host) against scipy's
recorded and live float64 outputs, the filter design, the output lengths, the WAV reader, the 16 kHz identity and the value
errors of the new arguments.  The bound of the twin against scipy is 1e-12: both evaluate the same sums in float64 (a few
hundred terms below 1 in magnitude, 2e-16 each).  Parity with ffmpeg's and soxr's resamplers is pinned nowhere."""
import math
import os
import wave

import numpy as np
import pytest

from calipsync_amd import audio, hubert

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_resample_cases.npz")
RATES = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000)
MONO = ("mean", "first")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return [(tuple(int(v) for v in row), z[f"pcm_{i}"], z[f"y_{i}"]) for i, row in enumerate(z["meta"])]


def write_wav(path, pcm, rate, width):
    pcm = np.asarray(pcm)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(audio.pcm_bytes(pcm, width).tobytes())
    return str(path)


def test_the_fixture_covers_what_it_says(golden):
    meta = np.array([m for m, _, _ in golden])
    assert sorted(set(meta[:, 0])) == list(RATES)
    assert set(meta[:, 2]) == {1, 2, 3, 4} and set(meta[:, 3]) == {1, 2, 3} and set(meta[:, 4]) == {0, 1}
    assert {(c, m) for c, m in meta[:, 3:5]} == {(c, m) for c in (1, 2, 3) for m in (0, 1)}
    for rate in RATES:
        up, down = audio.ratio(rate)
        span = 2 * 10 * max(up, down) // up + 1
        ns = set(meta[meta[:, 0] == rate, 1])
        assert {1, 7, span - 1, span, span + 1} <= ns and max(ns) > 2500
    assert os.path.getsize(GOLDEN) < 400_000


def test_frontend_host_is_scipy_on_the_fixture(golden):
    worst = 0.0
    for (rate, n, width, channels, mono), pcm, y in golden:
        assert pcm.shape == (n, channels)
        got, norm = audio.frontend_host(pcm, rate, width, MONO[mono], exact=True)
        assert got.dtype == np.float64 and got.shape == y.shape == (audio.out_samples(n, rate),)
        worst = max(worst, float(np.abs(got - y).max()))
        ref = (y - y.mean()) / np.sqrt(y.var() + 1e-7)
        assert np.abs(norm - ref).max() <= 1e-12 * max(1.0, float(np.abs(ref).max()))
    print(f"frontend_host(exact) against the recorded scipy outputs: max |d| = {worst:.2e}")
    assert worst <= 1e-12


def test_frontend_host_is_live_scipy():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(5)
    for rate in RATES + (16001,):
        up, down = audio.ratio(rate)
        pcm = rng.integers(-32768, 32768, (1500 if rate != 16001 else 300, 2), dtype=np.int16)
        x = pcm.astype(np.float64).sum(axis=1) / 2 / 32768.0
        got, _ = audio.frontend_host(pcm, rate, 2, "mean", exact=True)
        assert np.abs(got - signal.resample_poly(x, up, down)).max() <= 1e-12
        taps = signal.firwin(2 * 10 * max(up, down) + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
        assert np.abs(audio.resample_taps(rate, np.float64) - taps).max() <= 1e-14


def test_the_rounded_twin_stays_at_fp32_distance_of_the_exact_one(golden):
    """what the device path is held to (tests/test_audio_gpu.py), met by the twin that rounds where the device rounds: per output
    (taps + C + 3) 2^-24 A[k], A the formula on the absolute values of the downmixed samples and of the taps"""
    for (rate, n, width, channels, mono), pcm, y in golden[::5]:
        up, down = audio.ratio(rate)
        got, _ = audio.frontend_host(pcm, rate, width, MONO[mono])
        assert got.dtype == np.float32
        x = np.abs(audio.downmix(audio.decode(pcm, width), MONO[mono]))
        t64 = audio.resample_taps(rate, np.float64)
        a = audio.resample_host(x, up, down, np.abs(t64))
        bar = (2 * (len(t64) // 2) // up + 1 + channels + 3) * 2.0 ** -24 * a
        assert (np.abs(got - y) <= bar).all(), (rate, n, width, channels)


def test_resample_host_keeps_the_tap_order_of_recorded_upfirdn():
    """resample_host is the reference of the GPU cases with random taps: here it is held to scipy.signal.upfirdn's recorded
    outputs with random ASYMMETRIC taps (a reversed or shifted tap index passes every symmetric filter)"""
    z = np.load(GOLDEN)
    assert len(z["asym_meta"]) >= 4
    for j, (up, down, n) in enumerate(z["asym_meta"].tolist()):
        taps, x, y = z[f"asym_taps_{j}"], z[f"asym_x_{j}"], z[f"asym_y_{j}"]
        assert len(x) == n and len(taps) % 2 == 1 and not np.allclose(taps, taps[::-1])
        got = audio.resample_host(x, up, down, taps)
        assert got.shape == y.shape == (-((-n * up) // down),) and np.abs(y).max() > 1
        assert np.abs(got - y).max() <= 1e-12 * np.abs(taps).sum()
        assert np.abs(audio.resample_host(x, up, down, taps[::-1]) - y).max() > 0.1           # the check can tell
        ks = np.arange(len(y))[::-3]
        assert np.array_equal(audio.resample_host(x, up, down, taps, ks), got[ks])


def test_resample_host_keeps_the_tap_order_of_live_upfirdn():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(8)
    for up, down, half, n in ((3, 7, 21, 400), (7, 3, 10, 250), (160, 441, 4410, 900), (2, 1, 0, 50), (5, 4, 33, 1)):
        taps, x = rng.standard_normal(2 * half + 1), rng.uniform(-1, 1, n)
        n_out = -((-n * up) // down)
        full = signal.upfirdn(np.concatenate([np.zeros(-half % down), taps]), x, up, down)  # zeros ahead: k down + half on the grid
        first = (half + -half % down) // down
        full = np.concatenate([full, np.zeros(max(0, first + n_out - len(full)))])
        assert np.abs(audio.resample_host(x, up, down, taps) - full[first:first + n_out]).max() <= 1e-12 * np.abs(taps).sum()


@pytest.mark.parametrize("rate", RATES + (16001, 22051))
def test_taps(rate):
    up, down = audio.ratio(rate)
    assert (up, down) == (16000 // math.gcd(rate, 16000), rate // math.gcd(rate, 16000))
    half = 10 * max(up, down)
    t64, t32 = audio.resample_taps(rate, np.float64), audio.resample_taps(rate)
    assert t64.shape == t32.shape == (2 * half + 1,) and t32.dtype == np.float32
    assert np.array_equal(t32, t64.astype(np.float32))                 # rounded once
    assert np.array_equal(t64, t64[::-1]) or np.abs(t64 - t64[::-1]).max() < 1e-15
    assert abs(t64.sum() - up) <= 1e-9 * up                            # unit gain after the zero stuffing
    assert t64[half] == t64.max()
    # the formula, evaluated tap by tap with math only
    w_sum = (np.sinc(np.arange(-half, half + 1) / max(up, down)) / max(up, down) * np.kaiser(2 * half + 1, 5.0)).sum()
    for m in (0, 1, half // 3, half):
        x = m / max(up, down)
        sinc = 1.0 if m == 0 else math.sin(math.pi * x) / (math.pi * x)
        alpha = half
        kaiser = float(np.i0(5.0 * math.sqrt(max(0.0, 1 - ((m) / alpha) ** 2))) / np.i0(5.0))
        assert abs(t64[half + m] - up * sinc / max(up, down) * kaiser / w_sum) <= 1e-12 * up


def test_sixteen_khz_has_no_filter():
    assert audio.ratio(16000) == (1, 1) and np.array_equal(audio.resample_taps(16000), np.ones(1, np.float32))
    rng = np.random.default_rng(2)
    for width, lim, dt in ((1, None, np.uint8), (2, 1 << 15, np.int16), (3, 1 << 23, np.int32), (4, 1 << 31, np.int32)):
        pcm = rng.integers(0, 256, (999, 1), dtype=np.uint8) if lim is None else rng.integers(-lim, lim, (999, 1)).astype(dt)
        y, norm = audio.frontend_host(pcm, 16000, width)
        assert y.dtype == np.float32 and np.array_equal(y, audio.decode(pcm, width)[:, 0].astype(np.float32))
        x = y.astype(np.float64)                       # the normalise bar: four roundings and two of slack, against float64
        r = 1.0 / np.sqrt(x.var() + 1e-7)
        assert norm.dtype == np.float32 and (np.abs(norm - (x - x.mean()) * r) <= 6 * 2.0 ** -24 * (np.abs(x) + abs(x.mean())) * r).all()


def test_output_lengths_agree_with_the_library():
    from calipsync_amd import _lib, build
    build.build()
    lib = _lib.load()
    for rate in RATES + (16000, 16001, 7, 192000):
        up, down = audio.ratio(rate)
        for n in (0, 1, 2, 7, down - 1, down, down + 1, 2999, 13_500_000, 1 << 33):
            want = -((-n * up) // down)
            assert audio.out_samples(n, rate) == want == lib.casync_audio_out_samples(n, rate), (rate, n)
    assert lib.casync_audio_out_samples(-1, 16000) == -1 and lib.casync_audio_out_samples(5, 0) == -1
    assert lib.casync_op_audio_workspace_bytes(0) == -1 and lib.casync_op_audio_workspace_bytes(1) > 0
    assert lib.casync_op_audio_workspace_bytes(1) % 8 == 0


def test_the_entries_refuse_bad_arguments_before_any_launch():
    """no GPU needed: every one of these returns before the first device call (the pointers are never followed)"""
    from calipsync_amd import _lib, build
    build.build()
    lib = _lib.load()
    p = 1 << 20                                    # a made-up non-null, aligned address
    ok = dict(pcm=p, width=2, channels=1, frames=441, mono=0, up=160, down=441, taps=p, n_taps=8821, out=p, n_out=160)
    for change, word in ((dict(pcm=0), "null"), (dict(out=0), "null"), (dict(width=0), "bytes"), (dict(width=5), "bytes"),
                         (dict(channels=0), "channels"), (dict(channels=17), "channels"), (dict(mono=2), "mono"), (dict(up=0), "up"),
                         (dict(frames=0), "frames"), (dict(n_out=161), "n_out"), (dict(taps=0), "taps"), (dict(n_taps=8820), "taps"),
                         (dict(down=16 * 441 * 160, n_out=1, n_taps=1), "reaches"), (dict(out=p + 2), "aligned")):
        a = dict(ok, **change)
        st = lib.casync_op_audio_resample(a["pcm"], a["width"], a["channels"], a["frames"], a["mono"], a["up"], a["down"], a["taps"],
                                          a["n_taps"], a["out"], a["n_out"], None)
        assert st < 0 and word in lib.casync_last_error().decode(), (change, lib.casync_last_error())
    for x, n, ws, out, word in ((0, 4, p, p, "null"), (p, 0, p, p, "samples"), (p, 4, 0, p, "null"), (p, 4, p + 4, p, "8-byte"),
                                (p + 1, 4, p, p, "4-byte")):
        assert lib.casync_op_audio_normalize(x, n, ws, out, None) < 0 and word in lib.casync_last_error().decode()


@pytest.mark.parametrize("width", [1, 2, 3, 4])
@pytest.mark.parametrize("rate,channels", [(8000, 1), (24000, 2), (44100, 3)])
def test_read_pcm_wav_reads_any_rate(tmp_path, width, rate, channels):
    rng = np.random.default_rng(width * 10 + channels)
    lim = 1 << (8 * width - 1)
    pcm = rng.integers(0, 256, (321, channels)) if width == 1 else rng.integers(-lim, lim, (321, channels))
    pcm[0, 0] = 0 if width == 1 else -lim                 # the extremes
    pcm[1, 0] = 255 if width == 1 else lim - 1
    path = write_wav(tmp_path / "a.wav", pcm, rate, width)
    got, got_rate, got_width = audio.read_pcm_wav(path)
    assert (got_rate, got_width) == (rate, width) and got.shape == (321, channels)
    assert got.dtype == {1: np.uint8, 2: np.int16, 3: np.int32, 4: np.int32}[width]
    assert np.array_equal(got, pcm)
    assert np.array_equal(audio.pcm_bytes(got, width), audio.pcm_bytes(pcm, width))
    x = audio.decode(got, width)
    assert x.min() == -1.0 and x.max() == (lim - 1) / lim


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_decode_is_read_wav_at_16_khz(tmp_path, width):
    rng = np.random.default_rng(width)
    lim = 1 << (8 * width - 1)
    pcm = rng.integers(0, 256, (200, 2)) if width == 1 else rng.integers(-lim, lim, (200, 2))
    path = write_wav(tmp_path / "a.wav", pcm, 16000, width)
    got, rate, w = audio.read_pcm_wav(path)
    assert np.array_equal(audio.decode(got, w), hubert.read_wav(path))
    with pytest.raises(ValueError, match="8000 Hz"):      # read_wav keeps refusing other rates
        hubert.read_wav(write_wav(tmp_path / "b.wav", pcm, 8000, width))


def test_read_pcm_wav_refuses_what_it_cannot_read(tmp_path):
    bad = tmp_path / "x.wav"
    bad.write_bytes(b"not a wav file at all")
    with pytest.raises((wave.Error, EOFError)):
        audio.read_pcm_wav(str(bad))
    with pytest.raises(ValueError):
        audio.pcm_bytes(np.zeros((4, 1), np.float32), 2)
    with pytest.raises(ValueError):
        audio.pcm_bytes(np.zeros((4, 1), np.int16), 5)


def test_downmix_modes():
    x = np.array([[0.5, -0.25, 0.125], [1.0, 1.0, -0.5]])
    assert np.array_equal(audio.downmix(x, "mean"), np.array([0.375 / 3, 0.5]))
    assert np.array_equal(audio.downmix(x, "first"), np.array([0.5, 1.0]))
    pcm = np.array([[100, -100], [7, 9]], dtype=np.int16)
    assert np.array_equal(audio.frontend_host(pcm, 16000, 2, "mean")[0], np.float32([0.0, 8 / 32768]))
    assert np.array_equal(audio.frontend_host(pcm, 16000, 2, "first")[0], np.float32([100 / 32768, 7 / 32768]))


def test_frontend_and_mono_values_are_checked_before_anything_else(tmp_path):
    from calipsync_amd.frame_synth import VideoStreamManager
    missing = str(tmp_path / "no_such_checkpoint")
    with pytest.raises(ValueError, match="front end"):
        hubert.HubertExtractor(missing, "cuda:0", "fp32", frontend="ffmpeg")
    with pytest.raises(ValueError, match="mono"):
        hubert.HubertExtractor(missing, "cuda:0", "fp32", frontend="device", mono="left")
    with pytest.raises(ValueError, match="mono"):
        hubert.HubertExtractor(missing, "cuda:0", "fp32", mono="sum")
    with pytest.raises(FileNotFoundError):                 # both values good: the checkpoint is looked for next
        hubert.HubertExtractor(missing, "cuda:0", "fp32", frontend="device", mono="first")
    with pytest.raises(ValueError, match="front end"):
        VideoStreamManager(missing, None, hubert_frontend="gpu")
    pcm = np.zeros((10, 1), np.int16)
    for call in (audio.frontend_host, audio.frontend_device):
        with pytest.raises(ValueError, match="mono"):
            call(pcm, 24000, 2, "both")
    with pytest.raises(ValueError):
        audio.ratio(0)
    assert audio.check_frontend("reference") == "reference" and audio.check_mono("first") == 1


def test_chunked_features_keep_device_is_the_same_tensor():
    """one chunk/pad/trim routine: keep_device only leaves out the download"""
    import torch
    calls = []

    def encode(chunks):      # values that tell the chunks, their rows and their columns apart, the same at every call
        calls.append([c.shape[1] for c in chunks])
        return [float(c[0, 0]) + torch.arange(hubert.tokens(c.shape[1]) * 1024, dtype=torch.float32).reshape(-1, 1024) / 1024
                for c in chunks]

    x = torch.arange(hubert.CLIP + 5000, dtype=torch.float32)[None]
    a = hubert.chunked_features(x, encode)
    b = hubert.chunked_features(x, encode, keep_device=True)
    assert a.shape == b.shape and a.shape[1:] == (2, 1024) and torch.equal(a, b) and calls[:2] == calls[2:] and len(calls) == 4
    assert a[0, 0, 0] == 0 and a[0, 1, 1] == 1 + 1 / 1024 and a[-1, -1, 0] > hubert.CLIP      # both chunks are in it
