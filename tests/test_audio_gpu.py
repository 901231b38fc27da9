"""-m gpu: the device audio front end (calipsync_amd/audio.py frontend_device, csrc/audio.hip) against scipy's recorded float64
outputs, across 2^31 in k * down, and through HubertExtractor(frontend="device") and VideoStreamManager(hubert_frontend="device").

The bars are those of tests/kernel_ledger_audio.py, derived and not measured: a resampled sample within (T + C + 3) 2^-24 A[k] of
the float64 formula (T the taps an output can reach, A[k] the formula on the absolute values of the downmixed samples and of the
taps), a normalised one within
6 2^-24 (|x| + |mean|) r of float64 on the kernel's own fp32 waveform."""
import os
import wave

import numpy as np
import pytest
import torch

import hubert_ref
from calipsync_amd import audio, hubert

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_resample_cases.npz")
MONO = ("mean", "first")
DEV = "cuda:0"


def resample_bar(x_abs, rate, channels, ks=None):
    """x_abs: |downmixed samples|"""
    up, down = audio.ratio(rate)
    t64 = audio.resample_taps(rate, np.float64)
    reach = (len(t64) - 1) // up + 1
    return (reach + channels + 3) * 2.0 ** -24 * audio.resample_host(x_abs, up, down, np.abs(t64), ks)


def normalize_check(wave16k, normalised):
    """-> the worst |got - float64| as a fraction of 6 2^-24 (|x| + |mean|) r, on the waveform the kernel read"""
    x = wave16k.astype(np.float64)
    mean, var = x.mean(), x.var()
    r = 1.0 / np.sqrt(var + 1e-7)
    bar = 6 * 2.0 ** -24 * (np.abs(x) + abs(mean)) * r
    return float((np.abs(normalised.astype(np.float64) - (x - mean) * r) / bar).max())


def write_wav(path, pcm, rate, width):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(audio.pcm_bytes(pcm, width).tobytes())
    return str(path)


def test_device_frontend_against_the_recorded_scipy_outputs():
    z = np.load(GOLDEN)
    worst_y = worst_n = 0.0
    for i, (rate, n, width, channels, mono) in enumerate(z["meta"].tolist()):
        pcm, y = z[f"pcm_{i}"], z[f"y_{i}"]
        wave16k, normalised = (t.cpu().numpy() for t in audio.frontend_device(pcm, rate, width, MONO[mono], DEV))
        assert wave16k.dtype == normalised.dtype == np.float32 and wave16k.shape == normalised.shape == y.shape
        assert np.isfinite(wave16k).all() and np.isfinite(normalised).all()
        bar = resample_bar(np.abs(audio.downmix(audio.decode(pcm, width), MONO[mono])), rate, channels)
        d = np.abs(wave16k.astype(np.float64) - y)
        assert (d <= bar).all(), (i, rate, n, width, channels, mono, float((d / np.maximum(bar, 1e-300)).max()))
        worst_y = max(worst_y, float((d[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0)
        worst_n = max(worst_n, normalize_check(wave16k, normalised))
        again = audio.frontend_device(pcm, rate, width, MONO[mono], DEV)                   # the same bits on a second call
        assert again[0].cpu().numpy().tobytes() == wave16k.tobytes() and again[1].cpu().numpy().tobytes() == normalised.tobytes()
    print(f"device front end on {len(z['meta'])} recorded cases: resample {worst_y:.3f} of its bar, normalise {worst_n:.3f} of its bar")
    assert worst_n <= 1.0


def test_indices_past_2_to_the_31():
    """13.5 M samples at 44.1 kHz: k * 441 passes 2^31 at k = 4,869,577, where a resampler with 32-bit indices goes wrong"""
    rate, n = 44100, 13_500_000
    up, down = audio.ratio(rate)
    pcm = np.random.default_rng(31).integers(-32768, 32768, (n, 1), dtype=np.int16)
    wave16k, normalised = audio.frontend_device(pcm, rate, 2, "mean", DEV)
    n_out = audio.out_samples(n, rate)
    k_c = (1 << 31) // down
    assert wave16k.shape == (n_out,) and k_c + 1024 < n_out - 2048 and (k_c + 1) * down > 1 << 31
    x = audio.decode(pcm, 2)[:, 0]
    t64 = audio.resample_taps(rate, np.float64)
    for ks in (np.arange(k_c - 1024, k_c + 1024), np.arange(n_out - 2048, n_out)):
        got = wave16k[int(ks[0]):int(ks[-1]) + 1].cpu().numpy().astype(np.float64)
        ref = audio.resample_host(x, up, down, t64, ks)
        bar = resample_bar(np.abs(x), rate, 1, ks)
        assert np.abs(ref).max() > 0.1 and (np.abs(got - ref) <= bar).all(), float((np.abs(got - ref) / bar).max())
    y = wave16k.cpu().numpy()                                         # and the normalisation of all 4.9 M samples
    assert np.isfinite(y).all() and normalize_check(y, normalised.cpu().numpy()) <= 1.0


def test_sixteen_khz_is_the_reference_waveform(tmp_path):
    """a 16 kHz mono i16 file: the device path's normalised waveform within the normalise bar of float64 normalize(read_wav())"""
    pcm = (hubert_ref.golden_wave(16000, 41) * 32767).astype("<i2")[:, None]
    path = write_wav(tmp_path / "a.wav", pcm, 16000, 2)
    got_pcm, rate, width = audio.read_pcm_wav(path)
    wave16k, normalised = (t.cpu().numpy() for t in audio.frontend_device(got_pcm, rate, width, "mean", DEV))
    x = hubert.read_wav(path)
    assert np.array_equal(wave16k, x.astype(np.float32)) and np.array_equal(wave16k.astype(np.float64), x)
    mean, var = x.mean(), x.var()
    r = 1.0 / np.sqrt(var + 1e-7)
    assert (np.abs(normalised - (x - mean) * r) <= 6 * 2.0 ** -24 * (np.abs(x) + abs(mean)) * r).all()


@pytest.fixture(scope="module")
def stereo_24k(tmp_path_factory):
    from test_hubert import write_checkpoint
    tmp = tmp_path_factory.mktemp("audio_gpu")
    ckpt = write_checkpoint(str(tmp / "hubert"), 2)
    mono = hubert_ref.golden_wave(24000, 43)
    pcm = np.stack([mono * 30000, np.roll(mono, 5) * 20000], axis=1).astype("<i2")
    return tmp, ckpt, write_wav(tmp / "a.wav", pcm, 24000, 2)


def test_hubert_extractor_device_frontend(stereo_24k):
    tmp, ckpt, wav = stereo_24k
    ext = hubert.HubertExtractor(ckpt, DEV, frontend="device")
    feats = ext.extract_from_file(wav)
    assert isinstance(feats, np.ndarray) and feats.shape == (24, 2, 1024) and feats.dtype == np.float32
    pcm, rate, width = audio.read_pcm_wav(wav)
    assert (rate, width) == (24000, 2) and pcm.shape == (24000, 2)
    _, normalised = audio.frontend_device(pcm, rate, width, "mean", DEV)
    assert normalised.shape == (16000,)
    host = hubert.chunked_features(normalised.cpu()[None], ext._encode)       # the existing host routine, fed the device waveform
    assert host.device.type == "cpu" and host.numpy().tobytes() == feats.tobytes()
    on_dev = ext.extract_features_device(wav)
    assert on_dev.device.type == "cuda" and on_dev.shape == (24, 2, 1024) and on_dev.cpu().numpy().tobytes() == feats.tobytes()
    first = hubert.HubertExtractor(ckpt, DEV, frontend="device", mono="first").extract_from_file(wav)
    assert first.shape == feats.shape and not np.array_equal(first, feats)   # channel 0 alone is another waveform
    with pytest.raises(ValueError, match='frontend="device"'):               # the reference front end has no device waveform
        hubert.HubertExtractor(ckpt, DEV).extract_features_device(wav)


def test_video_stream_manager_device_frontend(stereo_24k):
    """VideoStreamManager(hubert_frontend="device") yields the frames of the same features passed as .npy"""
    tmp, ckpt, wav = stereo_24k
    from frame_data import write_dataset
    from calipsync_amd import mjpeg_avi, recipe
    from calipsync_amd.frame_synth import VideoStreamManager
    from calipsync_amd.unet import Model
    net = Model(6, "hubert").to(DEV)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe.make_state_dict().items()})
    net.eval()
    data = tmp / "data"
    write_dataset(str(data), 6, 270, 360, seed=4)
    vsm = VideoStreamManager(str(data), None, hubert_path=ckpt, device=DEV, batch_size=4, seed=9, net=net, hubert_frontend="device")
    out_a = vsm.process_single_file(wav, str(tmp / "a.mp4"))
    feats = hubert.HubertExtractor(ckpt, DEV, frontend="device").extract_from_file(wav)
    np.save(str(tmp / "f.npy"), feats)
    vsm2 = VideoStreamManager(str(data), None, device=DEV, batch_size=4, seed=9, net=net)
    out_b = vsm2.process_single_file(str(tmp / "f.npy"), str(tmp / "b.mp4"))
    if out_a.endswith(".avi"):
        fa, fb = mjpeg_avi.read_mjpeg_avi(out_a)[1], mjpeg_avi.read_mjpeg_avi(out_b)[1]
        assert len(fa) == len(fb) == 24 and all(np.array_equal(a, b) for a, b in zip(fa, fb))
    else:
        assert os.path.getsize(out_a) > 0 and os.path.getsize(out_b) > 0
    # the frame loop takes the device tensor as it is: the same frames as the host array of the same features
    fresh = lambda: VideoStreamManager(str(data), None, device=DEV, batch_size=4, seed=9, net=net).synthesizer   # the walk starts over
    frames_dev = [f["frame"] for f in fresh().iterate_synthesized_frames(torch.from_numpy(feats).to(DEV), 0, True)]
    frames_host = [f["frame"] for f in fresh().iterate_synthesized_frames(feats, 0, True)]
    assert len(frames_dev) == len(frames_host) == 24 and all(np.array_equal(a, b) for a, b in zip(frames_dev, frames_host))
