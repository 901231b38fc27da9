"""The audio leg of one utterance on one MI355X: from a WAV file to HuBERT features, through the "reference" front end (ffmpeg to
16 kHz, host normalisation, upload) and through the "device" one (calipsync_amd/audio.py: the PCM bytes uploaded once; decode,
downmix, resampling and normalisation as HIP kernels), in one process.

    python tools/audio_bench.py [--layers 24] [--precision bf16] [--rounds 7] [--warmup 2] [--seconds 60] [--out profiles/audio_frontend.json]

Input: `--seconds` of mono 16-bit audio at 24, 44.1 and 48 kHz, and stereo at 48 kHz, written to a temporary directory.  Per
input one JSON line:
  reference_*      load_audio_16k + normalize + upload, where ffmpeg exists ("reference": "ffmpeg"); otherwise "reference":
                   "not available" and no figure (without ffmpeg the reference path reads 16 kHz files only)
  device_upload_*  the PCM bytes host -> device
  device_kernels_* the resample and normalise entries on bytes already on the device
  device_frontend_* read_pcm_wav + upload + kernels: what stands in for the reference figure
  device_e2e_*     the file -> features [T/2,2,1024] on the device (HubertExtractor.extract_features_device)
  hubert_*         the chunked HuBERT forward alone, on a normalised waveform already on the device
The two front ends alternate round by round after `--warmup` rounds; every figure is the median of `--rounds` rounds with its
range (_min, _max), each round timed between two device synchronisations.  --out writes the lines with source_hash.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

INPUTS = ((24000, 1), (44100, 1), (48000, 1), (48000, 2))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(prefix, ms):
    return {f"{prefix}_ms": statistics.median(ms), f"{prefix}_ms_min": min(ms), f"{prefix}_ms_max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--precision", default="bf16", choices=("fp32", "bf16"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds: at least 5")
    import hubert_ref
    from calipsync_amd import audio, build, hubert
    dev = "cuda:0"
    ext = hubert.HubertExtractor.__new__(hubert.HubertExtractor)       # the extractor around a recipe engine: no checkpoint directory
    ext.model = hubert.HubertEngine(hubert_ref.recipe_state_dict(a.layers), a.layers, dev, a.precision)
    ext.device, ext.frontend, ext.mono, ext.do_normalize = dev, "device", "mean", True
    have_ffmpeg = shutil.which("ffmpeg") is not None
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for rate, channels in INPUTS:
            n = int(round(a.seconds * rate))
            mono = hubert_ref.golden_wave(n, 60 + channels)
            pcm = np.stack([np.roll(mono, 7 * c) * (30000 - 5000 * c) for c in range(channels)], axis=1).astype("<i2")
            path = os.path.join(tmp, f"a_{rate}_{channels}.wav")
            with wave.open(path, "wb") as w:
                w.setnchannels(channels)
                w.setsampwidth(2)
                w.setframerate(rate)
                w.writeframes(pcm.tobytes())
            raw_host = torch.from_numpy(audio.pcm_bytes(pcm, 2))
            raw_dev = raw_host.to(dev)
            up, down = audio.ratio(rate)
            taps = audio.taps_device(rate, dev)
            resident = audio.frontend_device(pcm, rate, 2, "mean", dev)[1][None]

            def reference():
                x = hubert.normalize(hubert.load_audio_16k(path))
                return torch.from_numpy(x)[None].to(dev)

            def kernels():
                return audio.normalize_device(audio.resample_device(raw_dev, 2, channels, "mean", up, down, taps))

            def frontend():
                p, r, wd = audio.read_pcm_wav(path)
                return audio.frontend_device(p, r, wd, "mean", dev)

            steps = {"device_upload": lambda: raw_host.to(dev), "device_kernels": kernels, "device_frontend": frontend,
                     "device_e2e": lambda: ext.extract_features_device(path),
                     "hubert": lambda: hubert.chunked_features(resident, ext._encode, keep_device=True)}
            if have_ffmpeg:
                steps = {"reference": reference, **steps}
            ms = {k: [] for k in steps}
            for r in range(a.warmup + a.rounds):
                for k, fn in steps.items():          # the front ends take turns within a round
                    t = timed(fn)
                    if r >= a.warmup:
                        ms[k].append(t)
            line = {"rate": rate, "channels": channels, "seconds": a.seconds, "pcm_mb": raw_host.numel() / 1e6,
                    "samples_16k": audio.out_samples(n, rate), "layers": a.layers, "precision": a.precision, "rounds": a.rounds,
                    "reference": "ffmpeg" if have_ffmpeg else "not available"}
            for k, v in ms.items():
                line.update(summary(k, v))
            if have_ffmpeg:
                line["device_frontend_vs_reference"] = line["reference_ms"] / line["device_frontend_ms"]
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": f"tools/audio_bench.py --layers {a.layers} --precision {a.precision} --rounds {a.rounds} --warmup {a.warmup} "
                               f"--seconds {a.seconds:g} on one MI355X, profiler off: milliseconds, median and range of the rounds",
                       "source_hash": build.source_hash(), "lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
