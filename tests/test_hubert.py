"""HuBERT feature extractor, CPU side: the torch restatement against the reference's own extract_features
(tests/golden/hubert_*.npz, made by tests/golden/make_hubert_golden.py), the repo's chunking bit for bit, the
checkpoint loader and packer, and the WAV reader."""
import hashlib
import json
import os
import wave

import numpy as np
import pytest
import torch

import hubert_ref
from calipsync_amd import hubert

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def restated_features(wave_np, layers, P=None):
    """extract_features with the CPU restatement as the model."""
    P = P if P is not None else hubert.packed_tensors(hubert_ref.recipe_state_dict(layers), layers)
    x = torch.from_numpy(hubert.normalize(wave_np))[None]
    return hubert.chunked_features(x, lambda chunks: [hubert_ref.forward(P, layers, c)[0] for c in chunks])


def test_restatement_matches_reference_2_layers():
    g = golden("hubert_l2.npz")
    wave_np = hubert_ref.golden_wave(int(g["samples"]), int(g["seed"]))
    assert sha(wave_np) == str(g["wave_sha256"])
    P = hubert.packed_tensors(hubert_ref.recipe_state_dict(2), 2)
    got = restated_features(wave_np, 2, P).numpy()
    assert got.shape == g["out"].shape
    assert np.abs(got - g["out"]).max() <= 1e-5
    taps = {}
    hubert_ref.forward(P, 2, torch.from_numpy(hubert.normalize(wave_np))[None], taps)
    assert np.abs(taps["conv"][0].numpy().reshape(-1)[g["conv_idx"]] - g["conv_val"]).max() <= 1e-5
    assert np.abs(taps["layer0_in"][0].numpy().reshape(-1)[g["l0_idx"]] - g["l0_val"]).max() <= 1e-5
    # the recipe is not degenerate: attention is far from uniform and from one-hot
    assert 0.05 < g["att_maxp"].mean() < 0.9


def test_restatement_matches_reference_24_layers_across_a_chunk_seam():
    g = golden("hubert_l24.npz")
    wave_np = hubert_ref.golden_wave(int(g["samples"]), int(g["seed"]))
    assert sha(wave_np) == str(g["wave_sha256"])
    got = restated_features(wave_np, 24).numpy()
    assert tuple(got.shape) == tuple(g["out_shape"])
    flat = got.reshape(-1, 1024)
    assert np.abs(flat[g["rows"]] - g["row_val"]).max() <= 1e-4
    assert np.abs(flat.reshape(-1)[g["idx"]] - g["val"]).max() <= 1e-4
    assert np.abs(np.linalg.norm(flat.astype(np.float64), axis=1) - g["norms"]).max() <= 1e-3
    assert (g["att_maxp"] > 10.0 / 1000).all() and (g["att_maxp"] < 0.9).all()   # between uniform (1e-3) and one-hot


def test_chunking_equals_the_reference_bit_for_bit():
    g = golden("hubert_chunks.npz")
    seed = int(g["seed"])

    def stub(chunks):
        return [hubert_ref.stub_encode(c) for c in chunks]

    for n in g["lengths"]:
        w = hubert_ref.golden_wave(int(n), seed)
        assert sha(w) == str(g[f"n{n}_wave_sha256"])
        x = torch.from_numpy(hubert.normalize(w))[None]
        if f"n{n}_raises" in g:
            with pytest.raises(ValueError):
                hubert.chunked_features(x, stub)
            continue
        f = hubert.chunked_features(x, stub).numpy()
        assert tuple(f.shape) == tuple(g[f"n{n}_shape"]), n
        assert sha(f) == str(g[f"n{n}_sha256"]), n
    stereo = np.stack([hubert_ref.golden_wave(720, seed), hubert_ref.golden_wave(720, seed + 1)], 1)
    assert sha(stereo) == str(g["stereo_wave_sha256"])
    x = torch.from_numpy(hubert.normalize(stereo[:, 0]))[None]
    f = hubert.chunked_features(x, stub).numpy()
    assert tuple(f.shape) == tuple(g["stereo_shape"]) and sha(f) == str(g["stereo_sha256"])


def test_chunking_batches_full_chunks_and_runs_the_rest_apart():
    calls = []

    def enc(chunks):
        calls.append([c.shape[1] for c in chunks])
        return [hubert_ref.stub_encode(c) for c in chunks]

    hubert.chunked_features(torch.zeros(1, 2 * hubert.CLIP + 5000), enc)
    assert calls == [[hubert.CHUNK, hubert.CHUNK], [5000]]
    calls.clear()
    hubert.chunked_features(torch.zeros(1, 2 * hubert.CLIP + 40), enc)     # the last chunk is cut short by the end
    assert calls == [[hubert.CHUNK], [hubert.CLIP + 40]]


def write_checkpoint(path, layers, spelling="weight_g", cfg_over=None):
    os.makedirs(path, exist_ok=True)
    cfg = dict(hubert_ref.config(layers), **(cfg_over or {}))
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f)
    with open(os.path.join(path, "preprocessor_config.json"), "w") as f:
        json.dump({"do_normalize": True, "sampling_rate": 16000, "feature_size": 1}, f)
    sd = {"hubert." + k: v for k, v in hubert_ref.recipe_state_dict(layers, spelling).items()}
    sd["hubert.masked_spec_embed"] = torch.zeros(1024)
    sd["lm_head.weight"] = torch.zeros(32, 1024)
    sd["lm_head.bias"] = torch.zeros(32)
    torch.save(sd, os.path.join(path, "pytorch_model.bin"))
    return path


@pytest.mark.parametrize("spelling", ["weight_g", "parametrizations"])
def test_loader_packs_a_checkpoint_directory_that_reproduces_the_reference(tmp_path, spelling):
    cfg, sd, do_norm = hubert.load_checkpoint(write_checkpoint(str(tmp_path / "ckpt"), 2, spelling))
    assert do_norm and cfg["num_hidden_layers"] == 2
    assert not any(k.startswith(("hubert.", "lm_head")) or k == "masked_spec_embed" for k in sd)
    buf = hubert.pack(sd, 2)
    from calipsync_amd import _lib
    assert buf.size == _lib.load().casync_hubert_packed_total(2)
    P = hubert.unpack(buf, 2)
    g = golden("hubert_l2.npz")
    got = restated_features(hubert_ref.golden_wave(int(g["samples"]), int(g["seed"])), 2, P).numpy()
    assert np.abs(got - g["out"]).max() <= 1e-5


@pytest.mark.parametrize("field,value", [("hidden_act", "gelu_new"), ("do_stable_layer_norm", False), ("hidden_size", 768),
                                         ("feat_extract_norm", "group"), ("num_attention_heads", 12), ("layer_norm_eps", 1e-6)])
def test_loader_refuses_a_config_it_does_not_compute(tmp_path, field, value):
    path = str(tmp_path / "ckpt")
    os.makedirs(path)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(hubert_ref.config(2), **{field: value}), f)
    with pytest.raises(ValueError, match=field):
        hubert.load_checkpoint(path)


def test_wav_reader_round_trips_pcm16(tmp_path):
    x = (hubert_ref.golden_wave(5000, 3) * 32767).astype("<i2")
    p = str(tmp_path / "a.wav")
    with wave.open(p, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(x.tobytes())
    got = hubert.read_wav(p)
    assert got.dtype == np.float64 and np.array_equal(got, x.astype(np.float64) / 32768.0)
    with wave.open(p, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(8000)
        w.writeframes(x.tobytes())
    with pytest.raises(ValueError, match="ffmpeg"):
        hubert.read_wav(p)


def test_token_count_matches_the_engine():
    from calipsync_amd import _lib
    lib = _lib.load()
    for n in (399, 400, 401, 719, 720, 2000, 48000, hubert.CHUNK, 328000):
        assert hubert.tokens(n) == lib.casync_hubert_tokens(n)
    assert hubert.tokens(hubert.CHUNK) == 1000 and hubert.tokens(399) == 0
