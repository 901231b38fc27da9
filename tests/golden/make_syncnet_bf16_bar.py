"""Measure the bars of the bf16 SyncNet_color handle by running the REFERENCE itself under bf16 autocast (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_syncnet_bf16_bar.py    # tests/golden/syncnet_bf16_bar.npz

Reaches the reference as make_syncnet_golden.py does (the cv2 stand-in, the same assertion afterwards) and runs the two cases of
that script -- hubert B = 3 and wenet B = 2, ``recipe.make_syncnet_state_dict(mode)`` and ``recipe.make_syncnet_inputs`` -- twice:
``SyncNet_color(mode).eval()`` under ``torch.autocast("cpu", dtype=torch.bfloat16)`` and its ``.double()`` copy.  Recorded per
mode, keys ``<mode>.<name>``:

  * ``<stage>``                [max, mean] of |autocast - float64| over the 4096 sample positions of the fp32 fixture, for the 31
                               block outputs;
  * ``audio_emb``, ``face_emb``  the same two figures over the whole embedding;
  * ``cos_bound``              max over the pairs of |da|_2 / |a|_2 + |df|_2 / |f|_2 (d = autocast - float64): the cosine of two
                               vectors moves by at most that, so it bounds autocast's cosine error;
  * ``cos_err``                autocast's measured max |cos - cos64|, for the record;
  * ``fp32_vs_fixture``        max |float64 embedding - the one in syncnet_<mode>_b<B>.npz|: ties this file to those fixtures.

Only data is written; nothing under ``tests/`` imports this script.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True


class _NoCv2(types.ModuleType):
    asked = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        _NoCv2.asked.append(name)
        raise AttributeError(f"cv2.{name}: the stand-in has no attributes")


sys.modules.setdefault("cv2", _NoCv2("cv2"))
sys.path.insert(0, "/root/reference")
from module.syncnet import SyncNet_color                      # noqa: E402  (the reference)
sys.path.pop(0)

from calipsync_amd import recipe, syncnet                     # noqa: E402

N_SAMPLES = 4096
CASES = (("hubert", 3), ("wenet", 2))


def sample_indices(numel: int) -> np.ndarray:
    return (np.arange(N_SAMPLES, dtype=np.int64) * 2654435761) % numel


def run(net, face, audio, autocast):
    taps = {}
    hooks = []
    for enc, short in ((net.face_encoder, "face"), (net.audio_encoder, "audio")):
        for i, m in enumerate(enc):
            hooks.append(m.register_forward_hook(lambda _m, _i, out, n=f"{short}.{i}": taps.__setitem__(n, out.detach().double())))
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        a_emb, f_emb = net(face, audio)
    for h in hooks:
        h.remove()
    return a_emb.double(), f_emb.double(), taps


def make(mode: str, batch: int, store: dict) -> None:
    sd = {k: torch.from_numpy(v.copy()) for k, v in recipe.make_syncnet_state_dict(mode).items()}
    net = SyncNet_color(mode).eval()
    net.load_state_dict(sd, strict=True)
    net64 = SyncNet_color(mode).double().eval()
    net64.load_state_dict({k: v.double() if v.dtype != torch.int64 else v for k, v in sd.items()}, strict=True)
    x, a = (torch.from_numpy(v) for v in recipe.make_syncnet_inputs(batch, mode))
    a16, f16, taps16 = run(net, x, a, True)
    a64, f64, taps64 = run(net64, x.double(), a.double(), False)
    assert list(taps64) == list(taps16) == list(syncnet.STAGES)
    fx = np.load(os.path.join(HERE, f"syncnet_{mode}_b{batch}.npz"))
    for n in syncnet.STAGES:
        d = (taps16[n] - taps64[n]).abs().reshape(-1).numpy()
        s = sample_indices(d.size)
        assert np.array_equal(taps64[n].reshape(-1).numpy()[s], fx[f"{n}.samples"]), n     # the same float64 run, the same positions
        store[f"{mode}.{n}"] = np.array([d[s].max(), d[s].mean()])
        print(f"{mode} {n:9s} autocast - fp64 at the samples: max {d[s].max():.3e} mean {d[s].mean():.3e}   (whole tensor {d.max():.3e} {d.mean():.3e})")
    for name, e16, e64 in (("audio_emb", a16, a64), ("face_emb", f16, f64)):
        d = (e16 - e64).abs()
        store[f"{mode}.{name}"] = np.array([float(d.max()), float(d.mean())])
    bound = ((a16 - a64).norm(dim=1) / a64.norm(dim=1) + (f16 - f64).norm(dim=1) / f64.norm(dim=1)).max()
    cos16 = torch.nn.functional.cosine_similarity(a16, f16)
    cos64 = torch.nn.functional.cosine_similarity(a64, f64)
    store[f"{mode}.cos_bound"] = np.array(float(bound))
    store[f"{mode}.cos_err"] = np.array(float((cos16 - cos64).abs().max()))
    store[f"{mode}.fp32_vs_fixture"] = np.array(max(float(np.abs(a64.numpy() - fx["audio_emb64"]).max()),
                                                    float(np.abs(f64.numpy() - fx["face_emb64"]).max())))
    assert float(store[f"{mode}.fp32_vs_fixture"]) <= 1e-12
    print(mode, "embeddings", store[f"{mode}.audio_emb"], store[f"{mode}.face_emb"], "cos bound", float(bound), "cos err",
          float(store[f"{mode}.cos_err"]))


def main() -> None:
    torch.manual_seed(0)
    torch.set_num_threads(8)
    store: dict = {}
    for mode, batch in CASES:
        make(mode, batch, store)
    assert not _NoCv2.asked, f"the reference asked the cv2 stand-in for {_NoCv2.asked}"
    path = os.path.join(HERE, "syncnet_bf16_bar.npz")
    np.savez_compressed(path, **store)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
