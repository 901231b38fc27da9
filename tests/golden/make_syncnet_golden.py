"""Generate the SyncNet_color golden fixtures by running the REFERENCE itself (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_syncnet_golden.py    # syncnet_hubert_b3.npz, syncnet_wenet_b2.npz, manifests

module/syncnet.py imports cv2 at its head and the build image has none: an attribute-less stand-in is placed in sys.modules
for the import (as make_frame_golden.py does) and the script asserts afterwards that no attribute of it was ever asked for --
neither the constructor nor forward touches cv2.  Loads ``recipe.make_syncnet_state_dict(mode)`` (217 keys) into the
reference ``SyncNet_color(mode).eval()`` with strict=True, runs ``recipe.make_syncnet_inputs(B, mode)`` in fp32 and again in
a ``.double()`` copy, and records in make_pfld_golden.py's format: both embeddings in full (fp32 and fp64), ``ref_err.<stage>``
= max|fp32 - fp64| of the 31 block outputs and of the two embeddings, the fp64 block outputs as (statistics, 4096 strided
samples), the reference's cosine_similarity of the B pairs in both precisions.  Only data is written; nothing under
``tests/`` imports this script.
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


def summarize(name: str, t: torch.Tensor, store: dict) -> None:
    a = t.detach().contiguous().numpy()
    flat = a.reshape(-1)
    f64 = flat.astype(np.float64)
    store[f"{name}.shape"] = np.array(a.shape, dtype=np.int64)
    store[f"{name}.stats"] = np.array([f64.sum(), np.abs(f64).sum(), (f64 * f64).sum(), f64.min(), f64.max()], dtype=np.float64)
    store[f"{name}.samples"] = flat[sample_indices(flat.size)]


def run(net, face, audio):
    taps = {}
    hooks = []
    for enc, short in ((net.face_encoder, "face"), (net.audio_encoder, "audio")):
        for i, m in enumerate(enc):
            hooks.append(m.register_forward_hook(lambda _m, _i, out, n=f"{short}.{i}": taps.__setitem__(n, out.detach().clone())))
    with torch.no_grad():
        a_emb, f_emb = net(face, audio)
    for h in hooks:
        h.remove()
    return a_emb, f_emb, taps


def make(mode: str, batch: int) -> None:
    sd_np = recipe.make_syncnet_state_dict(mode)
    sd = {k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}
    net = SyncNet_color(mode).eval()
    print(mode, "load_state_dict:", net.load_state_dict(sd, strict=True))
    net64 = SyncNet_color(mode).double().eval()
    net64.load_state_dict({k: v.double() if v.dtype != torch.int64 else v for k, v in sd.items()}, strict=True)
    x, a = (torch.from_numpy(v) for v in recipe.make_syncnet_inputs(batch, mode))
    a32, f32, taps32 = run(net, x, a)
    a64, f64, taps64 = run(net64, x.double(), a.double())
    assert list(taps64) == list(syncnet.STAGES)

    store: dict = {"batch": np.array([batch]), "audio_emb64": a64.numpy(), "face_emb64": f64.numpy(), "audio_emb32": a32.numpy(),
                   "face_emb32": f32.numpy()}
    for n in syncnet.STAGES:
        m = float(taps64[n].abs().max())
        assert 0.1 <= m <= 16.0, f"stage {n}: max |x| = {m} outside [0.1, 16]: the recipe does not keep the network in range"
        store[f"ref_err.{n}"] = np.array(float((taps32[n].double() - taps64[n]).abs().max()))
        summarize(n, taps64[n], store)
        print(f"{n:9s} {tuple(taps64[n].shape)} max {m:.3f} ref_err {float(store[f'ref_err.{n}']):.2e}")
    store["ref_err.audio_emb"] = np.array(float((a32.double() - a64).abs().max()))
    store["ref_err.face_emb"] = np.array(float((f32.double() - f64).abs().max()))
    cos32 = torch.nn.functional.cosine_similarity(a32, f32)
    cos64 = torch.nn.functional.cosine_similarity(a64, f64)
    store.update(cos32=cos32.numpy(), cos64=cos64.numpy(), **{"ref_err.cos": np.array(float((cos32.double() - cos64).abs().max()))})
    print("embeddings ref_err", float(store["ref_err.audio_emb"]), float(store["ref_err.face_emb"]), "cos", cos64.numpy(),
          "ref_err", float(store["ref_err.cos"]))
    path = os.path.join(HERE, f"syncnet_{mode}_b{batch}.npz")
    np.savez_compressed(path, **store)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    with open(os.path.join(HERE, f"state_dict_manifest_syncnet_{mode}.txt"), "w") as f:
        for k, v in net.state_dict().items():
            f.write(f"{k} {tuple(v.shape)} {str(v.dtype).replace('torch.', '')}\n")
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def main() -> None:
    torch.manual_seed(0)
    torch.set_num_threads(8)
    for mode, batch in CASES:
        make(mode, batch)
    assert not _NoCv2.asked, f"the reference asked the cv2 stand-in for {_NoCv2.asked}"


if __name__ == "__main__":
    main()
