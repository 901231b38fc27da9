"""Generate the mode='wenet' golden fixture by running the REFERENCE itself (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_wenet_golden.py     # G1.2 wenet, B=2 -> unet_wenet_b2.npz

Loads the repo's deterministic G1.2 recipe in its wenet form (``recipe.make_state_dict(mode="wenet")``,
577 keys) into the reference ``Model(6, 'wenet')`` in eval mode, runs ``recipe.make_inputs(2,
mode="wenet")`` (audio [2,256,16,32]) through it on PyTorch-CPU fp32, and records the output and named
intermediates as (statistics, 4096 strided samples) -- ``make_golden.py``'s format -- plus frame 0 of the output
in full (``out.frame0``; the whole output would double the file).  Also writes ``state_dict_manifest_wenet.txt``.
Only data is written (compressed); nothing under ``tests/`` imports this script.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True

from calipsync_amd import arch, recipe          # noqa: E402
from module.unet import Model                   # noqa: E402  (the reference)

sys.path.insert(0, HERE)
from make_golden import summarize               # noqa: E402

BATCH = 2


def main() -> None:
    torch.manual_seed(0)
    torch.set_num_threads(8)
    sd_np = recipe.make_state_dict(mode="wenet")
    net = Model(6, "wenet").eval()
    print("load_state_dict:", net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}, strict=True))
    x_np, a_np = recipe.make_inputs(BATCH, mode="wenet")
    x, a = torch.from_numpy(x_np), torch.from_numpy(a_np)

    taps: dict = {}
    pre: list = []

    def hook(name):
        def fn(_m, _inp, out):
            taps[name] = out.detach().clone()
        return fn

    am = net.audio_model
    named = {"audio_conv1": am.conv1, "audio_conv2": am.conv2, "audio_conv4": am.conv4, "a": am,
             "x5": net.down4, "tx": net.bn_tx, "kx": net.lru_kx, "fuse": net.fuse_conv, "u4": net.up4}
    handles = [m.register_forward_hook(hook(n)) for n, m in named.items()]
    # am.relu serves conv3 and conv5: its outputs in call order; bn3 / bn5 give the pre-activations
    handles.append(am.relu.register_forward_hook(lambda _m, _i, out: pre.append(out.detach().clone())))
    handles.append(am.bn3.register_forward_hook(hook("bn3")))
    handles.append(am.bn5.register_forward_hook(hook("bn5")))
    with torch.no_grad():
        out = net(x, a)
        for h in handles:
            h.remove()
        net64 = Model(6, "wenet").double().eval()
        net64.load_state_dict({k: torch.from_numpy(v.copy()).double() if v.dtype != np.int64
                               else torch.from_numpy(v.copy()) for k, v in sd_np.items()})
        out64 = net64(x.double(), a.double())
        out_sw = net(x, a.flip(0))
    taps["out"] = out
    taps["audio_conv3"], taps["audio_conv5"] = pre[0], pre[1]
    neg3, neg5 = float((taps.pop("bn3") < 0).double().mean()), float((taps.pop("bn5") < 0).double().mean())
    print("out range", float(out.min()), float(out.max()), "std", float(out.std()))
    print("fp32 vs fp64 max|d|", float((out.double() - out64).abs().max()))
    print("audio-swap max|d|", float((out - out_sw).abs().max()))
    print(f"negative pre-activations: conv3 {neg3:.3f}, conv5 {neg5:.3f}")

    store: dict = {}
    for name, t in taps.items():
        summarize(name, t, store, False)
    store["out.frame0"] = out[0].numpy()
    store["fp32_vs_fp64_maxdiff"] = np.array([float((out.double() - out64).abs().max())])
    store["audio_swap_maxdiff"] = np.array([float((out - out_sw).abs().max())])
    store["negative_preact"] = np.array([neg3, neg5])
    h = hashlib.sha256()
    for k, _s, _d, _r in arch.manifest("wenet"):
        h.update(np.ascontiguousarray(sd_np[k]).tobytes())
    store["weights_sha256"] = np.frombuffer(h.digest(), dtype=np.uint8)
    store["inputs_sha256"] = np.frombuffer(hashlib.sha256(x_np.tobytes() + a_np.tobytes()).digest(), dtype=np.uint8)
    store["batch"] = np.array([BATCH])
    store["n_parameters"] = np.array([sum(p.numel() for p in net.parameters())])
    path = os.path.join(HERE, "unet_wenet_b2.npz")
    np.savez_compressed(path, **store)
    with open(os.path.join(HERE, "state_dict_manifest_wenet.txt"), "w") as f:
        for k, v in net.state_dict().items():
            f.write(f"{k} {tuple(v.shape)} {str(v.dtype).replace('torch.', '')}\n")
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
