"""Generate the end-to-end bars of the bf16 U-Net engine from the REFERENCE itself (build container only): how far the
reference's own ``Model`` moves under ``torch.autocast("cpu", dtype=torch.bfloat16)`` against its own float64 run.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_unet_bf16_bar.py      # -> tests/golden/unet_bf16_bar.npz

The reference is reached exactly as ``make_golden.py`` / ``make_wenet_golden.py`` reach it (``/root/reference/module/unet.py``,
forward hooks on the same modules).  Two cases, the recipe weights and the B = 2 inputs of the fp32 fixtures:

    hubert   ``Model(6, 'hubert')``, ``recipe.make_inputs(2)``                 (fixture ``unet_g12_b2.npz``)
    wenet    ``Model(6, 'wenet')``,  ``recipe.make_inputs(2, mode="wenet")``   (fixture ``unet_wenet_b2.npz``)

each run three ways -- float32, float64, autocast -- and per case the file holds

    <case>.<tap>             [max, mean] of |autocast - float64| over the whole tensor, for every tap name and for ``out``
    <case>.fp32_vs_fixture   max |float32 run here - value stored in the fp32 fixture| / max(1, max|stored|) over the fixture's taps
    <case>.f64_vs_oracle     max |float64 run here - the repository's CPU restatement in float64| / max(1, max|.|) over the taps:
                             the GPU tests measure the engine against that restatement (the reference is not on the GPU machine)

Only these figures are written; tests/test_unet_bf16_model.py and tests/test_model_bf16_contract_gpu.py read them.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True

from calipsync_amd import recipe               # noqa: E402
from module.unet import Model                   # noqa: E402  (the reference)
from oracle import unet_oracle                  # noqa: E402
import wenet_ref                                # noqa: E402

TAPS = {"hubert": ["x1", "x2", "x3", "x4", "x5", "audio_conv1", "audio_conv2", "audio_conv3", "audio_conv4", "audio_conv5", "a",
                   "tx", "att0", "att1", "att2", "att3", "kx", "fuse", "u1", "u2", "u3", "u4", "out"],
        "wenet": ["x1", "x2", "x3", "x4", "x5", "audio_conv1", "audio_conv2", "audio_conv3", "audio_conv4", "audio_conv5", "a",
                  "tx", "att0", "att1", "att2", "att3", "kx", "fuse", "u1", "u2", "u3", "u4", "out"]}
FIXTURE = {"hubert": "unet_g12_b2.npz", "wenet": "unet_wenet_b2.npz"}


def sample_indices(numel: int, n: int = 4096) -> np.ndarray:
    return (np.arange(n, dtype=np.int64) * 2654435761) % numel


def run(net, x, a) -> dict:
    """one forward with make_golden.py's hooks: every tap as a float64 NumPy array"""
    taps, relu = {}, []
    am = net.audio_model
    named = {"x1": net.inc, "x2": net.down1, "x3": net.down2, "x4": net.down3, "x5": net.down4, "audio_conv1": am.conv1,
             "audio_conv2": am.conv2, "audio_conv4": am.conv4, "a": am, "tx": net.bn_tx, "kx": net.lru_kx, "fuse": net.fuse_conv,
             "u1": net.up1, "u2": net.up2, "u3": net.up3, "u4": net.up4}
    for i, blk in enumerate(net.attention_blocks):
        named[f"att{i}"] = blk

    def hook(name):
        def fn(_m, _inp, out):
            taps[name] = out.detach().clone()
        return fn

    handles = [m.register_forward_hook(hook(n)) for n, m in named.items()]
    handles.append(am.relu.register_forward_hook(lambda _m, _i, out: relu.append(out.detach().clone())))
    with torch.no_grad():
        taps["out"] = net(x, a)
    for h in handles:
        h.remove()
    taps["audio_conv3"], taps["audio_conv5"] = relu[0], relu[1]
    return {k: v.double().numpy() for k, v in taps.items()}


def rel(a, b) -> float:
    return float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))


def main() -> None:
    torch.manual_seed(0)
    torch.set_num_threads(16)   # fixed: the bf16 GEMMs of the autocast run sum in an order that depends on the thread count
    store: dict = {}
    for case in ("hubert", "wenet"):
        sd_np = recipe.make_state_dict(mode=case)
        x_np, a_np = recipe.make_inputs(2, mode=case)
        x, a = torch.from_numpy(x_np), torch.from_numpy(a_np)
        net = Model(6, case).eval()
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}, strict=True)
        net64 = Model(6, case).double().eval()
        net64.load_state_dict({k: torch.from_numpy(v.copy()).double() if v.dtype != np.int64 else torch.from_numpy(v.copy())
                               for k, v in sd_np.items()}, strict=True)
        t32, t64 = run(net, x, a), run(net64, x.double(), a.double())
        with torch.autocast("cpu", dtype=torch.bfloat16):
            tac = run(net, x, a)
        for name in TAPS[case]:
            d = np.abs(tac[name] - t64[name])
            store[f"{case}.{name}"] = np.array([d.max(), d.mean()])
        # the tie to the fp32 fixture: whatever that fixture stores of these taps
        fx, tie = np.load(os.path.join(HERE, FIXTURE[case])), 0.0
        for name in TAPS[case]:
            flat = t32[name].reshape(-1)
            if f"{name}.full" in fx.files:
                tie = max(tie, rel(flat, fx[f"{name}.full"].reshape(-1).astype(np.float64)))
            elif f"{name}.samples" in fx.files:
                tie = max(tie, rel(flat[sample_indices(flat.size)], fx[f"{name}.samples"].astype(np.float64)))
        store[f"{case}.fp32_vs_fixture"] = np.array(tie)
        # ... and to the float64 the GPU tests can compute: the restatement of oracle/ (tests/wenet_ref.py for wenet)
        o64 = {}
        sd64 = unet_oracle.to_torch(sd_np, torch.float64)
        o64["out"] = (wenet_ref if case == "wenet" else unet_oracle).forward(sd64, x.double(), a.double(), o64)
        store[f"{case}.f64_vs_oracle"] = np.array(max(rel(o64[n].numpy(), t64[n]) for n in TAPS[case] if n in o64))
        for k in sorted(store):
            if k.startswith(case):
                print(k, store[k], flush=True)
        assert tie <= 1e-5 and float(store[f"{case}.f64_vs_oracle"]) <= 1e-12
    path = os.path.join(HERE, "unet_bf16_bar.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
