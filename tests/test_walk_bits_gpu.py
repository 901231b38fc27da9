"""-m gpu: the S3FD, HuBERT and SyncNet_color handles give the BITS, launch the kernels and ask for the workspace of the commit
recorded in tests/golden/walk_bits.json (S3FD, HuBERT) and tests/golden/walk_bits_sync.json (SyncNet_color).

A file holds, per case, the SHA-256 of the output bytes, the set of kernel names of the launch log and the workspace size the
library reported, written by tools/record_walk_bits.py from a library built from the commit BEFORE a handle's host code was
folded (`parent_commit` in the file): one templated S3FD pass for both precisions, one HuBERT entry over a layout whose offsets
are resolved once, and (the second file, a later commit) one SyncNet_color walk for both precisions over one arena rule, with
one stem body under the two stem kernels.  Those changes move host code and kernel text only, so every case has to reproduce
its recording.  The hashes are that commit's, never the head's: a mismatch means the head is wrong.

Nothing here asserts accuracy (tests/test_facedet*_gpu.py, tests/test_hubert*_gpu.py and tests/test_syncnet*_gpu.py do); a hash
is a fair bar because the handles are bit-reproducible by construction: no stream-K, no K split, no atomics.  The cases are the
smallest that reach every branch of the walks: every S3FD tap at 77 x 93 (odd sizes, pool 3 has a clipped window) and the late
ones at 32 x 32 (the smallest frame the network takes: every late map is 1 x 1) and at 16 x 16 (pool 5 has nothing left: the
forward refuses the frame, and the recording holds the status and its text), every HuBERT stage with 0, 1 and 2 layers behind
the stage-3 tap (0: nothing is pending in the bf16 walk, >= 1: its extra folding pass), and the workspace rules on both sides
of the 2 GiB sub-batch limit.  SyncNet_color: all 31 taps of the hubert mode and the 14 audio taps of the wenet mode at B = 2
(every block, both fp32 outputs and the widening tap of the bf16 precision, both 1x1 paths, the narrow bf16 tile, cin 256 and
stride (1, 2)), the full forward of both modes (both embeddings hashed, audio first), the forward and the last tap at B = 257 (a
pass of 256 frames and a pass of one: every pointer advance of the pass loop), a forward refused for a caller's workspace 256
bytes short, and the workspace sizes on both sides of the 256-frame pass and of the batch limits."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import hubert_ref
from calipsync_amd import _lib, facedet, hubert, recipe, syncnet
from gpu_util import dev, launched

pytestmark = pytest.mark.gpu

_GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = {"walk": os.path.join(_GOLDEN_DIR, "walk_bits.json"), "sync": os.path.join(_GOLDEN_DIR, "walk_bits_sync.json")}   # per family
PRECISIONS = ("fp32", "bf16")
HB_SAMPLES = 720        # the shortest waveform of tests/test_hubert_gpu.py with two tokens
HB_LAYERS = 2
SYNC_PASSES = 257       # SyncNet_color: a pass of 256 frames and a pass of one


def _cases():
    """id -> ("s3fd", precision, h, w, u8, stage) | ("hubert", precision, stage, n_layers) | ("ws_s3fd", precision, batch, h, w) |
    ("ws_hubert", precision, batch, samples) | ("sync_tap", precision, mode, batch, stage) |
    ("sync_fwd", precision, mode, batch, bytes the caller's workspace is short of) | ("ws_sync", precision, mode, batch) |
    ("ws_sync_fp32", "fp32", mode, batch): casync_sync_workspace_bytes"""
    c = {}
    for p in PRECISIONS:
        for stage in facedet.STAGES:
            c[f"s3fd_{p}_77x93_u8_{stage}"] = ("s3fd", p, 77, 93, True, stage)
        c[f"s3fd_{p}_77x93_f32_det"] = ("s3fd", p, 77, 93, False, "det")
        for stage in ("conv5_3", "fc6", "conv7_2", "conf", "det"):
            c[f"s3fd_{p}_32x32_u8_{stage}"] = ("s3fd", p, 32, 32, True, stage)
            c[f"s3fd_{p}_16x16_u8_{stage}"] = ("s3fd", p, 16, 16, True, stage)
    for p in PRECISIONS:
        for stage, n_layers in ((0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (3, 2)):
            c[f"hubert_{p}_stage{stage}_layers{n_layers}"] = ("hubert", p, stage, n_layers)
    for p in PRECISIONS:
        for b, h, w in ((1, 16, 16), (1, 32, 32), (3, 77, 93), (65, 270, 480), (130, 270, 480)):   # the last two: more than one pass, fp32 / both
            c[f"ws_s3fd_{p}_{b}x{h}x{w}"] = ("ws_s3fd", p, b, h, w)
        for b, s in ((2, HB_SAMPLES), (3, 16000)):
            c[f"ws_hubert_{p}_{b}x{s}"] = ("ws_hubert", p, b, s)
    for p in PRECISIONS:
        for stage in syncnet.STAGES:
            c[f"sync_{p}_hubert_b2_{stage}"] = ("sync_tap", p, "hubert", 2, stage)
        for stage in syncnet.STAGES[17:]:   # the face encoder is the same in both modes
            c[f"sync_{p}_wenet_b2_{stage}"] = ("sync_tap", p, "wenet", 2, stage)
        for mode, b, short in (("hubert", 3, 0), ("wenet", 2, 0), ("hubert", SYNC_PASSES, 0), ("hubert", 3, 256)):
            c[f"sync_{p}_{mode}_b{b}_forward" + (f"_ws_short_{short}" if short else "")] = ("sync_fwd", p, mode, b, short)
        c[f"sync_{p}_hubert_b{SYNC_PASSES}_audio.13"] = ("sync_tap", p, "hubert", SYNC_PASSES, "audio.13")
        for mode in ("hubert", "wenet"):
            for b in (0, 1, 3, 256, 257, 65536, 65537):   # 0 and 65537: no handle takes them, the size is 0
                c[f"ws_sync_{p}_{mode}_{b}"] = ("ws_sync", p, mode, b)
    for mode in ("hubert", "wenet"):
        for b in (3, 257):
            c[f"ws_sync_fp32_entry_{mode}_{b}"] = ("ws_sync_fp32", "fp32", mode, b)
    return c


CASES = _cases()


def family(name):
    """the recording file (a key of GOLDEN) that holds the case"""
    return "sync" if "sync" in CASES[name][0] else "walk"


@functools.lru_cache(maxsize=None)
def s3fd_engine(precision):
    return facedet.S3FDEngine(_s3fd_weights(), dev(), precision=precision)


@functools.lru_cache(maxsize=None)
def _s3fd_weights():
    return recipe.make_s3fd_state_dict()


@functools.lru_cache(maxsize=None)
def hubert_engine(precision):
    return hubert.HubertEngine(hubert_ref.recipe_state_dict(HB_LAYERS), HB_LAYERS, precision=precision)


@functools.lru_cache(maxsize=None)
def _frames(h, w):
    return recipe.make_s3fd_inputs(3, h, w)


@functools.lru_cache(maxsize=None)
def _waves():
    return torch.stack([torch.from_numpy(hubert.normalize(hubert_ref.golden_wave(HB_SAMPLES, s))) for s in (21, 22)])


@functools.lru_cache(maxsize=None)
def sync_engine(mode, precision):
    """one engine, and so one workspace, per mode and precision: the B = 257 cases grow it once"""
    return syncnet.SyncNetEngine(syncnet.pack(recipe.make_syncnet_state_dict(mode), mode), mode, dev(), precision=precision)


@functools.lru_cache(maxsize=None)
def _sync_inputs(mode, batch):
    """(face, audio) on the device; more than 3 frames: the 3-frame input repeated (a frame of a batch has the bits of that
    frame alone)"""
    pick = torch.arange(batch) % 3
    return tuple(torch.from_numpy(v)[pick].contiguous().to(dev()) for v in recipe.make_syncnet_inputs(min(batch, 3), mode))


def _run_sync(kind, precision, mode, batch, arg=None):
    lib, m = _lib.load(), _lib.AUDIO_MODES[mode]
    if kind == "ws_sync":
        return None, set(), int(lib.casync_syncnet_workspace_bytes_ex(m, syncnet.PRECISIONS[precision], batch))
    if kind == "ws_sync_fp32":
        return None, set(), int(lib.casync_sync_workspace_bytes(m, batch))
    eng, (face, audio) = sync_engine(mode, precision), _sync_inputs(mode, batch)
    need = int(eng.workspace_bytes(batch))
    with launched() as names:
        try:
            if kind == "sync_tap":
                out = eng.tap(arg, face if arg.startswith("face") else audio).cpu()
            else:
                short = torch.empty((need - arg) // 4, dtype=torch.float32, device=dev()) if arg else None
                out = torch.cat([e.cpu() for e in eng.forward(face, audio, workspace=short)])   # audio first
        except RuntimeError as exc:
            out = str(exc)
    return out, names, need


def run_case(name):
    """-> (the output on the CPU, the text of the error where the forward refused the case or None where the case launches
    nothing; the set of kernels that ran; the workspace bytes the library reported for the case's shape)"""
    kind, precision, *rest = CASES[name]
    lib = _lib.load()
    if "sync" in kind:
        return _run_sync(kind, precision, *rest)
    if kind == "ws_s3fd":
        return None, set(), int(lib.casync_s3fd_workspace_bytes_ex(facedet.PRECISIONS[precision], *rest))
    if kind == "ws_hubert":
        return None, set(), int(lib.casync_hubert_workspace_bytes_h(hubert_engine(precision)._h, *rest))
    if kind == "s3fd":
        h, w, u8, stage = rest
        eng, frames = s3fd_engine(precision), _frames(h, w)
        x = torch.from_numpy(frames) if u8 else torch.from_numpy((frames.astype(np.float32) - facedet.IMG_MEAN).transpose(0, 3, 1, 2).copy())
        with launched() as names:
            try:
                out = eng.forward_tap(x, stage, u8=u8).cpu()
            except RuntimeError as exc:
                out = str(exc)
        return out, names, int(eng.workspace_bytes(len(frames), h, w))
    stage, n_layers = rest
    eng, wave = hubert_engine(precision), _waves()
    with launched() as names:
        out = eng(wave.to(dev()), stage=stage, n_layers=n_layers).cpu()
    return out, names, int(lib.casync_hubert_workspace_bytes_h(eng._h, wave.shape[0], wave.shape[1]))


def record(name):
    """what the golden file holds for one case; AssertionError for an output that is not finite"""
    out, names, workspace = run_case(name)
    if out is None:
        return {"workspace": workspace}
    if isinstance(out, str):
        assert not names, f"{name}: refused after launching {sorted(names)}"
        return {"error": out, "workspace": workspace}
    assert bool(torch.isfinite(out).all()), f"{name}: output not finite"
    assert names, f"{name}: nothing launched"
    return {"sha256": hashlib.sha256(out.contiguous().numpy().tobytes()).hexdigest(), "kernels": sorted(names), "workspace": workspace}


@pytest.fixture(scope="module")
def golden():
    """family -> its recording"""
    out = {}
    for fam, path in GOLDEN.items():
        with open(path) as f:
            out[fam] = json.load(f)
    return out


def test_the_recording_holds_these_cases(golden):
    for fam, rec in golden.items():
        assert sorted(rec["cases"]) == sorted(n for n in CASES if family(n) == fam), fam


@pytest.mark.parametrize("name", list(CASES))
def test_walk_bits(golden, name):
    golden = golden[family(name)]
    got, want = record(name), golden["cases"][name]
    print(f"walk bits {name}: workspace {got['workspace']}, kernels {got.get('kernels')}")
    assert got["workspace"] == want["workspace"], f"{name}: workspace differs from commit {golden['parent_commit'][:12]}"
    assert got.get("kernels") == want.get("kernels"), f"{name}: launched kernels differ from commit {golden['parent_commit'][:12]}"
    assert got.get("error") == want.get("error"), f"{name}: the refusal differs from commit {golden['parent_commit'][:12]}"
    assert got.get("sha256") == want.get("sha256"), f"{name}: output bits differ from commit {golden['parent_commit'][:12]}"
