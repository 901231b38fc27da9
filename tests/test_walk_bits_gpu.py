"""-m gpu: the S3FD, HuBERT, SyncNet_color and U-Net handles give the BITS, launch the kernels and ask for the workspace of the commit
recorded in tests/golden/walk_bits.json (S3FD, HuBERT), tests/golden/walk_bits_sync.json (SyncNet_color) and
tests/golden/walk_bits_unet.json (the U-Net plan of csrc/engine.hip).

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
bytes short, and the workspace sizes on both sides of the 256-frame pass and of the batch limits.

The U-Net family (`unet`) was recorded in front of the commit that resolved the plan's weight offsets once and put the choice of a
block's expand path into one function: host code only, so the head reproduces the recording.  A forward case holds the SHA-256
of `out` of a plain Model.forward, of every tap behind it (all 22 up to 12 frames, the ones at 20 x 20 or below above that, one
entry per tap so that a mismatch names the first tensor that differs), the launch-log set of that forward, the ordered rows of
Model.profile on the same input (name, kernel, flops, bytes; forward_windows has no profiling entry: no rows) and the workspace
size.  Bits, kernels, row names and sizes are compared for equality, flops and bytes to 1e-12 relative: the bookings are products
and sums of integers below 2^53 plus one ratio in conv3x3, which a reordered double expression moves by a few units of 2^-53.
The cases are the smallest that reach every arm of encode, trunk, decode, Plan::ir and run_forward (_unet_cases), each in two
variants: `sk0` (gemm_streamk=0: no K split, bits that have to repeat) and `default`.  Here the U-Net differs from the other
handles: stream-K recombines in a fixed order, but a `default` case whose hashes did not repeat over the recorder's three runs
holds null hashes and the reason, and only its hashes go unchecked.  The workspace-only cases ask casync_workspace_bytes_h at
B = 1, 11, 12 and 33 under every option set of the forward cases, in both precisions and both modes."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import hubert_ref
from calipsync_amd import _lib, facedet, hubert, recipe, syncnet
from gpu_util import dev, launched, options
from stream_contract import _tile
from workspace_contract import UNET_TAPS

pytestmark = pytest.mark.gpu

_GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = {"walk": os.path.join(_GOLDEN_DIR, "walk_bits.json"), "sync": os.path.join(_GOLDEN_DIR, "walk_bits_sync.json"),
          "unet": os.path.join(_GOLDEN_DIR, "walk_bits_unet.json")}   # per family
PRECISIONS = ("fp32", "bf16")
HB_SAMPLES = 720        # the shortest waveform of tests/test_hubert_gpu.py with two tokens
HB_LAYERS = 2
SYNC_PASSES = 257       # SyncNet_color: a pass of 256 frames and a pass of one


def _cases():
    """id -> ("s3fd", precision, h, w, u8, stage) | ("hubert", precision, stage, n_layers) | ("ws_s3fd", precision, batch, h, w) |
    ("ws_hubert", precision, batch, samples) | ("sync_tap", precision, mode, batch, stage) |
    ("sync_fwd", precision, mode, batch, bytes the caller's workspace is short of) | ("ws_sync", precision, mode, batch) |
    ("ws_sync_fp32", "fp32", mode, batch): casync_sync_workspace_bytes | the U-Net family's, see _unet_cases"""
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
    c.update(_unet_cases())
    return c


UNET_VARIANTS = {"sk0": {"gemm_streamk": 0}, "default": {}}
UNET_ALL_TAPS_TO = 12     # frames up to which a forward case hashes all 22 taps
UNET_SMALL_TAPS = ("x4", "x5", "audio_conv3", "audio_conv4", "audio_conv5", "a", "tx", "kx", "att0", "att1", "att2", "att3", "fuse", "u1")
UNET_WS_BATCHES = (1, 11, 12, 33)
_ONE_OPTION = (("fuse_ir", 0), ("fuse_up", 0), ("ups_commute", 0), ("ups_commute", 1), ("fuse_dw", 0), ("fuse_dw", 1), ("fuse_q", 0),
               ("skip_early", 0), ("kv_early", 0), ("overlap", 0), ("fuse_min_hw", 81))
_BF16_OPTION = (("ups_commute_bf16", 0), ("fuse_dw_bf16", 0), ("fuse_dw_bf16", 1), ("att_bf16", 0))


def _unet_cases():
    """id -> ("unet_fwd", precision, mode, batch, ((option, value), ...), variant, windows) |
    ("ws_unet", precision, mode, ((option, value), ...)): casync_workspace_bytes_h at UNET_WS_BATCHES"""
    fwd = [("fp32", "hubert", b, ()) for b in (1, 3, 8, 12, 33)]     # one frame / the deep tiles / 40x40 strips / whole-frame tiles / two lanes
    fwd += [("fp32", "hubert", b, (kv,)) for kv in _ONE_OPTION for b in (3, 12)]
    fwd += [("fp32", "hubert", 33, (("trunk_lanes", 1),)), ("fp32", "hubert", 33, (("kv_early", 2),))]
    fwd += [("fp32", "wenet", 3, ()), ("fp32", "wenet", 12, ())]      # 12: the rectangular kernels
    fwd += [("bf16", "hubert", b, ()) for b in (3, 12, 33)]           # 12: fuse_dw_bf16_min
    fwd += [("bf16", "hubert", 48, (("bf16_plan", 48),))]             # three lanes, the ring GEMM, overlap 0
    fwd += [("bf16", "hubert", 12, (kv,)) for kv in _BF16_OPTION]
    fwd += [("bf16", "wenet", 3, ()), ("bf16", "wenet", 12, ())]      # 3: the A0L residual
    sets = []
    for _, _, _, opts in fwd:
        if opts not in sets:
            sets.append(opts)
    tag = lambda opts: "".join(f"_{k}{v}" for k, v in opts)
    c = {}
    for variant in UNET_VARIANTS:
        for p, mode, b, opts in fwd:
            c[f"unet_{p}_{mode}_b{b}{tag(opts)}_{variant}"] = ("unet_fwd", p, mode, b, opts, variant, False)
        for p in PRECISIONS:
            c[f"unet_{p}_windows_b3_{variant}"] = ("unet_fwd", p, "hubert", 3, (), variant, True)
    for p in PRECISIONS:
        for mode in ("hubert", "wenet"):
            for opts in sets:
                c[f"ws_unet_{p}_{mode}{tag(opts)}"] = ("ws_unet", p, mode, opts)
    return c


CASES = _cases()


def family(name):
    """the recording file (a key of GOLDEN) that holds the case"""
    kind = CASES[name][0]
    return "unet" if "unet" in kind else "sync" if "sync" in kind else "walk"


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


@functools.lru_cache(maxsize=None)
def unet_model(precision, mode):
    """one Model per precision and mode, weights on the device"""
    from calipsync_amd.unet import Model, WenetModel
    net = (WenetModel(6, precision=precision) if mode == "wenet" else Model(6, "hubert", precision=precision)).to(dev())
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe.make_state_dict(mode=mode).items()})
    net.eval()
    net._ensure_weights(net._device())
    return net


@functools.lru_cache(maxsize=None)
def _unet_inputs(mode, batch, windows):
    """device inputs: the recipe's frames, tiled above 12; windows: the feature array and indices before, inside and past the clip"""
    import frame_data
    x, a = recipe.make_inputs(min(batch, 12), recipe.INPUT_SEED, mode)
    x = torch.from_numpy(_tile(x, batch)).to(dev())
    if windows:
        return x, torch.from_numpy(frame_data.golden_features(24, seed=3)).to(dev()), (torch.arange(batch, dtype=torch.int32) * 11 - 3).to(dev())
    return x, torch.from_numpy(_tile(a, batch)).to(dev())


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def record_unet(name):
    """what the golden file holds for one case of the U-Net family"""
    kind, precision, mode, *rest = CASES[name]
    net, lib = unet_model(precision, mode), _lib.load()
    if kind == "ws_unet":
        with options(net, **dict(rest[0])):
            return {"workspace": {str(b): int(lib.casync_workspace_bytes_h(net._engine, b)) for b in UNET_WS_BATCHES}}
    batch, opts, variant, windows = rest
    inputs = _unet_inputs(mode, batch, windows)
    with options(net, **{**dict(opts), **UNET_VARIANTS[variant]}):
        with launched() as names:
            out = net.forward_windows(*inputs) if windows else net(*inputs)
        assert bool(torch.isfinite(out).all()), f"{name}: output not finite"
        rec = {"out": _sha(out)}
        rec["taps"] = {t: _sha(net.tap(t, batch)) for t in unet_taps(name)}
        rec["kernels"] = sorted(names)
        rec["rows"] = [] if windows else [[r["name"], r["kernel"], r["flops"], r["bytes"]] for r in net.profile(*inputs)]
        rec["workspace"] = int(lib.casync_workspace_bytes_h(net._engine, batch))
    assert names, f"{name}: nothing launched"
    return rec


def unet_taps(name):
    """the taps a forward case hashes, in the order the file holds them"""
    return UNET_TAPS if CASES[name][3] <= UNET_ALL_TAPS_TO else UNET_SMALL_TAPS


UNET_TABLES = ("strings", "rows", "hashes")


def unet_pack(cases):
    """-> (tables, cases) as the file holds them.  Every text (row name, kernel name), every profiled row and every hash is written
    once, in a table, and a case holds indices: a row recurs in most cases of its batch size and a tap's hash wherever the
    option under test sits behind it, so written out in every case the file would be eight times the size.  The taps of a case
    are a list in the order of unet_taps(); whole-numbered flops and bytes are written as integers."""
    tables, index = {k: [] for k in UNET_TABLES}, {k: {} for k in UNET_TABLES}

    def ref(kind, value):
        key = json.dumps(value)
        if key not in index[kind]:
            index[kind][key] = len(tables[kind])
            tables[kind].append(value)
        return index[kind][key]

    def whole(v):
        return int(v) if v == int(v) else v

    out = {}
    for name, rec in cases.items():
        rec = dict(rec)
        if "rows" in rec:
            assert list(rec["taps"]) == list(unet_taps(name)), name
            rec["kernels"] = [ref("strings", k) for k in rec["kernels"]]
            rec["rows"] = [ref("rows", [ref("strings", n), ref("strings", k), whole(f), whole(b)]) for n, k, f, b in rec["rows"]]
            rec["out"] = None if rec["out"] is None else ref("hashes", rec["out"])
            rec["taps"] = [None if h is None else ref("hashes", h) for h in rec["taps"].values()]
        out[name] = rec
    return tables, out


def unet_unpack(doc):
    """the cases of a loaded file as record_unet() returns them"""
    strings, rows, hashes = (doc[k] for k in UNET_TABLES)
    out = {}
    for name, rec in doc["cases"].items():
        rec = dict(rec)
        if "rows" in rec:
            rec["kernels"] = [strings[k] for k in rec["kernels"]]
            rec["rows"] = [[strings[rows[r][0]], strings[rows[r][1]], rows[r][2], rows[r][3]] for r in rec["rows"]]
            rec["out"] = None if rec["out"] is None else hashes[rec["out"]]
            rec["taps"] = {t: None if h is None else hashes[h] for t, h in zip(unet_taps(name), rec["taps"])}
        out[name] = rec
    return out


def record(name):
    """what the golden file holds for one case; AssertionError for an output that is not finite"""
    if family(name) == "unet":
        return record_unet(name)
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
    out["unet"]["cases"] = unet_unpack(out["unet"])
    return out


def test_the_recording_holds_these_cases(golden):
    for fam, rec in golden.items():
        assert sorted(rec["cases"]) == sorted(n for n in CASES if family(n) == fam), fam


@pytest.mark.parametrize("name", [n for n in CASES if family(n) != "unet"])
def test_walk_bits(golden, name):
    golden = golden[family(name)]
    got, want = record(name), golden["cases"][name]
    print(f"walk bits {name}: workspace {got['workspace']}, kernels {got.get('kernels')}")
    assert got["workspace"] == want["workspace"], f"{name}: workspace differs from commit {golden['parent_commit'][:12]}"
    assert got.get("kernels") == want.get("kernels"), f"{name}: launched kernels differ from commit {golden['parent_commit'][:12]}"
    assert got.get("error") == want.get("error"), f"{name}: the refusal differs from commit {golden['parent_commit'][:12]}"
    assert got.get("sha256") == want.get("sha256"), f"{name}: output bits differ from commit {golden['parent_commit'][:12]}"


@pytest.mark.parametrize("name", [n for n in CASES if family(n) == "unet"])
def test_unet_walk_bits(golden, name):
    golden = golden["unet"]
    got, want, at = record(name), golden["cases"][name], f"commit {golden['parent_commit'][:12]}"
    print(f"walk bits {name}: {json.dumps(got)}")
    assert got["workspace"] == want["workspace"], f"{name}: workspace differs from {at}"
    if CASES[name][0] == "ws_unet":
        return
    assert got["kernels"] == want["kernels"], f"{name}: launched kernels differ from {at}"
    assert [r[:2] for r in got["rows"]] == [r[:2] for r in want["rows"]], f"{name}: the profiled rows differ from {at}"
    for g, w in zip(got["rows"], want["rows"]):
        for what, a, b in (("flops", g[2], w[2]), ("bytes", g[3], w[3])):
            assert abs(a - b) <= 1e-12 * abs(b), f"{name}: row {g[0]} books {a!r} {what}, {at} booked {b!r}"
    if want["out"] is None:
        assert CASES[name][5] == "default" and want["unstable"], f"{name}: only a `default` case may go without hashes, with the reason"
        return
    for tap, sha in want["taps"].items():
        assert got["taps"][tap] == sha, f"{name}: tap {tap} is the first tensor whose bits differ from {at}"
    assert sorted(got["taps"]) == sorted(want["taps"])
    assert got["out"] == want["out"], f"{name}: output bits differ from {at}"
