"""The stream contract of the C ABI: "Enqueues on `stream`, no host synchronisation, no allocation" (include/casync_hip.h),
and "on torch's current stream and does not synchronise" of the Python wrappers.

The arithmetic tests all run on torch's null stream, or start from a synchronised device, where a launch, memset or copy sent
to the wrong stream still sees the right data.  Here every call runs on a side stream BEHIND a long row of matrix products
(busy), and everything it reads is put in place by copies enqueued behind them as well:

  * a stream that runs independently of the null stream is found first (independent_streams: the positive control -- work on
    stream 0 overtakes the busy side stream, so work WRONGLY sent to stream 0 would too);
  * run_behind(adapter) computes `ref` on the idle null stream, then repeats the call on the side stream behind busy(): what ran
    early read the other input X' (or was undone by the copies that restore the buffers), what was not joined leaves X' results
    in the snapshot taken right behind the call; the host must come back while the matrix products are still running
    (`pending`) where the contract says the entry does not synchronise.

Every byte a kernel can read at any moment was written by a correct earlier run (X, X' or their results): buffers start as
zeros and go through the same history (zeros, X' call, X call) on both streams, so that regions an entry leaves unwritten by
contract compare equal too.

ADAPTERS / LEDGER_CASES / EXEMPT classify every entry of the header that takes a casync_stream
(tests/test_stream_contract.py closes the set on any machine).  The LEDGER_CASES leg is weaker: a ledger case uploads its
operands with blocking copies before its call, so it proves that the entry works on a non-null stream behind other work, not
that the host comes back early -- it has no `pending` assertion.

Nothing here touches a GPU at import."""
from __future__ import annotations

import functools
import importlib
import math
import os
import re
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "casync_hip.h")

MM_N = 4096            # busy(): fp32 products of two MM_N x MM_N matrices
FACTOR = 10.0          # the busy delay is at least FACTOR x the idle wall time of the call (host enqueue time <= that wall time)
FLOOR_MS = 20.0        # ... and at least this long: a few hundred microseconds of delay would measure the host's jitter
PROBE_MS = 50.0        # the delay of the positive control
CANDIDATES = 8         # streams of torch.cuda.Stream() the control tries
DEV = "cuda:0"

_state: dict = {}
TABLE: list = []       # (adapter, delay_ms, t_idle_ms, R) of this session, as printed


def _t():
    import torch
    return torch


# ====================================================================================================== the header
def stream_entries(path: str = HEADER):
    """every function the header declares with a casync_stream parameter, in order"""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return [m.group(1) for m in re.finditer(r"\b(casync_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
            if re.search(r"\bcasync_stream\b", m.group(2))]


# ====================================================================================================== busy streams
def _mats():
    if "mats" not in _state:
        torch = _t()
        a = torch.rand(MM_N, MM_N, generator=torch.Generator().manual_seed(7)).to(DEV)
        _state["mats"] = (a, a.t().contiguous(), {})
        torch.cuda.synchronize()
    return _state["mats"]


def _product_of(stream):
    """the product matrix of one stream, allocated once (two busy streams do not write one buffer)"""
    torch = _t()
    outs = _mats()[2]
    if stream.cuda_stream not in outs:
        outs[stream.cuda_stream] = torch.zeros(MM_N, MM_N, device=DEV)
        torch.cuda.synchronize()
    return outs[stream.cuda_stream]


def busy(stream, repeats: int):
    """`repeats` fp32 products of two 4096 x 4096 matrices on `stream`, a marker event right behind them -> the marker"""
    torch = _t()
    a, b, _ = _mats()
    c = _product_of(stream)
    with torch.cuda.stream(stream):
        for _ in range(int(repeats)):
            torch.mm(a, b, out=c)
        marker = torch.cuda.Event(enable_timing=True)
        marker.record(stream)
    return marker


def mm_ms() -> float:
    """one product on the idle device, measured once per session with events"""
    if "mm_ms" not in _state:
        torch = _t()
        s = torch.cuda.current_stream()
        busy(s, 2).synchronize()
        start = torch.cuda.Event(enable_timing=True)
        start.record(s)
        marker = busy(s, 8)
        marker.synchronize()
        _state["mm_ms"] = max(start.elapsed_time(marker) / 8.0, 1e-3)
        print(f"stream contract: one {MM_N}^3 fp32 product takes {_state['mm_ms']:.3f} ms")
    return _state["mm_ms"]


def measured_delay(stream, repeats: int) -> float:
    """busy(stream, repeats) alone on the idle device, in ms"""
    torch = _t()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    start.record(stream)
    marker = busy(stream, repeats)
    marker.synchronize()
    return start.elapsed_time(marker)


def _runs_ahead(stream) -> bool:
    """the positive control on one stream: a tiny copy on the null stream completes while the busy stream's marker is pending"""
    torch = _t()
    null = torch.cuda.default_stream()
    busy(stream, 1).synchronize()                     # (the BLAS handle and workspace of this stream exist from here on)
    src, dst = _state.setdefault("tiny", (torch.ones(16, device=DEV), torch.zeros(16, device=DEV)))
    torch.cuda.synchronize()
    marker = busy(stream, math.ceil(PROBE_MS / mm_ms()))
    with torch.cuda.stream(null):
        dst.copy_(src, non_blocking=True)
        done = torch.cuda.Event()
        done.record(null)
    done.synchronize()
    ahead = not marker.query()
    stream.synchronize()
    return ahead


def independent_streams(n: int = 1):
    """the first n of up to CANDIDATES pooled streams on which the positive control holds; AssertionError when there are fewer
    (the tests that need them then FAIL with that message: a skip would hide the whole file)"""
    torch = _t()
    found = _state.setdefault("sides", [])
    while len(found) < n and _state.get("tried", 0) < CANDIDATES:
        _state["tried"] = _state.get("tried", 0) + 1
        s = torch.cuda.Stream()
        if all(s.cuda_stream != f.cuda_stream for f in found) and _runs_ahead(s):
            found.append(s)
    assert len(found) >= n, (f"stream contract: {len(found)} of {_state.get('tried', 0)} pooled streams run independently of the null "
                             f"stream, {n} needed: work on stream 0 does not overtake a busy side stream here, so a misplaced launch "
                             f"could not be told from a right one")
    return found[:n]


def independent_stream():
    return independent_streams(1)[0]


# ====================================================================================================== the protocol
class Adapter:
    """One call of the product under the protocol.  entries: the C-ABI functions it covers.  nosync: the contract of what it
    calls says it does not synchronise the host (`pending` is asserted); where False, `reason` says why.  Results are compared
    with torch.equal throughout: every adapter's own suite asserts run-to-run bits (the handles, the codecs, audio, the byte
    movers, and stream-K's fixed-order recombination in tests/test_ops_gpu.py)."""
    name = ""
    entries: tuple = ()
    nosync = True
    reason = ""

    def setup(self):                 # handles and weights, made once on the idle device
        pass

    def make(self, seed: int) -> dict:      # host inputs: {name: CPU tensor for self.inp[name], anything else for the adapter}
        raise NotImplementedError

    def buffers(self):               # self.inp / self.own: every device tensor the call reads / owns (scratch and outputs), zeros
        self.inp, self.own = {}, {}

    def load(self, host: dict):      # (blocking copies: steps 1 and 2 only)
        self.host = host
        for k, v in self.inp.items():
            v.copy_(host[k])

    def call(self):                  # reads torch's current stream as the product does
        raise NotImplementedError

    def outputs(self) -> list:       # device tensors, valid on the current stream right behind call()
        return []

    def finish(self) -> list:        # host results of a wrapper that waits by contract (read after `pending`)
        return []

    def close(self):
        pass


def _zeros(shape, dtype=None):
    torch = _t()
    return torch.zeros(shape, dtype=dtype or torch.float32, device=DEV)


def _as_tensors(values):
    torch = _t()
    return [v.clone() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v).copy()) for v in values]


def run_behind(adapters, sides=None):
    """The protocol on one adapter (or on several, each on a side stream of its own, called in turn).  Returns nothing; every
    assertion names the adapter."""
    torch = _t()
    adapters = list(adapters) if isinstance(adapters, (list, tuple)) else [adapters]
    sides = list(sides) if sides is not None else independent_streams(len(adapters))
    null = torch.cuda.default_stream()
    label = "+".join(a.name for a in adapters)
    for a in adapters:
        a.setup()
    X = [a.make(0) for a in adapters]
    Xp = [a.make(1) for a in adapters]
    try:
        # ---- 1: the null stream.  zeros -> X' call (lazy initialisation happens here) -> X call, timed -> ref
        for a, xp in zip(adapters, Xp):
            a.buffers()
            a.load(xp)
            a.call()
            a.finish()
        torch.cuda.synchronize()
        for a, x in zip(adapters, X):
            a.load(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        refs = []
        for a in adapters:
            a.call()
            refs.append([a.outputs(), None])
        for a, r in zip(adapters, refs):
            r[1] = a.finish()
        torch.cuda.synchronize()
        t_idle_ms = (time.perf_counter() - t0) * 1e3
        refs = [[o.clone() for o in outs] + _as_tensors(fin) for outs, fin in refs]
        torch.cuda.synchronize()

        # ---- the delay: at least FACTOR x t_idle, measured alone with events
        need = max(FACTOR * t_idle_ms, FLOOR_MS)
        R = math.ceil(1.2 * need / mm_ms())
        for _ in range(3):
            delay_ms = min(measured_delay(s, R) for s in sides)
            if delay_ms >= need:
                break
            R = math.ceil(1.3 * R * need / max(delay_ms, 1e-3))
        print(f"stream contract: {label}: delay_ms {delay_ms:.1f} t_idle_ms {t_idle_ms:.2f} R {R}")
        TABLE.append((label, delay_ms, t_idle_ms, R))
        assert delay_ms >= need, f"{label}: {R} products delay the side stream {delay_ms:.1f} ms, under {need:.1f} ms"

        # ---- 2: the side streams, idle.  fresh zeros -> X staged -> X' call -> snapshot of everything the caller owns
        staged, own_snap, snaps = [], [], []
        for a, s, x, xp in zip(adapters, sides, X, Xp):
            with torch.cuda.stream(s):
                a.buffers()
                a.load(x)
                staged.append({k: v.clone() for k, v in a.inp.items()})
                a.load(xp)
                a.call()
                outs = a.outputs()
                s.synchronize()
                a.finish()
                own_snap.append({k: v.clone() for k, v in a.own.items()})
                snaps.append([torch.empty_like(o) for o in outs])
                s.synchronize()
        torch.cuda.synchronize()

        # ---- 3: behind the busy streams
        idle = torch.cuda.Event()
        idle.record(null)
        markers = [busy(s, R) for s in sides]
        for a, s, x, st, ow, sn in zip(adapters, sides, X, staged, own_snap, snaps):
            with torch.cuda.stream(s):
                for k, v in a.inp.items():
                    v.copy_(st[k], non_blocking=True)
                for k, v in a.own.items():
                    v.copy_(ow[k], non_blocking=True)
                a.host = x
                a.call()
                outs = a.outputs()
                assert [tuple(o.shape) for o in outs] == [tuple(b.shape) for b in sn], f"{a.name}: output shapes changed"
                for b, o in zip(sn, outs):
                    b.copy_(o, non_blocking=True)
                end = torch.cuda.Event()
                end.record(s)
        # ---- 4: the host is back; are the products still running?
        pending = [not m.query() for m in markers]
        null_idle = idle.query() and null.query()
        fins = [a.finish() for a in adapters]
        # ---- 5
        for s in sides:
            s.synchronize()
        torch.cuda.synchronize()
        for a, ref, sn, fin, p in zip(adapters, refs, snaps, fins, pending):
            got = sn + _as_tensors(fin)
            assert len(got) == len(ref), f"{a.name}: {len(got)} results, {len(ref)} on the null stream"
            for i, (g, r) in enumerate(zip(got, ref)):
                assert g.shape == r.shape and g.dtype == r.dtype, f"{a.name}: result {i} is {g.dtype} {tuple(g.shape)}, not {r.dtype} {tuple(r.shape)}"
                same = torch.equal(g.cpu(), r.cpu())
                assert same, (f"{a.name}: result {i} behind a busy stream differs from the null-stream run in "
                              f"{int((g.cpu() != r.cpu()).sum())} of {g.numel()} values: something ran early, or was not joined")
            assert null_idle, f"{a.name}: the null stream was not idle"
            if a.nosync:
                assert p, (f"{a.name}: the call came back only after the side stream's {delay_ms:.0f} ms of products had finished: "
                           f"it waited for the device")
            else:
                assert a.reason, f"{a.name}: exempt from `pending` without a reason"
    finally:
        torch.cuda.synchronize()
        for a in adapters:
            a.close()


def run_ledger_behind(module: str, case):
    """The weaker leg: a ledger case, uncached, under a busy side stream, held to the ledger's own bar."""
    torch = _t()
    side = independent_stream()
    importlib.import_module(module)
    busy(side, math.ceil(FLOOR_MS / mm_ms()))
    try:
        with torch.cuda.stream(side):
            out = case.fn(*case.params)
            side.synchronize()
    finally:
        torch.cuda.synchronize()
    print(f"{case}: {out.what}: err {out.err:.3e} (bar {out.bar:.1e})")
    assert out.err <= out.bar, f"{out.what} on a side stream: error {out.err:.3e} above {out.bar:.1e}"


# ====================================================================================================== shared handles
def _stream():
    return _t().cuda.current_stream().cuda_stream


def _lib():
    from calipsync_amd import _lib as L
    return L.load()


def _ok(status, what):
    from calipsync_amd import _lib as L
    return L.check(status, what)


@functools.lru_cache(maxsize=None)
def _unet(precision):
    torch = _t()
    from calipsync_amd import recipe
    from calipsync_amd.unet import Model
    net = Model(6, "hubert", precision=precision).to(DEV)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe.make_state_dict().items()})
    return net.eval()


@functools.lru_cache(maxsize=None)
def _hubert(precision):
    import hubert_ref
    from calipsync_amd import hubert
    return hubert.HubertEngine(hubert_ref.recipe_state_dict(2), 2, DEV, precision)


@functools.lru_cache(maxsize=None)
def _s3fd(precision):
    from calipsync_amd import facedet, recipe
    return facedet.S3FDEngine(recipe.make_s3fd_state_dict(), DEV, precision)


@functools.lru_cache(maxsize=None)
def _pfld():
    from calipsync_amd import landmarks, recipe
    return landmarks.PFLDEngine(recipe.make_pfld_state_dict(), DEV)


@functools.lru_cache(maxsize=None)
def _syncnet(precision):
    from calipsync_amd import recipe, syncnet
    return syncnet.SyncNetEngine(syncnet.pack(recipe.make_syncnet_state_dict("hubert")), "hubert", DEV, precision)


def _tile(a: np.ndarray, n: int) -> np.ndarray:
    return np.ascontiguousarray(np.concatenate([a] * (-(-n // len(a))))[:n])


# ====================================================================================================== adapters
class UNet(Adapter):
    """Model.forward / forward_windows / tap, and casync_profile_forward through the model's handle.  B = 3: one lane; fp32
    B = 33: two ragged lanes (17 + 16) on the pool's streams; bf16 B = 264: the three-lane plan."""

    def __init__(self, precision, batch, kind="forward"):
        self.precision, self.batch, self.kind = precision, batch, kind
        self.name = f"unet-{precision}-b{batch}" + ("" if kind == "forward" else f"-{kind}")
        self.entries = {"forward": ("casync_forward",), "windows": ("casync_forward_windows",), "tap": ("casync_tap",),
                        "profile": ("casync_profile_forward",)}[kind]
        if kind == "profile":
            self.nosync, self.reason = False, "casync_profile_forward times every launch with events and synchronises (include/casync_hip.h)"

    def setup(self):
        self.net = _unet(self.precision)

    def make(self, seed):
        torch = _t()
        import frame_data
        from calipsync_amd import recipe
        x, a = recipe.make_inputs(min(self.batch, 11), recipe.INPUT_SEED + 17 * seed)
        h = {"x": torch.from_numpy(_tile(x, self.batch)), "a": torch.from_numpy(_tile(a, self.batch))}
        if self.kind == "windows":           # indices before the clip, inside it and past its end
            h["feat"] = torch.from_numpy(frame_data.golden_features(24, seed=3 + seed))
            h["idx"] = torch.arange(self.batch, dtype=torch.int32) * 11 - 3 + seed
            del h["a"]
        return h

    def buffers(self):
        torch = _t()
        b = self.batch
        self.inp = {"x": _zeros((b, 6, 160, 160))}
        if self.kind == "windows":
            self.inp.update(feat=_zeros((24, 2, 1024)), idx=_zeros((b,), torch.int32))
        else:
            self.inp["a"] = _zeros((b, 32, 32, 32))
        self.own = {"out": _zeros((b, 3, 160, 160))} if self.kind == "profile" else {}

    def call(self):
        i = self.inp
        if self.kind == "windows":
            self.res = [self.net.forward_windows(i["x"], i["feat"], i["idx"])]
        elif self.kind == "profile":
            from calipsync_amd import _lib as L
            net, out = self.net, self.own["out"]
            net._ensure_weights(net._device())
            ws = net._ws(self.batch, net._device())
            rows = (L.KernelTime * 1024)()
            n = _ok(_lib().casync_profile_forward(net._engine, i["x"].data_ptr(), i["a"].data_ptr(), out.data_ptr(), self.batch,
                                                  ws.data_ptr(), ws.numel(), _stream(), rows, 1024), "casync_profile_forward")
            assert n > 0
            self.res = [out]
        else:
            self.res = [self.net(i["x"], i["a"])]
            if self.kind == "tap":
                self.res.append(self.net.tap("u4", self.batch))

    def outputs(self):
        return self.res


class Hubert(Adapter):
    """HubertEngine (2 layers) on B = 2 waves of 2000 samples: the forward, or one forward_tap stage"""

    def __init__(self, precision, stage=0):
        self.precision, self.stage = precision, stage
        self.name = f"hubert-{precision}" + (f"-tap{stage}" if stage else "")
        self.entries = ("casync_hubert_forward_tap",) if stage else ("casync_hubert_forward",)

    def setup(self):
        self.eng = _hubert(self.precision)

    def make(self, seed):
        import hubert_ref
        return {"wave": _t().from_numpy(np.stack([hubert_ref.golden_wave(2000, 31 + 2 * seed + i) for i in range(2)]).astype(np.float32))}

    def buffers(self):
        self.inp, self.own = {"wave": _zeros((2, 2000))}, {}

    def call(self):
        self.res = [self.eng.forward(self.inp["wave"], self.stage, 1 if self.stage == 3 else 0)]

    def outputs(self):
        return self.res


class S3fd(Adapter):
    """S3FDEngine.forward_u8 (the tap entry at its last stage), the two forward entries on the same frames, then the candidate
    rows and the device NMS of the engine's output: B = 2 frames of 141 x 86"""
    B, H, W, CAP = 2, 141, 86, 256

    def __init__(self, precision):
        self.precision = precision
        self.name = f"s3fd-{precision}"
        self.entries = ("casync_s3fd_forward_tap", "casync_s3fd_forward_u8", "casync_s3fd_forward", "casync_op_s3fd_candidates",
                        "casync_op_s3fd_nms")

    def setup(self):
        self.eng = _s3fd(self.precision)

    def make(self, seed):
        from calipsync_amd import facedet, recipe
        u8 = recipe.make_s3fd_inputs(self.B, self.H, self.W, recipe.S3FD_INPUT_SEED + 5 * seed)
        f32 = (u8.astype(np.float32) - facedet.IMG_MEAN).transpose(0, 3, 1, 2).copy()
        return {"u8": _t().from_numpy(u8), "f32": _t().from_numpy(f32)}

    def buffers(self):
        torch = _t()
        from calipsync_amd import face_ops, facedet
        b, p = self.B, facedet.n_priors(self.H, self.W)
        self.inp = {"u8": _zeros((b, self.H, self.W, 3), torch.uint8), "f32": _zeros((b, 3, self.H, self.W))}
        self.own = {"det": _zeros((b, p, 5)), "det_u8": _zeros((b, p, 5)), "det_f32": _zeros((b, p, 5)),
                    "counts": _zeros((b,), torch.int32), "rows": _zeros((b, self.CAP, 5)), "status": _zeros((b,), torch.int32),
                    "faces": _zeros((b, face_ops.NMS_TOP_K, 5), torch.float64)}

    def call(self):
        from calipsync_amd import face_ops, facedet
        e, i, o, lib = self.eng, self.inp, self.own, _lib()
        det = e.forward_u8(i["u8"], out=o["det"])
        ws = e._workspace(self.B, self.H, self.W)
        nbytes = ws.numel() * ws.element_size()
        _ok(lib.casync_s3fd_forward_u8(e._h, i["u8"].data_ptr(), self.B, self.H, self.W, o["det_u8"].data_ptr(), ws.data_ptr(), nbytes,
                                       _stream()), "casync_s3fd_forward_u8")
        _ok(lib.casync_s3fd_forward(e._h, i["f32"].data_ptr(), self.B, self.H, self.W, o["det_f32"].data_ptr(), ws.data_ptr(), nbytes,
                                    _stream()), "casync_s3fd_forward")
        face_ops.s3fd_candidates(det, facedet.CONF_THRESH, self.CAP, counts=o["counts"], rows=o["rows"])
        face_ops.s3fd_nms(o["counts"], o["rows"], self.W, self.H, 0.5, status=o["status"], faces=o["faces"])

    def outputs(self):
        return [self.own[k] for k in ("det", "det_u8", "det_f32", "counts", "rows", "status", "faces")]


class Pfld(Adapter):
    """PFLDEngine.forward_u8 (the tap entry at its last stage) and the two forward entries on B = 3 crops, then
    casync_op_landmarks_finalize on the engine's rows"""
    B = 3
    name = "pfld"
    entries = ("casync_pfld_forward_tap", "casync_pfld_forward_u8", "casync_pfld_forward", "casync_op_landmarks_finalize")

    def setup(self):
        self.eng = _pfld()

    def make(self, seed):
        import face_cases
        from calipsync_amd import recipe
        u8 = recipe.make_pfld_inputs(self.B, recipe.PFLD_INPUT_SEED + 3 * seed)
        f32 = (u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2).copy()
        _, mean, table = face_cases.finalize_inputs(self.B)
        return {"u8": _t().from_numpy(u8), "f32": _t().from_numpy(f32), "mean": _t().from_numpy(mean + np.float32(seed)), "table": table}

    def buffers(self):
        torch = _t()
        b = self.B
        self.inp = {"u8": _zeros((b, 192, 192, 3), torch.uint8), "f32": _zeros((b, 3, 192, 192)), "mean": _zeros((220,))}
        self.own = {"y": _zeros((b, 220)), "y_u8": _zeros((b, 220)), "y_f32": _zeros((b, 220)), "lms": _zeros((b, 110, 2), torch.int32)}

    def call(self):
        from calipsync_amd import face_ops
        e, i, o, lib = self.eng, self.inp, self.own, _lib()
        y = e.forward_u8(i["u8"], out=o["y"])
        ws = e._workspace(self.B)
        nbytes = ws.numel() * ws.element_size()
        _ok(lib.casync_pfld_forward_u8(e._h, i["u8"].data_ptr(), self.B, o["y_u8"].data_ptr(), ws.data_ptr(), nbytes, _stream()),
            "casync_pfld_forward_u8")
        _ok(lib.casync_pfld_forward(e._h, i["f32"].data_ptr(), self.B, o["y_f32"].data_ptr(), ws.data_ptr(), nbytes, _stream()),
            "casync_pfld_forward")
        face_ops.landmarks_finalize(y, i["mean"], self.host["table"], out=o["lms"])

    def outputs(self):
        return [self.own[k] for k in ("y", "y_u8", "y_f32", "lms")]


class SyncNet(Adapter):
    """SyncNetEngine.forward (B = 257 walks the batch in two passes), one tap of each encoder, and casync_op_sync_curve on the
    embeddings"""

    def __init__(self, precision, batch):
        self.precision, self.batch = precision, batch
        self.name = f"syncnet-{precision}-b{batch}"
        self.entries = ("casync_sync_forward", "casync_sync_forward_tap", "casync_op_sync_curve")

    def setup(self):
        self.eng = _syncnet(self.precision)

    def make(self, seed):
        from calipsync_amd import recipe
        x, a = recipe.make_syncnet_inputs(min(self.batch, 5), "hubert", recipe.SYNCNET_INPUT_SEED + 7 * seed)
        return {"face": _t().from_numpy(_tile(x, self.batch)), "audio": _t().from_numpy(_tile(a, self.batch))}

    def buffers(self):
        self.inp, self.own = {"face": _zeros((self.batch, 3, 160, 160)), "audio": _zeros((self.batch, 32, 32, 32))}, {}

    def call(self):
        from calipsync_amd import syncnet
        i = self.inp
        a_emb, f_emb = self.eng.forward(i["face"], i["audio"])
        self.res = [a_emb, f_emb, syncnet.shift_similarity(f_emb, a_emb, min(3, syncnet.MAX_SHIFT))]
        if self.batch <= 8:
            last_face = max(k for k, n in enumerate(syncnet.STAGES) if n.startswith("face"))
            last_audio = max(k for k, n in enumerate(syncnet.STAGES) if not n.startswith("face"))
            self.res += [self.eng.tap(last_face, i["face"]), self.eng.tap(last_audio, i["audio"])]

    def outputs(self):
        return self.res


class AudioOps(Adapter):
    """casync_op_audio_resample + casync_op_audio_normalize on device PCM: 44.1 kHz stereo 16-bit, 20 000 frames (several resample
    workgroups, 7257 samples = two moments blocks, so three normalise kernels)"""
    name = "audio-ops"
    entries = ("casync_op_audio_resample", "casync_op_audio_normalize")
    RATE, FRAMES = 44100, 20000

    def pcm(self, seed):
        return np.random.default_rng(900 + seed).integers(-32768, 32768, (self.FRAMES, 2), dtype=np.int64).astype(np.int16)

    def make(self, seed):
        from calipsync_amd import audio
        return {"raw": _t().from_numpy(audio.pcm_bytes(self.pcm(seed), 2).copy())}

    def buffers(self):
        self.inp, self.own = {"raw": _zeros((self.FRAMES * 4,), _t().uint8)}, {}

    def call(self):
        from calipsync_amd import audio
        up, down = audio.ratio(self.RATE)
        wave = audio.resample_device(self.inp["raw"], 2, 2, "mean", up, down, audio.taps_device(self.RATE, DEV))
        self.res = [wave, audio.normalize_device(wave)]

    def outputs(self):
        return self.res


class AudioFrontend(AudioOps):
    """audio.frontend_device on the same PCM, from host integers"""
    name = "audio-frontend"
    entries = ()
    nosync = False
    reason = "frontend_device uploads pageable host PCM with a blocking copy and promises nothing else; its two operators are held by audio-ops"

    def make(self, seed):
        return {"pcm": self.pcm(seed)}

    def buffers(self):
        self.inp, self.own = {}, {}

    def call(self):
        from calipsync_amd import audio
        self.res = list(audio.frontend_device(self.host["pcm"], self.RATE, 2, "mean", DEV))


class JpegEncode(Adapter):
    """jpeg.encode_jpeg_op on B = 3 frames of 48 x 64 (two-stage: code the rows, then pack them behind the offsets)"""

    def __init__(self, subsampling):
        self.sub = subsampling
        self.name = "jpeg-encode-" + subsampling.replace(":", "")
        self.entries = ("casync_op_jpeg420_encode",) if subsampling == "4:2:0" else ("casync_op_jpeg_encode",)

    def make(self, seed):
        import jpeg_decode_cases
        gen = jpeg_decode_cases.generator()
        return {"frames": _t().from_numpy(np.stack([gen.frame(k, 48, 64) for k in (("noise", "smooth", "noise") if seed else ("smooth", "noise", "smooth"))]).copy())}

    def buffers(self):
        torch = _t()
        from calipsync_amd import jpeg
        B, H, W = 3, 48, 64
        self.slot = jpeg.default_slot_bytes(W, self.sub)
        sub = jpeg._subsampling(self.sub)
        need = getattr(_lib(), jpeg._entry("workspace_bytes", sub))(B, H, W, self.slot)
        assert need > 0
        cap = B * (jpeg.HEADER_BYTES + jpeg.restart_rows(H, self.sub) * self.slot)
        self.inp = {"frames": _zeros((B, H, W, 3), torch.uint8)}
        self.own = {"scratch": _zeros((need,), torch.uint8), "out": _zeros((cap,), torch.uint8), "offsets": _zeros((B + 1,), torch.int64),
                    "status": _zeros((B,), torch.int32)}

    def call(self):
        from calipsync_amd import jpeg
        o = self.own
        jpeg.encode_jpeg_op(self.inp["frames"], 90, self.slot, o["scratch"], o["out"], o["offsets"], o["status"], self.sub)

    def outputs(self):
        return [self.own[k] for k in ("out", "offsets", "status")]


class JpegEncodeDevice(Adapter):
    """jpeg.encode_jpeg_device: the files only"""
    name = "jpeg-encode-device"
    entries = ()
    nosync = False
    reason = "encode_jpeg_device returns the files' bytes: it waits for the offsets, then for the data (its docstring)"
    make = JpegEncode.make

    def buffers(self):
        self.inp, self.own = {"frames": _zeros((3, 48, 64, 3), _t().uint8)}, {}

    def call(self):
        from calipsync_amd import jpeg
        self.files = jpeg.encode_jpeg_device(self.inp["frames"], 90, subsampling="4:2:0")

    def finish(self):
        return [np.frombuffer(b"".join(self.files), dtype=np.uint8), np.asarray([len(f) for f in self.files])]


class JpegDecode(Adapter):
    """jpeg.decode_jpeg_op (coefficient memset, entropy rounds, IDCT + colour) at chunk_bits 32.  baseline: B = 4 of 48 x 64;
    mjpeg: mjpeg_decode_cases.mixed_batch(), one file of each sampling; rounds: B = 65 of the 8 x 16 4:2:2 file, which crosses
    FRAMES_PER_LAUNCH and makes two launch rounds"""

    def __init__(self, which):
        self.which = which
        self.name = "jpeg-decode-" + which
        self.entries = ("casync_op_jpegdec_decode",) if which == "baseline" else ("casync_op_mjpegdec_decode",) if which == "mjpeg" else ()

    def files(self, seed):
        import jpeg_decode_cases as jd
        import mjpeg_decode_cases as mj
        if self.which == "baseline":
            names = ["noise_48x64_default", "smooth_48x64_default", "noise_48x64_sub0", "smooth_48x64_default"]
            return [jd.case(n)[0] for n in (names[::-1] if seed else names)], "baseline"
        if self.which == "mjpeg":
            files = [f for f, _, _ in mj.mixed_batch()]
            return (files[::-1] if seed else files), "mjpeg"
        a, b = mj.case("c422noise_8x16_default")[0], mj.case("c422smooth_8x16_default")[0]
        return [b if (i + seed) % 2 else a for i in range(65)], "mjpeg"

    def setup(self):
        from calipsync_amd import jpeg
        self.plans = [jpeg.plan_decode(self.files(seed)[0], 32, subset=self.files(seed)[1]) for seed in (0, 1)]
        p = self.plans[0]
        self.B, self.H, self.W = len(p.infos), p.H, p.W
        assert (self.H, self.W) == (self.plans[1].H, self.plans[1].W) and self.H > 0
        self.blob = max(pl.blob.size for pl in self.plans)
        self.need = max(jpeg.workspace_bytes(pl, self.B, self.H, self.W) for pl in self.plans)

    def make(self, seed):
        blob = np.zeros(self.blob, dtype=np.uint8)
        blob[:self.plans[seed].blob.size] = self.plans[seed].blob
        return {"data": _t().from_numpy(blob), "plan": self.plans[seed]}

    def buffers(self):
        torch = _t()
        self.inp = {"data": _zeros((self.blob,), torch.uint8)}
        self.own = {"scratch": _zeros((max(self.need, 16),), torch.uint8), "out": _zeros((self.B, self.H, self.W, 3), torch.uint8),
                    "status": _zeros((self.B,), torch.int32)}

    def call(self):
        from calipsync_amd import jpeg
        o = self.own
        jpeg.decode_jpeg_op(self.host["plan"], self.inp["data"], o["scratch"], o["out"], o["status"], self.H, self.W)

    def outputs(self):
        return [self.own["out"], self.own["status"]]


class JpegDecodeDevice(Adapter):
    """jpeg.decode_jpeg_device on three 48 x 64 files, the middle one outside the baseline subset (4:2:2: the Pillow fallback)"""
    name = "jpeg-decode-device"
    entries = ()
    nosync = False
    reason = "decode_jpeg_device reads the status words back before it returns, and uploads Pillow's pixels with blocking copies"

    def make(self, seed):
        import jpeg_decode_cases as jd
        import mjpeg_decode_cases as mj
        a, b = jd.case("noise_48x64_default")[0], jd.case("smooth_48x64_default")[0]
        return {"files": [b if seed else a, mj.case("c422smooth_48x64_default")[0], a if seed else b]}

    def call(self):
        from calipsync_amd import jpeg
        self.res = [jpeg.decode_jpeg_device(self.host["files"], device=DEV, chunk_bits=32)]

    def outputs(self):
        return self.res


class FrameLoop(Adapter):
    """frame_loop.submit_batch_device on two 270 x 360 frames (one with a mask): pinned upload, casync_frame_prepare, the model,
    casync_frame_paste_back with its two memsets, pinned download; result() after `pending`"""
    name = "frame-loop"
    entries = ("casync_frame_prepare", "casync_frame_paste_back")

    def setup(self):
        self.net = _unet("fp32")

    def make(self, seed):
        import frame_data
        imgs, lms, masks = frame_data.make_frames(2, 270, 360, seed=40 + seed, with_masks=True)
        w = np.random.default_rng(50 + seed).standard_normal((2, 32, 32, 32)).astype(np.float32)
        return {"windows": _t().from_numpy(w), "frames": (imgs, lms, masks)}

    def buffers(self):
        self.inp, self.own = {"windows": _zeros((2, 32, 32, 32))}, {}

    def call(self):
        from calipsync_amd import frame_loop
        imgs, lms, masks = self.host["frames"]
        self.batch = frame_loop.submit_batch_device(self.net, imgs, lms, masks, windows=self.inp["windows"])

    def finish(self):
        return [np.stack(self.batch.result())]


class CropToInput(Adapter):
    """casync_op_crop_to_input through frame_loop.crops_to_model_input (the entry the host-resize path uses; its kernel also
    runs inside casync_frame_prepare)"""
    name = "crop-to-input"
    entries = ("casync_op_crop_to_input",)

    def make(self, seed):
        return {"crops": _t().from_numpy(np.random.default_rng(60 + seed).integers(0, 256, (2, 168, 168, 3), dtype=np.uint8))}

    def buffers(self):
        self.inp, self.own = {"crops": _zeros((2, 168, 168, 3), _t().uint8)}, {}

    def call(self):
        from calipsync_amd import frame_loop
        self.res = [frame_loop.crops_to_model_input(self.inp["crops"])]

    def outputs(self):
        return self.res


class FaceOps(Adapter):
    """casync_op_resize_linear_u8 (the 41 x 50 quarter-scale case, B = 3) then casync_op_face_crops192 on the resized frames"""
    name = "face-ops"
    entries = ("casync_op_resize_linear_u8", "casync_op_face_crops192")
    GEOM = np.asarray([(0, -2, 1, 9, 9), (1, 3, 2, 7, 5), (2, 0, 0, 12, 10), (1, 8, 6, 11, 11)], dtype=np.int32)

    def make(self, seed):
        import face_cases
        return {"src": _t().from_numpy(np.stack([face_cases.image(41, 50, "stream contract", seed, b) for b in range(3)]))}

    def buffers(self):
        torch = _t()
        self.inp = {"src": _zeros((3, 41, 50, 3), torch.uint8)}
        self.own = {"small": _zeros((3, 10, 12, 3), torch.uint8), "crops": _zeros((len(self.GEOM), 192, 192, 3), torch.uint8)}

    def call(self):
        from calipsync_amd import face_ops
        assert face_ops.scaled_size(41, 50, 0.25) == (12, 10)
        small = face_ops.resize_frames_u8(self.inp["src"], fx=0.25, out=self.own["small"])
        face_ops.face_crops192(small, self.GEOM, out=self.own["crops"])

    def outputs(self):
        return [self.own["small"], self.own["crops"]]


class Clip(Adapter):
    """ResidentClip.submit (gather, frame_prepare, the model, paste_back, compose) and fetch, B = 4 of a 6-frame 48 x 64 clip.
    download=False: result_device() behind the call; download=True: result() after `pending`"""

    def __init__(self, download):
        self.download = download
        self.name = "resident-clip" + ("-download" if download else "")
        self.entries = ("casync_op_clip_gather", "casync_op_clip_compose")     # (submit does not wait; result() is read after `pending`)

    def setup(self):
        import frame_data
        from calipsync_amd.resident_clip import ResidentClip
        self.net = _unet("fp32")
        self.clips = []
        for seed in (0, 1):
            imgs, lms, _ = frame_data.make_frames(6, 48, 64, seed=70 + seed)
            self.clips.append(ResidentClip(imgs, lms, None, DEV))
        assert not self.clips[0].geometry.empty.any() and self.clips[0].geometry.valid.any(), "the clip synthesises nothing"

    def make(self, seed):
        w = np.random.default_rng(80 + seed).standard_normal((4, 32, 32, 32)).astype(np.float32)
        return {"windows": _t().from_numpy(w), "frames": self.clips[seed].frames.cpu().clone()}

    def buffers(self):
        self.inp, self.own = {"windows": _zeros((4, 32, 32, 32)), "frames": self.clips[0].frames}, {}

    def call(self):
        clip = self.clips[0]
        self.batches = [clip.submit(self.net, [3, 0, 5, 3], windows=self.inp["windows"], download=self.download),
                        clip.fetch([5, 1], download=self.download)]

    def outputs(self):
        return [] if self.download else [b.result_device() for b in self.batches]

    def finish(self):
        return [np.stack(b.result()) for b in self.batches] if self.download else []

    def close(self):
        for c in getattr(self, "clips", []):
            c.close()


class ClipFromFrames(Adapter):
    """ResidentClip.from_frames under the side stream: the pinned staging upload of face_ops.FrameStager, the crops, PFLD and the
    finalize kernel on explicit boxes, the kept frames stored; then the chunked pinned upload of ResidentClip(host frames)"""
    name = "resident-clip-from-frames"
    entries = ()
    nosync = False
    reason = "from_frames returns host landmarks (detect_landmarks_device downloads them chunk by chunk); the upload of host frames waits for its last copy before it gives the pinned buffer back"
    BOXES = [[(100, 80, 135, 120)], None, [(50, 40, 183, 170)], [(10.6, 20.9, 150.2, 135.7)]]

    def setup(self):
        import frame_data
        from calipsync_amd import landmarks, recipe
        mean = frame_data.landmarks(0.5, 0.45, 0.3, np.random.default_rng(0), jitter=0.0).astype(np.float32).reshape(-1)
        self.lm = landmarks.LandmarkDetector(state_dict=recipe.make_pfld_state_dict(), mean_face=mean, device=DEV)

    def make(self, seed):
        from calipsync_amd import recipe
        two = np.repeat(np.repeat(recipe.make_s3fd_inputs(2, 77, 93, recipe.S3FD_INPUT_SEED + 9 * seed), 4, 1), 4, 2)       # 308 x 372
        return {"bgr": [two[0], two[1], two[0][::-1].copy(), two[1][:, ::-1].copy()]}

    def call(self):
        from calipsync_amd.resident_clip import ResidentClip
        self.clip = ResidentClip.from_frames(self.host["bgr"], self.lm, boxes=self.BOXES, chunk=3)
        assert self.clip.source_index == [0, 2, 3]
        self.uploaded = ResidentClip(self.host["bgr"], [self.clip.landmarks[0]] * 4, None, DEV)

    def outputs(self):
        return [self.clip.frames, self.uploaded.frames]

    def finish(self):
        return [np.stack(self.clip.landmarks)]


class Gemm(Adapter):
    """casync_op_pw_gemm at a stream-K shape of test_pw_gemm_stream_k_remainder, two calls back to back: the process-wide
    stream-K scratch and its self-resetting counters on a non-null stream"""
    name = "pw-gemm-stream-k"
    entries = ("casync_op_pw_gemm",)
    M, N, K = 1111, 512, 256

    def make(self, seed):
        torch = _t()
        g = torch.Generator().manual_seed(self.M + self.N + self.K + seed)
        return {"a": torch.randn(self.M, self.K, generator=g), "w": torch.randn(self.N, self.K, generator=g) / self.K ** 0.5,
                "b": torch.randn(self.N, generator=g), "pre": torch.randn(self.M, self.N, generator=g)}

    def buffers(self):
        m, n, k = self.M, self.N, self.K
        self.inp = {"a": _zeros((m, k)), "w": _zeros((n, k)), "b": _zeros((n,)), "pre": _zeros((m, n))}
        self.own = {"c1": _zeros((m, n)), "c2": _zeros((m, n))}

    def call(self):
        i, o, lib = self.inp, self.own, _lib()
        m, n, k = self.M, self.N, self.K
        _lib().casync_op_set_dtype(0)
        _ok(lib.casync_op_pw_gemm(i["a"].data_ptr(), k, i["w"].data_ptr(), i["b"].data_ptr(), o["c1"].data_ptr(), n, m, n, k, 1,
                                  i["pre"].data_ptr(), n, 0, 0, 0, 0, 0, _stream()), "casync_op_pw_gemm")
        _ok(lib.casync_op_pw_gemm(i["a"].data_ptr(), k, i["w"].data_ptr(), i["b"].data_ptr(), o["c2"].data_ptr(), n, m, n, k, 1,
                                  o["c1"].data_ptr(), n, 0, 0, 0, 0, 0, _stream()), "casync_op_pw_gemm")

    def outputs(self):
        return [self.own["c1"], self.own["c2"]]


def adapters() -> dict:
    """{name: factory}: every adapter of the issue's list, made fresh for each test"""
    out = {}

    def add(factory):
        out[factory().name] = factory

    for args in (("fp32", 3), ("fp32", 33), ("bf16", 3), ("bf16", 264), ("fp32", 3, "windows"), ("fp32", 3, "tap"), ("fp32", 3, "profile")):
        add(functools.partial(UNet, *args))
    for args in (("fp32",), ("bf16",), ("fp32", 2)):
        add(functools.partial(Hubert, *args))
    for p in ("fp32", "bf16"):
        add(functools.partial(S3fd, p))
    add(Pfld)
    for args in (("fp32", 2), ("bf16", 2), ("fp32", 257)):
        add(functools.partial(SyncNet, *args))
    add(AudioOps)
    add(AudioFrontend)
    for sub in ("4:4:4", "4:2:0"):
        add(functools.partial(JpegEncode, sub))
    add(JpegEncodeDevice)
    for which in ("baseline", "mjpeg", "rounds"):
        add(functools.partial(JpegDecode, which))
    add(JpegDecodeDevice)
    add(FrameLoop)
    add(CropToInput)
    add(FaceOps)
    for download in (False, True):
        add(functools.partial(Clip, download))
    add(ClipFromFrames)
    add(Gemm)
    return out


PAIR = "pair-hubert-unet"      # two handles alternating on two side streams: the forward gate's path (casync_gate_enter)


def pair():
    return [Hubert("fp32"), UNet("fp32", 3)]


def _adapter_table() -> dict:
    """{entry: (adapter names)} from the adapters' own `entries`"""
    table: dict = {}
    for name, factory in adapters().items():
        for e in factory().entries:
            table.setdefault(e, []).append(name)
    return {e: tuple(v) for e, v in table.items()}


ADAPTERS = _adapter_table()


# ====================================================================================================== the single-launch entries
def _ledger_cases() -> dict:
    import kernel_ledger as kl
    import kernel_ledger_det as det
    import kernel_ledger_det16 as det16
    import kernel_ledger_hb16 as hb16
    import kernel_ledger_lmk as lmk
    import kernel_ledger_sync as sync
    import kernel_ledger_sync16 as sync16
    C, F32 = kl.C, kl.F32
    return {
        "casync_op_conv3x3_ex": ("kernel_ledger", C(kl.conv3x3, F32, 3, 9, 13, 64, 64, 1, 2, 1, -1)),
        "casync_op_dw3x3": ("kernel_ledger", C(kl.dw3x3, F32, 3, 21, 13, 8, 2)),
        "casync_op_dw3x3_ups": ("kernel_ledger", C(kl.dw3x3_ups, 3, 10, 64, 68)),
        "casync_op_pw_dw": ("kernel_ledger", C(kl.pw_dw, F32, 10, 1, 64, 128, 3)),
        "casync_op_pw_dw_rect": ("kernel_ledger", C(kl.pw_dw, F32, 16, 1, 64, 128, 1, 128, 32)),
        "casync_op_pw_gemm_ups": ("kernel_ledger", C(kl.gemm_ups, 1, 40, 32, 128)),
        "casync_op_ir_fused": ("kernel_ledger", C(kl.ir_fused, F32, 32, 32, 1, 3, 24, 40)),
        "casync_op_ir_fused_up": ("kernel_ledger", C(kl.ir_fused_up, F32, 64, 3, 20, 52, "load")),
        "casync_op_ir_fused_upg": ("kernel_ledger", C(kl.ir_fused_up, F32, 64, 3, 20, 52, "commuted")),
        "casync_op_upsample2x": ("kernel_ledger", C(kl.upsample, F32, 2, 3, 5, 4)),
        "casync_op_cross_attention": ("kernel_ledger", C(kl.cross_attention, F32, 3)),
        "casync_op_audio_windows": ("kernel_ledger", C(kl.audio_windows, F32, 1)),
        "casync_op_pred_to_u8": ("kernel_ledger", C(kl.pred_to_u8, 3)),
        "casync_op_nchw_to_nhwc": ("kernel_ledger", C(kl.nchw_to_nhwc, F32, 3, 32, 1024)),
        "casync_op_inc": ("kernel_ledger", C(kl.inc, F32, 3)),
        "casync_op_outc": ("kernel_ledger", C(kl.outc, F32, 3)),
        "casync_op_hubert_conv0": ("kernel_ledger", C(kl.hb_conv0, 2, 2007)),
        "casync_op_hubert_layernorm": ("kernel_ledger", C(kl.hb_layernorm, 512, 0, 37, "strided")),
        "casync_op_hubert_posconv": ("kernel_ledger", C(kl.hb_posconv, 3, 63)),
        "casync_op_hubert_attention": ("kernel_ledger", C(kl.hb_attention, 2, 31, False)),
        "casync_op_rows_gemm": ("kernel_ledger", C(kl.rows_gemm, 77, 4096, 1024, 1024, 3, False)),
        "casync_op_hubert16_conv0": ("kernel_ledger_hb16", C(hb16.hb16_conv0, 2, 2007)),
        "casync_op_hubert16_layernorm512": ("kernel_ledger_hb16", C(hb16.hb16_layernorm512, 0, 37, "strided")),
        "casync_op_hubert16_layernorm1024": ("kernel_ledger_hb16", C(hb16.hb16_layernorm1024, 0, 0, 1, 37, True)),
        "casync_op_hubert16_gelu": ("kernel_ledger_hb16", C(hb16.hb16_gelu, 8)),
        "casync_op_hubert16_widen": ("kernel_ledger_hb16", C(hb16.hb16_widen, 8)),
        "casync_op_hubert16_attention": ("kernel_ledger_hb16", C(hb16.hb16_attention, 2, 31, False)),
        "casync_op_rows_gemm_bf16": ("kernel_ledger_hb16", C(hb16.rows_gemm_bf16, 77, 4096, 1024, 1024)),
        "casync_op_pfld_stem": ("kernel_ledger_lmk", C(lmk.stem, 0, 2, 23, 37)),
        "casync_op_pfld_ghost": ("kernel_ledger_lmk", C(lmk.ghost, 1, 2, 7, 5, 40, 30, 0)),
        "casync_op_pfld_dw_s2": ("kernel_ledger_lmk", C(lmk.dw_s2, 2, 13, 9, 48)),
        "casync_op_pfld_head": ("kernel_ledger_lmk", C(lmk.head, 3)),
        "casync_op_s3fd_stem": ("kernel_ledger_det", C(det.stem, 1, 2, 13, 19)),
        "casync_op_s3fd_maxpool": ("kernel_ledger_det", C(det.maxpool, 1, 2, 7, 10, 256)),
        "casync_op_s3fd_im2col_dil": ("kernel_ledger_det", C(det.im2col, 2, 2, 3, 512, 6)),
        "casync_op_s3fd_relu": ("kernel_ledger_det", C(det.relu, 6 * 1024 + 4)),
        "casync_op_s3fd_l2norm": ("kernel_ledger_det", C(det.l2norm, 37, 256)),
        "casync_op_s3fd_head": ("kernel_ledger_det", C(det.head, 2, 1, 2, 256, 1)),
        "casync_op_s3fd_decode": ("kernel_ledger_det", C(det.decode, 2, 77, 93)),
        "casync_op_s3fd16_stem": ("kernel_ledger_det16", C(det16.stem, 1, 2, 13, 19)),
        "casync_op_s3fd16_maxpool": ("kernel_ledger_det16", C(det16.maxpool, 1, 2, 7, 10, 256)),
        "casync_op_s3fd16_im2col_dil": ("kernel_ledger_det16", C(det16.im2col, 2, 2, 3, 512, 6)),
        "casync_op_s3fd16_relu": ("kernel_ledger_det16", C(det16.relu, 6 * 1024 + 8)),
        "casync_op_s3fd16_widen": ("kernel_ledger_det16", C(det16.widen, 6 * 1024 + 8)),
        "casync_op_s3fd16_l2norm": ("kernel_ledger_det16", C(det16.l2norm, 37, 256)),
        "casync_op_s3fd16_head": ("kernel_ledger_det16", C(det16.head, 2, 1, 2, 256, 1)),
        "casync_op_sync_stem7": ("kernel_ledger_sync", C(sync.stem7, 2, 9, 11)),
        "casync_op_sync_conv5": ("kernel_ledger_sync", C(sync.conv5, 2, 3, 3)),
        "casync_op_sync_conv3": ("kernel_ledger_sync", C(sync.conv3, 2, 9, 11, 64, 64, 1, 1, 1, 1)),
        "casync_op_sync_relu": ("kernel_ledger_sync", C(sync.relu, 1028)),
        "casync_op_sync_to_nchw": ("kernel_ledger_sync", C(sync.to_nchw, 2, 25, 12)),
        "casync_op_sync_embed": ("kernel_ledger_sync", C(sync.embed)),
        "casync_op_sync16_stem7": ("kernel_ledger_sync16", C(sync16.stem7, 2, 9, 11)),
        "casync_op_sync16_conv5": ("kernel_ledger_sync16", C(sync16.conv, 5, 0, 2, 3, 3, 32, 64, 2, 2, 1, 0)),
        "casync_op_sync16_conv3": ("kernel_ledger_sync16", C(sync16.conv, 3, 64, 2, 5, 7, 64, 64, 1, 1, 1, 1)),
        "casync_op_sync16_conv1": ("kernel_ledger_sync16", C(sync16.conv, 1, 0, 3, 3, 3, 64, 64, 1, 1, 0, 0)),
        "casync_op_sync16_to_nchw": ("kernel_ledger_sync16", C(sync16.to_nchw, 2, 25, 12)),
    }


LEDGER_CASES = _ledger_cases()


def ledger_known(module: str):
    """every case a ledger module lists (its LEDGER, and kernel_ledger_hb16's rows-GEMM list)"""
    mod = importlib.import_module(module)
    known = [c for cs in mod.LEDGER.values() for c in cs]
    if hasattr(mod, "rows_gemm_cases"):
        known += [c for _, c in mod.rows_gemm_cases()]
    return known


EXEMPT = {
    "casync_op_conv3x3": "one line that hands its arguments and its stream to casync_op_conv3x3_ex (csrc/engine.hip), which has a ledger case",
}
