"""The workspace contract of the C ABI: the bytes of a caller-owned `workspace*` / `scratch*` on entry mean nothing, so they never
reach an output.  Every Python wrapper relies on it (engine_base._grow_workspace, Model._workspace and audio.py allocate with
torch.empty and keep the tensor across batch sizes and shapes), and almost no entry clears anything: the kernels get there by
masking their loads.

The arithmetic tests cannot see a breach: in a pytest process a handle's first workspace is usually fresh, zeroed memory, and later
forwards see that handle's own earlier, plausible results.  Here every call of an adapter runs on a workspace the test owns,
of exactly the bytes the matching *_workspace_bytes* entry answers, with a guard of GUARD bytes behind it:

  zero     all bytes 0x00: the reference
  ff       all bytes 0xFF: NaN as fp32, bf16 and float64, -1 as any integer
  7f       all bytes 0x7F: about 3.4e38, finite, as fp32 and bf16
  stale    the same memory first used by a valid call of the same entry on other input, at a batch or shape that is no larger
  foreign  the same memory first used as the workspace of another handle of the other precision (an S3FD forward)

and every output and tap of every other run equals the reference with torch.equal: the code under test against itself, so there
is no tolerance.  After every call the guard is intact, the engine held the pointer that was handed in, and the workspace differs
from what it held on entry (or the test would be empty).  An output the contract leaves partly unwritten (the JPEG `out` beyond the last
offset) starts from the fill as well; there an element also passes when it is untouched: the fill under both fills, zero in the
reference.

ADAPTERS / EXEMPT classify every entry of the header with a `workspace*` or `scratch*` parameter (tests/test_workspace_contract.py
closes the set on any machine).  Nothing here touches a GPU at import."""
from __future__ import annotations

import functools
import re
import time

import numpy as np

import stream_contract as sc
from stream_contract import DEV, HEADER, _lib, _ok, _stream, _t, _tile

GUARD = 4096
GUARD_BYTE = 0xA5
FILLS = {"zero": 0x00, "ff": 0xFF, "7f": 0x7F}
VARIANTS = ("ff", "7f", "stale", "foreign")
SECONDS: dict = {}     # (adapter, variant) -> seconds of this session, as printed


# ====================================================================================================== the header
def workspace_entries(path: str = HEADER):
    """every function the header declares with a parameter named workspace* or scratch*, in order"""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return [m.group(1) for m in re.finditer(r"\b(casync_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
            if re.search(r"\b(?:workspace|scratch)\w*\s*(?:,|$)", m.group(2).strip())]


# ====================================================================================================== the protocol
class Adapter:
    """Calls of the product on a workspace the test owns.  entries: the C-ABI functions it covers.  precision: of its handle
    ("fp32", "bf16" or None), which picks the foreign handle.  untouched_ok: its outputs have elements the contract leaves
    unwritten.  variants: the runs beside the zero-fill reference; where some are left out, `reason` says why."""
    name = ""
    entries: tuple = ()
    precision = None
    untouched_ok = False
    variants = VARIANTS
    reason = ""

    def setup(self):                          # handles, weights and the device inputs of seeds 0 and 1, made once
        pass

    def need(self) -> int:                    # what the matching *_workspace_bytes* entry answers for the calls of seed 0
        raise NotImplementedError

    def calls(self) -> list:                  # labels: each is run on a workspace prepared afresh
        return ["forward"]

    def run(self, call: str, ws, seed: int, fill: int) -> list:
        """one call on `ws` (uint8, exactly need() bytes) -> [(label, device tensor)]: its outputs, then every tap read right
        behind it.  Asserts that the engine used ws.  Outputs with unwritten elements start from `fill`."""
        raise NotImplementedError

    def prior(self, call: str, ws):           # the stale variant's earlier call: other input, no larger
        self.run(call, ws, 1, 0)

    def close(self):
        pass


def _bytes(t):
    return t.contiguous().view(-1).view(_t().uint8)


def _foreign_engine(precision):
    """the S3FD handle of the other precision (bf16 for an fp32 adapter and for one without a precision)"""
    return sc._s3fd("fp32" if precision == "bf16" else "bf16")


def _foreign_plan(precision, need: int):
    """(frames, bytes): 64 x 64 S3FD frames whose workspace covers as much of `need` as at most 6 frames do"""
    from calipsync_amd import recipe
    eng = _foreign_engine(precision)
    one = eng.workspace_bytes(1, 64, 64)
    b = max(1, min(6, need // max(one, 1)))
    return recipe.make_s3fd_inputs(b, 64, 64, recipe.S3FD_INPUT_SEED + 11), eng.workspace_bytes(b, 64, 64)


def execute(adapter: Adapter, variant: str) -> list:
    """every call of the adapter under one variant -> [(call:label, tensor)], each tensor a copy"""
    torch = _t()
    need = int(adapter.need())
    assert need > 0, f"{adapter.name}: workspace_bytes says {need}"
    total = need + GUARD
    frames = None
    if variant == "foreign":
        frames, fbytes = _foreign_plan(adapter.precision, need)
        frames = torch.from_numpy(frames).to(DEV)
        total = max(total, fbytes)
    base = torch.empty(total, dtype=torch.uint8, device=DEV)      # (the foreign handle may reach past the guard; the guard is set behind it)
    ws, guard = base[:need], base[need:need + GUARD]
    results = []
    for call in adapter.calls():
        if variant in FILLS:
            base.fill_(FILLS[variant])
        else:
            base.zero_()
            if variant == "stale":
                adapter.prior(call, ws)
            else:
                _foreign_engine(adapter.precision).forward_u8(frames, workspace=base)
            torch.cuda.synchronize()
            assert bool((ws != 0).any()), f"{adapter.name} [{variant}] {call}: the earlier call left the workspace at zero"
        guard.fill_(GUARD_BYTE)
        before = ws.clone()
        outs = adapter.run(call, ws, 0, FILLS.get(variant, 0))
        torch.cuda.synchronize()
        assert bool((guard == GUARD_BYTE).all()), f"{adapter.name} [{variant}] {call}: bytes behind the {need}-byte workspace were written"
        assert not torch.equal(ws, before), f"{adapter.name} [{variant}] {call}: the workspace is unchanged: the call did not use it"
        results += [(f"{call}:{label}", t.clone()) for label, t in outs]
    return results


_cache: dict = {}      # the latest adapter's runs by variant (the tests come adapter by adapter)


def _run_cached(adapter: Adapter, variant: str) -> list:
    if _cache.get("name") != adapter.name:
        _cache.clear()
        _cache["name"] = adapter.name
    if variant not in _cache:
        _cache[variant] = execute(adapter, variant)
    return _cache[variant]


def _first_difference(got, ref):
    bad = (got != ref) | (got != got) if got.is_floating_point() else (got != ref)
    idx = int(bad.reshape(-1).nonzero()[0])
    at = tuple(int(v) for v in np.unravel_index(idx, tuple(got.shape))) if got.dim() else ()
    return idx, at, got.reshape(-1)[idx].item(), ref.reshape(-1)[idx].item(), int(bad.sum())


def check(factory, variant: str):
    """the protocol on one adapter and one variant; every assertion names the adapter and the variant"""
    torch = _t()
    adapter = factory()
    assert variant in adapter.variants, f"{adapter.name} does not run [{variant}]: {adapter.reason}"
    t0 = time.perf_counter()
    adapter.setup()
    try:
        ref = _run_cached(adapter, "zero")
        got = _run_cached(adapter, variant) if adapter.untouched_ok and variant in FILLS else execute(adapter, variant)
        assert [l for l, _ in got] == [l for l, _ in ref], f"{adapter.name} [{variant}]: the outputs are not those of the zero-fill run"
        for (label, g), (_, r) in zip(got, ref):
            assert g.shape == r.shape and g.dtype == r.dtype, f"{adapter.name} [{variant}]: {label} is {g.dtype} {tuple(g.shape)}, not {r.dtype} {tuple(r.shape)}"
            if torch.equal(g, r):
                continue
            if adapter.untouched_ok and variant in ("ff", "7f"):
                both = {v: dict(_run_cached(adapter, v))[label] for v in ("ff", "7f")}
                gb, rb = _bytes(g), _bytes(r)
                untouched = (rb == 0) & (_bytes(both["ff"]) == 0xFF) & (_bytes(both["7f"]) == 0x7F)
                bad = (gb != rb) & ~untouched
                if not bool(bad.any()):
                    continue
                idx = int(bad.nonzero()[0])
                raise AssertionError(f"{adapter.name} [{variant}]: {label} differs from the zero-fill run first at byte {idx} "
                                     f"({int(gb[idx])} vs {int(rb[idx])}), in {int(bad.sum())} of {gb.numel()} bytes that the call wrote")
            idx, at, gv, rv, n = _first_difference(g, r)
            raise AssertionError(f"{adapter.name} [{variant}]: {label} differs from the zero-fill run first at index {idx} {at} "
                                 f"({gv!r} vs {rv!r}), in {n} of {g.numel()} values: bytes the workspace held on entry reached it")
    finally:
        torch.cuda.synchronize()
        adapter.close()
    SECONDS[(adapter.name, variant)] = time.perf_counter() - t0
    print(f"workspace contract: {adapter.name} [{variant}]: {len(ref)} outputs and taps, {SECONDS[(adapter.name, variant)]:.2f} s")


# ====================================================================================================== shared handles
@functools.lru_cache(maxsize=None)
def _unet(precision, mode):
    if mode == "hubert":
        return sc._unet(precision)
    torch = _t()
    from calipsync_amd import recipe
    from calipsync_amd.unet import WenetModel
    net = WenetModel(6, precision=precision).to(DEV)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe.make_state_dict(mode="wenet").items()})
    return net.eval()


@functools.lru_cache(maxsize=None)
def _syncnet(precision, mode):
    if mode == "hubert":
        return sc._syncnet(precision)
    from calipsync_amd import recipe, syncnet
    return syncnet.SyncNetEngine(syncnet.pack(recipe.make_syncnet_state_dict("wenet"), "wenet"), "wenet", DEV, precision)


def _dev(a):
    return _t().from_numpy(np.ascontiguousarray(a)).to(DEV)


_inputs: dict = {}     # adapter name -> its device inputs, made once a session (no call writes them)


def _memo(name, make):
    if name not in _inputs:
        _inputs[name] = make()
    return _inputs[name]


# ====================================================================================================== adapters
UNET_TAPS = ("x1", "x2", "x3", "x4", "x5", "audio_conv1", "audio_conv2", "audio_conv3", "audio_conv4", "audio_conv5", "a", "tx", "kx",
             "att0", "att1", "att2", "att3", "fuse", "u1", "u2", "u3", "u4")


class UNet(Adapter):
    """Model.forward / forward_windows / casync_profile_forward on a preset Model._workspace, then casync_tap of every name on the
    same memory.  B = 1, 5, 12: one lane with uneven tiles, the bf16 plan switch at 12.  The arena holds activations only (the
    stream-K counters are the engine's own memory, csrc/engine.hip sk_ctx), so no fill can become an index.  The stale variant's
    earlier call runs the largest smaller batch whose arena fits (B = 1: one other frame), whose buffers sit at other offsets of
    the same arena; with
    prior_batch above batch (the 9-then-4 case) the workspace is the larger batch's, as the grow-only arena of a clip is."""

    def __init__(self, precision, batch, mode="hubert", kind="forward", prior_batch=None):
        self.precision, self.batch, self.mode, self.kind = precision, batch, mode, kind
        self.prior_batch = prior_batch
        self.name = f"unet-{precision}-{mode}-b{batch}" + ("" if kind == "forward" else f"-{kind}") + \
                    (f"-after-b{prior_batch}" if prior_batch else "")
        self.entries = {"forward": ("casync_forward", "casync_tap"), "windows": ("casync_forward_windows", "casync_tap"),
                        "profile": ("casync_profile_forward", "casync_tap")}[kind]
        if prior_batch:
            self.variants, self.reason = ("stale",), "the one case that makes test_workspace_is_reused_across_batch_sizes exact"

    def _inputs(self, seed, batch):
        import frame_data
        from calipsync_amd import recipe
        x, a = recipe.make_inputs(min(batch, 12), recipe.INPUT_SEED + 17 * seed, self.mode)
        h = {"x": _dev(_tile(x, batch)), "a": _dev(_tile(a, batch))}
        if self.kind == "windows":           # indices before the clip, inside it and past its end
            h["feat"] = _dev(frame_data.golden_features(24, seed=3 + seed))
            h["idx"] = (_t().arange(batch, dtype=_t().int32) * 11 - 3 + seed).to(DEV)
        return h

    def setup(self):
        self.net = _unet(self.precision, self.mode)
        self.net._ensure_weights(self.net._device())
        if self.prior_batch is None:         # the largest smaller batch whose arena fits (the plan switch at 12 frames needs less than 11 do)
            fits = [b for b in range(1, self.batch) if self._need(b) <= self._need(self.batch)]
            self.prior_batch = max(fits) if fits else 1
        self.inp = _memo(self.name, lambda: {0: self._inputs(0, self.batch), 1: self._inputs(1, self.prior_batch)})
        self.saved = self.net._workspace

    def _need(self, batch):
        return _lib().casync_workspace_bytes_h(self.net._engine, batch)

    def need(self):
        return self._need(max(self.batch, self.prior_batch))

    def run(self, call, ws, seed, fill):
        torch = _t()
        net, i = self.net, self.inp[seed]
        batch = i["x"].shape[0]
        net._workspace = ws
        if self.kind == "windows":
            out = net.forward_windows(i["x"], i["feat"], i["idx"])
        elif self.kind == "profile":
            from calipsync_amd import _lib as L
            out = torch.zeros((batch, 3, 160, 160), dtype=torch.float32, device=DEV)
            rows = (L.KernelTime * 1024)()
            n = _ok(_lib().casync_profile_forward(net._engine, i["x"].data_ptr(), i["a"].data_ptr(), out.data_ptr(), batch, ws.data_ptr(),
                                                  ws.numel(), _stream(), rows, 1024), "casync_profile_forward")
            assert n > 0
        else:
            out = net(i["x"], i["a"])
        assert net._workspace is ws, f"{self.name}: the model replaced the {ws.numel()}-byte workspace it was given"
        res = [("out", out)]
        if seed == 0:
            res += [(f"tap {name}", net.tap(name, batch)) for name in UNET_TAPS]
            assert net._workspace is ws
        return res

    def close(self):
        self.net._workspace = self.saved


class Hubert(Adapter):
    """HubertEngine (2 layers) on a preset grow-only `_ws`: the forward, and casync_hubert_forward_tap at stage 1, 2 and 3 (after
    one layer and after two), each a call of its own.  401 and 2000 samples give T = 1 and 6 tokens (keys past T inside one
    attention tile), 720 samples T = 2 at B = 1.  The stale variant's earlier call is the same shape on other waves."""

    CALLS = {"forward": (0, 0), "tap conv": (1, 0), "tap layer0_in": (2, 0), "tap after1": (3, 1), "tap after2": (3, 2)}

    def __init__(self, precision, batch, samples):
        self.precision, self.batch, self.samples = precision, batch, samples
        self.name = f"hubert-{precision}-b{batch}-s{samples}"
        self.entries = ("casync_hubert_forward", "casync_hubert_forward_tap")

    def setup(self):
        import hubert_ref
        self.eng = sc._hubert(self.precision)
        self.inp = _memo(self.name, lambda: {seed: _dev(np.stack([hubert_ref.golden_wave(self.samples, 31 + 2 * seed + i)
                                                                    for i in range(self.batch)]).astype(np.float32)) for seed in (0, 1)})
        self.saved = self.eng._ws

    def need(self):
        return self.eng._lib.casync_hubert_workspace_bytes_h(self.eng._h, self.batch, self.samples)

    def calls(self):
        return list(self.CALLS)

    def run(self, call, ws, seed, fill):
        assert ws.numel() % 4 == 0
        mine = ws.view(_t().float32)
        self.eng._ws = mine
        stage, n_layers = self.CALLS[call]
        out = self.eng.forward(self.inp[seed], stage, n_layers)
        assert self.eng._ws is mine and mine.data_ptr() == ws.data_ptr(), f"{self.name}: the engine replaced the workspace it was given"
        return [("out", out)]

    def close(self):
        self.eng._ws = self.saved


class Pfld(Adapter):
    """PFLDEngine with workspace=: casync_pfld_forward_tap at every stage (uint8 crops; the last stage once more on float input),
    casync_pfld_forward_u8 and casync_pfld_forward through ctypes, each a call of its own."""
    precision = "fp32"
    entries = ("casync_pfld_forward_tap", "casync_pfld_forward_u8", "casync_pfld_forward")

    def __init__(self, batch):
        self.batch = batch
        self.name = f"pfld-b{batch}"

    def setup(self):
        from calipsync_amd import recipe
        self.eng = sc._pfld()
        self.inp = {}
        for seed in (0, 1):
            u8 = recipe.make_pfld_inputs(self.batch, recipe.PFLD_INPUT_SEED + 3 * seed)
            self.inp[seed] = (_dev(u8), _dev((u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)))

    def need(self):
        return self.eng.workspace_bytes(self.batch)

    def calls(self):
        from calipsync_amd import landmarks
        return [f"tap {s}" for s in landmarks.STAGES] + ["tap float", "forward_u8", "forward"]

    def _out(self):
        return _t().zeros((self.batch, 220), dtype=_t().float32, device=DEV)

    def run(self, call, ws, seed, fill):
        e, (u8, f32), own = self.eng, self.inp[seed], self.eng._ws
        if call == "tap float":
            out = e.forward(f32, workspace=ws)
        elif call.startswith("tap "):
            out = e.forward_u8(u8, stage=call[4:], workspace=ws)
        elif call == "forward_u8":
            out = self._out()
            _ok(e._lib.casync_pfld_forward_u8(e._h, u8.data_ptr(), self.batch, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), call)
        else:
            out = self._out()
            _ok(e._lib.casync_pfld_forward(e._h, f32.data_ptr(), self.batch, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), call)
        assert e._ws is own, f"{self.name}: the engine took a workspace of its own"
        return [("out", out)]


class S3fd(Adapter):
    """S3FDEngine with workspace=: casync_s3fd_forward_tap at every stage (uint8 frames; the last stage once more on float
    input), casync_s3fd_forward_u8 and casync_s3fd_forward through ctypes, each a call of its own.  One 64 x 64 frame, and the
    three 77 x 93 frames of recipe.make_s3fd_inputs (odd maps at every pool)."""
    entries = ("casync_s3fd_forward_tap", "casync_s3fd_forward_u8", "casync_s3fd_forward")

    def __init__(self, precision, batch, h, w):
        self.precision, self.batch, self.h, self.w = precision, batch, h, w
        self.name = f"s3fd-{precision}-b{batch}-{h}x{w}"

    def setup(self):
        from calipsync_amd import facedet, recipe
        self.eng = sc._s3fd(self.precision)
        self.inp = {}
        for seed in (0, 1):
            u8 = recipe.make_s3fd_inputs(self.batch, self.h, self.w, recipe.S3FD_INPUT_SEED + 5 * seed)
            self.inp[seed] = (_dev(u8), _dev((u8.astype(np.float32) - facedet.IMG_MEAN).transpose(0, 3, 1, 2)))

    def need(self):
        return self.eng.workspace_bytes(self.batch, self.h, self.w)

    def calls(self):
        from calipsync_amd import facedet
        return [f"tap {s}" for s in facedet.STAGES] + ["tap float", "forward_u8", "forward"]

    def _out(self):
        from calipsync_amd import facedet
        return _t().zeros((self.batch, facedet.n_priors(self.h, self.w), 5), dtype=_t().float32, device=DEV)

    def run(self, call, ws, seed, fill):
        e, (u8, f32), own = self.eng, self.inp[seed], self.eng._ws
        if call == "tap float":
            out = e.forward(f32, workspace=ws)
        elif call.startswith("tap "):
            out = e.forward_u8(u8, stage=call[4:], workspace=ws)
        elif call == "forward_u8":
            out = self._out()
            _ok(e._lib.casync_s3fd_forward_u8(e._h, u8.data_ptr(), self.batch, self.h, self.w, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _stream()), call)
        else:
            out = self._out()
            _ok(e._lib.casync_s3fd_forward(e._h, f32.data_ptr(), self.batch, self.h, self.w, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                           _stream()), call)
        assert e._ws is own, f"{self.name}: the engine took a workspace of its own"
        return [("out", out)]


class SyncNet(Adapter):
    """SyncNetEngine with workspace=: casync_sync_forward (both embeddings), and casync_sync_forward_tap at each of the 31 blocks,
    each a call of its own."""
    entries = ("casync_sync_forward", "casync_sync_forward_tap")

    def __init__(self, mode, precision, batch):
        self.mode, self.precision, self.batch = mode, precision, batch
        self.name = f"syncnet-{mode}-{precision}-b{batch}"

    def setup(self):
        from calipsync_amd import recipe
        self.eng = _syncnet(self.precision, self.mode)
        self.inp = {}
        for seed in (0, 1):
            x, a = recipe.make_syncnet_inputs(self.batch, self.mode, recipe.SYNCNET_INPUT_SEED + 7 * seed)
            self.inp[seed] = (_dev(x), _dev(a))

    def need(self):
        return self.eng.workspace_bytes(self.batch)

    def calls(self):
        from calipsync_amd import syncnet
        return ["forward"] + [f"tap {s}" for s in syncnet.STAGES]

    def run(self, call, ws, seed, fill):
        e, (face, audio), own = self.eng, self.inp[seed], self.eng._ws
        if call == "forward":
            a_emb, f_emb = e.forward(face, audio, workspace=ws)
            res = [("audio_emb", a_emb), ("face_emb", f_emb)]
        else:
            res = [("out", e.tap(call[4:], face if call.startswith("tap face") else audio, workspace=ws))]
        assert e._ws is own, f"{self.name}: the engine took a workspace of its own"
        return res


def _filled(shape, dtype, fill):
    torch = _t()
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(fill)
    return t


class JpegEncode(Adapter):
    """casync_op_jpeg_encode / casync_op_jpeg420_encode through jpeg.encode_jpeg_op on three 48 x 64 frames.  `out` beyond
    offsets[B] is unwritten by contract: out, offsets and status start from the fill, and an untouched byte passes.

    The scratch holds integers: the row lengths, unsigned [frame][restart row], ahead of the slots.  This call writes every one of
    them before any thread reads it: lane 0 of every (row, frame) workgroup of the rows kernel ends in close_row, which stores
    *len unconditionally (csrc/jpeg_enc.hip:178, csrc/jpeg_enc420.hip:277; csrc/jpeg_enc_common.h:217-221; neither rows kernel
    returns early), and the entry launches the rows kernels over all frames, then the plan kernel, then the pack kernels on one
    stream (jpeg_enc_common.h:426-438).  The plan kernel reads len[r] for r < rows of frames < batch only (:233-239), the pack
    kernel len[r] for r <= row of a frame whose status is 0 (:292-295, :308), and a length that is not ROW_OVERFLOW is at most
    the slot (:220).  The slots hold bytes that are copied, never indices.  So both byte fills apply."""
    untouched_ok = True

    def __init__(self, subsampling):
        self.sub = subsampling
        self.name = "jpeg-encode-" + subsampling.replace(":", "")
        self.entries = ("casync_op_jpeg420_encode",) if subsampling == "4:2:0" else ("casync_op_jpeg_encode",)

    def setup(self):
        import jpeg_decode_cases
        from calipsync_amd import jpeg
        gen = jpeg_decode_cases.generator()
        kinds = {0: ("smooth", "noise", "smooth"), 1: ("noise", "smooth", "noise")}
        self.inp = {seed: _dev(np.stack([gen.frame(k, 48, 64) for k in kinds[seed]])) for seed in (0, 1)}
        self.slot = jpeg.default_slot_bytes(64, self.sub)
        self.cap = 3 * (jpeg.HEADER_BYTES + jpeg.restart_rows(48, self.sub) * self.slot)

    def need(self):
        from calipsync_amd import jpeg
        return getattr(_lib(), jpeg._entry("workspace_bytes", jpeg._subsampling(self.sub)))(3, 48, 64, self.slot)

    def run(self, call, ws, seed, fill):
        torch = _t()
        from calipsync_amd import jpeg
        out, offsets, status = _filled((self.cap,), torch.uint8, fill), _filled((4,), torch.int64, fill), _filled((3,), torch.int32, fill)
        jpeg.encode_jpeg_op(self.inp[seed], 90, self.slot, ws, out, offsets, status, self.sub)      # (ws.data_ptr() and ws.numel() go to the entry)
        return [("out", out), ("offsets", offsets), ("status", status)]


class JpegDecode(Adapter):
    """casync_op_jpegdec_decode / casync_op_mjpegdec_decode through jpeg.decode_jpeg_op at chunk_bits 32 on three 48 x 64 files
    whose scans end early (cut at a half, a third and two thirds of their length), so that the blocks behind the cut stay at the
    coefficient memset's zero and reach the IDCT as they are.  baseline: 4:2:0, 4:2:0, 4:4:4; mjpeg: 4:2:2, grayscale, 4:2:0.
    Every frame is decoded (status 2 comes from the device), so no element of `out` is left unwritten.

    The scratch holds integers: 64 bytes of scan state (SubState) per subsequence, ahead of the coefficients and the sample
    planes.  This call writes every one of them before any thread reads it: the sync kernel's workgroup of a frame stores a whole
    zero-initialised SubState to subs[g] for every g < nsub and passes a barrier (csrc/jpeg_dec_common.h:258-270) before its
    rounds, its prefix sum and its status read subs[g], g < nsub, and subs[g - 1], g > 0 (:271-395); a frame's states start at
    its sub_base, which the entry checks to be the sum of the earlier frames' counts (csrc/jpeg_dec.hip:203), so no workgroup
    reads another's.  The write kernel, launched behind it on the same stream (jpeg_dec.hip:246-252, the same order in
    csrc/jpeg_dec_mjpeg.hip), reads subs_all[sub_base + g] for g < nsub (jpeg_dec_common.h:404-409).  Every other value that
    forms an address comes from the record or the data, clamped (:207-208).  The coefficients are cleared by hipMemsetAsync
    (jpeg_dec.hip:230, jpeg_dec_mjpeg.hip:246) and are arithmetic input of the IDCT (jpeg_dec_common.h:463-489); the planes are
    written whole by the IDCT kernel and read as samples.  No index is derived from either.  So both byte fills apply."""

    def __init__(self, which):
        self.which = which
        self.name = "jpeg-decode-" + which
        self.entries = ("casync_op_jpegdec_decode",) if which == "baseline" else ("casync_op_mjpegdec_decode",)

    def files(self, seed):
        import jpeg_decode_cases as jd
        import mjpeg_decode_cases as mj
        from calipsync_amd import jpeg
        if self.which == "baseline":
            whole = [jd.case(n)[0] for n in ("noise_48x64_default", "smooth_48x64_default", "noise_48x64_sub0")]
        else:
            whole = [mj.case("c422smooth_48x64_default")[0], mj.case("graynoise_48x64_optimize")[0], jd.case("noise_48x64_default")[0]]
        cuts = ((1, 2), (1, 3), (2, 3)) if seed == 0 else ((1, 3), (1, 4), (1, 2))       # seed 1: shorter everywhere, fewer subsequences
        out = []
        for data, (num, den) in zip(whole, cuts):
            info = jpeg.parse_jpeg(data, self.which)
            assert info.restart_interval == 0, "a file with restart markers would get its status on the host"
            out.append(data[:info.scan_offset + info.scan_length * num // den])
        return out

    def setup(self):
        from calipsync_amd import jpeg
        self.plans = {seed: jpeg.plan_decode(self.files(seed), 32, subset=self.which) for seed in (0, 1)}
        assert all((p.H, p.W) == (48, 64) and not p.rec[:, 9].any() for p in self.plans.values())
        self.needs = {seed: jpeg.workspace_bytes(p, 3, 48, 64) for seed, p in self.plans.items()}
        assert self.needs[1] <= self.needs[0] and self.plans[1].total_sub < self.plans[0].total_sub
        self.inp = {seed: _dev(p.blob.copy()) for seed, p in self.plans.items()}

    def need(self):
        return self.needs[0]

    def run(self, call, ws, seed, fill):
        torch = _t()
        from calipsync_amd import jpeg
        out, status = torch.zeros((3, 48, 64, 3), dtype=torch.uint8, device=DEV), torch.zeros((3,), dtype=torch.int32, device=DEV)
        jpeg.decode_jpeg_op(self.plans[seed], self.inp[seed], ws, out, status, 48, 64)              # (ws.data_ptr() and ws.numel() go to the entry)
        return [("out", out), ("status", status)]


class AudioNormalize(Adapter):
    """casync_op_audio_normalize through ctypes on n = 4097 samples (two moments blocks, the vector path with one sample left
    over): the normalised wave and the float64 {mean, variance} head the contract leaves at the start of the workspace.  The
    workspace holds float64 partial sums only (csrc/audio.hip:171-210)."""
    name = "audio-normalize"
    entries = ("casync_op_audio_normalize",)
    N = 4097

    def setup(self):
        self.inp = {seed: _dev(np.random.default_rng(900 + seed).standard_normal(self.N).astype(np.float32) * np.float32(0.3 + seed)) for seed in (0, 1)}

    def need(self):
        return _lib().casync_op_audio_workspace_bytes(self.N)

    def run(self, call, ws, seed, fill):
        torch = _t()
        out = torch.zeros((self.N,), dtype=torch.float32, device=DEV)
        _ok(_lib().casync_op_audio_normalize(self.inp[seed].data_ptr(), self.N, ws.data_ptr(), out.data_ptr(), _stream()), "casync_op_audio_normalize")
        return [("out", out), ("moments", ws[:16].view(torch.float64))]


def unet_9_then_4():
    """the fp32 U-Net on 4 frames in the arena a 9-frame forward on other input has just used"""
    return UNet("fp32", 4, prior_batch=9)


def adapters() -> dict:
    """{name: factory}: every adapter of the table in DESIGN.md, made fresh for each test"""
    out = {}

    def add(factory):
        out[factory().name] = factory

    for p in ("fp32", "bf16"):
        for args in ((p, 1), (p, 5), (p, 12), (p, 2, "wenet"), (p, 5, "hubert", "windows"), (p, 5, "hubert", "profile")):
            add(functools.partial(UNet, *args))
    for p in ("fp32", "bf16"):
        for batch, samples in ((2, 401), (2, 2000), (1, 720)):
            add(functools.partial(Hubert, p, batch, samples))
    for batch in (1, 3):
        add(functools.partial(Pfld, batch))
    for p in ("fp32", "bf16"):
        add(functools.partial(S3fd, p, 1, 64, 64))
        add(functools.partial(S3fd, p, 3, 77, 93))
    for mode in ("hubert", "wenet"):
        for p in ("fp32", "bf16"):
            for batch in (1, 3):
                add(functools.partial(SyncNet, mode, p, batch))
    for sub in ("4:4:4", "4:2:0"):
        add(functools.partial(JpegEncode, sub))
    for which in ("baseline", "mjpeg"):
        add(functools.partial(JpegDecode, which))
    add(AudioNormalize)
    add(unet_9_then_4)
    return out


def cases():
    """[(adapter name, variant)] in adapter order"""
    return [(name, v) for name, factory in adapters().items() for v in factory().variants]


def _adapter_table() -> dict:
    """{entry: (adapter names)} from the adapters' own `entries`"""
    table: dict = {}
    for name, factory in adapters().items():
        for e in factory().entries:
            table.setdefault(e, []).append(name)
    return {e: tuple(v) for e, v in table.items()}


ADAPTERS = _adapter_table()

EXEMPT: dict = {}      # {entry: reason}: none today
