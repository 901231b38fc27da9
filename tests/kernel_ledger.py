"""Which op-level check runs each compiled kernel instance.

LEDGER maps every kernel of the built library, by the short name tools/kernel_resources.table() and the profile rows use,
to the cases that launch it.  A case is a family function and its parameters: it sets the options it needs, calls one
entry of the C ABI with the launch log on (gpu_util.launched) and returns what it launched together with its error
against a float64 (or bit-exact) reference and the bar that error must meet.  Several kernels may share a case (an entry
that launches more than one kernel); each of their tests then checks that its own kernel is among the launched ones.

Nothing here touches a GPU at import: tests/test_kernel_ledger.py checks on any machine that the ledger names exactly
the built kernels, tests/test_kernel_ledger_gpu.py runs the cases.  The shapes sit on the edges where a kernel goes wrong:
partial tiles, leading dimensions wider than the logical width (written into sentinel-filled buffers, checked untouched),
odd frame counts, stride 2, batch > 1 where a grid axis is the batch."""
from __future__ import annotations

import functools
from typing import Callable, NamedTuple, Tuple


class Case(NamedTuple):
    fn: Callable
    params: Tuple

    def run(self):
        return _cached(self.fn, self.params)

    def __repr__(self):
        return f"{self.fn.__name__}{self.params}"


class Outcome(NamedTuple):
    launched: frozenset
    err: float        # max error against the reference (inf where a sentinel changed or a value is not finite)
    bar: float
    what: str


@functools.lru_cache(maxsize=None)
def _cached(fn, params):
    import torch
    out = fn(*params)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ helpers (import torch lazily: CPU collection)
def _t():
    import torch
    return torch


def _dev():
    return _t().device("cuda:0")


def _lib():
    from calipsync_amd import _lib as L
    return L.load()


def _ok(status, what):
    from calipsync_amd import _lib as L
    L.check(status, what)


def _s():
    return _t().cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _gen(*key):   # a seed that repeats across processes (hash() of a str does not)
    import zlib
    return _t().Generator().manual_seed(zlib.crc32(repr(key).encode()))


class _Run:
    """options + op dtype + launch log around one case's calls"""

    def __init__(self, dtype=0, **opts):
        self.dtype, self.opts = dtype, opts

    def __enter__(self):
        import contextlib
        import gpu_util
        self._stack = contextlib.ExitStack()
        self._stack.__enter__()
        self._stack.enter_context(gpu_util.options(**self.opts))
        _lib().casync_op_set_dtype(self.dtype)
        self._stack.callback(_lib().casync_op_set_dtype, 0)
        self.names = self._stack.enter_context(gpu_util.launched())
        return self

    def __exit__(self, *exc):
        return self._stack.__exit__(*exc)


def _rel(got, ref):
    torch = _t()
    got, ref = got.double(), ref.double().to(got.device)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float((got - ref).abs().max()) / max(1e-6, float(ref.abs().max()))


def _abs(got, ref):
    torch = _t()
    got, ref = got.double(), ref.double().to(got.device)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float((got - ref).abs().max())


def _bf16_rel1(got, ref):
    """|got - ref| / (|ref| + 1): the bf16 GEMM bar (tests/test_ops_gpu.py test_pw_gemm_bf16)"""
    torch = _t()
    got, ref = got.double(), ref.double().to(got.device)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / (ref.abs() + 1.0)).max())


def _max_mean(got, ref, bar_max, bar_mean):
    """two bars in one number: max(max |d|, mean |d| * bar_max / bar_mean) / max|ref|, held to bar_max"""
    torch = _t()
    got, ref = got.double(), ref.double().to(got.device)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    d, top = (got - ref).abs(), max(1e-6, float(ref.abs().max()))
    return max(float(d.max()), float(d.mean()) * bar_max / bar_mean) / top


def _sentinel(buf, lo, hi, value):
    """inf when anything outside columns [lo, hi) of the last axis is not `value`"""
    torch = _t()
    outside = torch.cat([buf[..., :lo].reshape(-1), buf[..., hi:].reshape(-1)]).float()
    return 0.0 if bool((outside == value).all()) else float("inf")


def _lrelu(x):
    return _t().nn.functional.leaky_relu(x, 0.01)


def _done(run, err, bar, what):
    return Outcome(frozenset(run.names), float(err), float(bar), what)


# ------------------------------------------------------------------ GEMM (casync_op_pw_gemm)
def gemm(dtype, m, n, k, cfg, glds=2, ring128=0):
    """C = aff(lrelu(A W^T + b + s * pre) + post) on column slices of wider buffers (lda, ldc, ld_pre, ld_post > widths),
    C written into a sentinel-filled buffer; `cfg` forces the tile (gemm_cfg), `glds` 0 takes the register-staged kernel.
    fp32: rel 2e-6; bf16 (operands and residuals bf16): |d| / (|ref| + 1) < 2^-8 on the same rounded operands."""
    torch = _t()
    F = torch.nn.functional
    g = _gen("gemm", dtype, m, n, k, cfg)
    bf = dtype == 1
    dt = torch.bfloat16 if bf else torch.float32
    e16 = 8 if bf else 4
    lda, ldc, ldr = k + 4 * e16, n + 2 * e16, n + 6 * e16
    A = torch.randn(m, lda, generator=g).to(dt)
    W = (torch.randn(n, k, generator=g) / k ** 0.5).to(dt)
    bias, ps, s2, t2 = (torch.randn(n, generator=g) for _ in range(4))
    pre, post = (torch.randn(m, ldr, generator=g).to(dt) for _ in range(2))
    d = _dev()
    Ad, Wd, bd, psd, s2d, t2d, pred, postd = (x.to(d) for x in (A, W, bias, ps, s2, t2, pre, post))
    a = Ad[:, 2 * e16:2 * e16 + k]
    v = a.double() @ Wd.double().T + bd.double() + psd.double() * pred[:, :n].double()
    v = _lrelu(v) + postd[:, :n].double()
    ref = _lrelu(v * s2d.double() + t2d.double())
    es = 2 if bf else 4
    c = torch.full((m, ldc), -7.0, device=d, dtype=dt)
    with _Run(dtype, gemm_cfg=cfg, gemm_glds=glds, gemm_ring128=ring128) as r:
        _ok(_lib().casync_op_pw_gemm(Ad.data_ptr() + 2 * e16 * es, lda, _p(Wd), _p(bd), c.data_ptr() + e16 * es, ldc, m, n, k, 1,
                                     _p(pred), ldr, _p(psd), _p(postd), ldr, _p(s2d), _p(t2d), _s()), "pw_gemm")
    err = (_bf16_rel1 if bf else _rel)(c[:, e16:e16 + n], ref)
    err = max(err, _sentinel(c, e16, e16 + n, -7.0))
    return _done(r, err, 2 ** -8 if bf else 2e-6, f"pw_gemm dt={dtype} {m}x{n}x{k} cfg={cfg} glds={glds} ring128={ring128}")


def gemm_ups(frames, hw, c_lo, cexp):
    """casync_op_pw_gemm_ups: lrelu(W1b . skip + b + up2x(G)) against the reference order (upsample, cat, conv) in float64;
    skip and G read from column slices of wider buffers, C into a sentinel-filled one."""
    torch = _t()
    F = torch.nn.functional
    g = _gen("gemm_ups", frames, hw, c_lo, cexp)
    d = _dev()
    lo = torch.randn(frames, c_lo, hw // 2, hw // 2, generator=g).to(d)
    skip = torch.randn(frames, c_lo, hw, hw, generator=g).to(d)
    w1 = (torch.randn(cexp, 2 * c_lo, generator=g) / (2 * c_lo) ** 0.5).to(d)
    b1 = (torch.randn(cexp, generator=g) * 0.3).to(d)
    x = torch.cat([F.interpolate(lo.double(), scale_factor=2, mode="bilinear", align_corners=True), skip.double()], 1)
    ref = _lrelu(torch.einsum("oc,bchw->bhwo", w1.double(), x) + b1.double()).reshape(-1, cexp)
    w1a, w1b = w1[:, :c_lo].contiguous(), w1[:, c_lo:].contiguous()
    ld_g, ld_s, ldc = cexp + 32, c_lo + 16, cexp + 8
    G = torch.full((frames * (hw // 2) ** 2, ld_g), 55.0, device=d)
    Gv = lo.double().permute(0, 2, 3, 1).reshape(-1, c_lo) @ w1a.double().T
    G[:, 16:16 + cexp] = Gv.float()
    S = torch.full((frames * hw * hw, ld_s), 3.0, device=d)
    S[:, 16:] = skip.permute(0, 2, 3, 1).reshape(-1, c_lo)
    c = torch.full((frames * hw * hw, ldc), -7.0, device=d)
    with _Run(0) as r:
        _ok(_lib().casync_op_pw_gemm_ups(S.data_ptr() + 64, ld_s, _p(w1b), _p(b1), c.data_ptr() + 16, ldc, c.shape[0], cexp, c_lo, 1,
                                         G.data_ptr() + 64, ld_g, hw, hw, _s()), "pw_gemm_ups")
    err = max(_rel(c[:, 4:4 + cexp], ref), _sentinel(c, 4, 4 + cexp, -7.0))
    return _done(r, err, 3e-6, f"pw_gemm_ups {frames}x{hw}x{hw} {c_lo}->{cexp}")


def conv3x3(dtype, b, h, w, cin, cout, sh, sw, pad, cfg):
    """casync_op_conv3x3_ex (implicit GEMM, taps gathered by the loads) vs F.conv2d in float64 (+ ReLU); bf16 on the same
    rounded operands at the bf16 GEMM bar."""
    torch = _t()
    F = torch.nn.functional
    g = _gen("conv3x3", dtype, b, h, w, cin, cout, sh, sw, pad)
    bf = dtype == 1
    dt = torch.bfloat16 if bf else torch.float32
    d = _dev()
    x = torch.randn(b, cin, h, w, generator=g).to(dt).to(d)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)).to(dt).to(d)
    bias = torch.randn(cout, generator=g).to(d)
    ref = torch.relu(F.conv2d(x.double().cpu(), wt.double().cpu(), bias.double().cpu(), (sh, sw), pad)).permute(0, 2, 3, 1)
    xd = x.permute(0, 2, 3, 1).contiguous()
    wp = wt.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous()
    out = torch.full(tuple(ref.shape), float("nan"), device=d, dtype=dt)
    with _Run(dtype, gemm_cfg=cfg) as r:
        _ok(_lib().casync_op_conv3x3_ex(_p(xd), _p(wp), _p(bias), _p(out), b, h, w, cin, cout, sh, sw, pad, 2, _s()), "conv3x3")
    err = (_bf16_rel1 if bf else _rel)(out, ref)
    return _done(r, err, 2 ** -8 if bf else 3e-6, f"conv3x3 dt={dtype} {b}x{h}x{w}x{cin}->{cout} s=({sh},{sw}) pad={pad}")


# ------------------------------------------------------------------ HuBERT
def rows_gemm(m, n, k, lda, act, res, ldc_pad=0):
    """casync_op_rows_gemm at one of the shapes the HuBERT forward launches.  lda < k: the A rows overlap (a channels-last
    conv, stride lda / 512); res: post-residual added IN PLACE (post_res == C, as the o-proj and FF2 GEMMs run);
    ldc_pad > 0: C is a slice of a wider, sentinel-filled buffer.  1e-4 abs against float64."""
    torch = _t()
    F = torch.nn.functional
    g = _gen("rows", m, n, k, lda, act, res)
    d = _dev()
    rows_a = (m - 1) * lda + k
    flat = torch.randn(rows_a, generator=g).to(d)
    W = (torch.randn(n, k, generator=g) / k ** 0.5).to(d)
    b = torch.randn(n, generator=g).to(d)
    a = flat.as_strided((m, k), (lda, 1))
    ref = a.double() @ W.double().T + b.double()
    ref = F.gelu(ref) if act == 3 else ref
    ldc = n + ldc_pad
    c = torch.full((m, ldc), -7.0, device=d)
    if res:
        r0 = torch.randn(m, n, generator=g).to(d)
        c[:, :n] = r0
        ref = ref + r0.double()
    with _Run(0) as r:
        _ok(_lib().casync_op_rows_gemm(_p(flat), lda, _p(W), _p(b), _p(c), ldc, m, n, k, act, _p(c) if res else 0, ldc if res else 0,
                                       _s()), "rows_gemm")
    err = _abs(c[:, :n], ref)
    if ldc_pad:
        err = max(err, _sentinel(c, 0, n, -7.0))
    return _done(r, err, 1e-4, f"rows_gemm {m}x{n}x{k} lda={lda} act={act} res={res} ldc={ldc}")


def hb_layernorm(cols, gelu, rows, mode):
    """casync_op_hubert_layernorm: mode 'strided' reads / writes slices of wider buffers (ldi, ldo > cols, sentinels kept),
    'inplace' runs in == out as the feature encoder does.  1e-4 abs against float64."""
    torch = _t()
    F = torch.nn.functional
    g = _gen("ln", cols, gelu, rows, mode)
    d = _dev()
    x = (torch.randn(rows, cols, generator=g) * 3 + 1).to(d)
    gm, be = torch.randn(cols, generator=g).to(d), torch.randn(cols, generator=g).to(d)
    ref = F.layer_norm(x.double(), (cols,), gm.double(), be.double(), 1e-5)
    ref = F.gelu(ref) if gelu else ref
    lib = _lib()
    if mode == "inplace":
        buf = x.clone()
        with _Run(0) as r:
            _ok(lib.casync_op_hubert_layernorm(_p(buf), cols, _p(buf), cols, rows, cols, _p(gm), _p(be), 1e-5, gelu, _s()), "layernorm")
        err = _abs(buf, ref)
    else:
        ldi, ldo = cols + 32, cols + 64
        inb = torch.full((rows, ldi), 9.0, device=d)
        inb[:, 32:] = x
        out = torch.full((rows, ldo), -7.0, device=d)
        with _Run(0) as r:
            _ok(lib.casync_op_hubert_layernorm(inb.data_ptr() + 128, ldi, out.data_ptr() + 64, ldo, rows, cols, _p(gm), _p(be), 1e-5,
                                               gelu, _s()), "layernorm")
        err = max(_abs(out[:, 16:16 + cols], ref), _sentinel(out, 16, 16 + cols, -7.0))
    return _done(r, err, 1e-4, f"hubert layernorm cols={cols} gelu={gelu} rows={rows} {mode}")


def hb_conv0(B, S):
    """casync_op_hubert_conv0 (conv k=10 s=5 + LayerNorm + GELU) vs float64: B waveforms of S samples."""
    torch = _t()
    F = torch.nn.functional
    g = _gen("conv0", B, S)
    d = _dev()
    x = torch.randn(B, S, generator=g).to(d)
    W = (torch.randn(512, 10, generator=g) / 3).to(d)
    b, gm, be = (torch.randn(512, generator=g).to(d) for _ in range(3))
    T0 = (S - 10) // 5 + 1
    y = x.double().unfold(1, 10, 5) @ W.double().T + b.double()
    ref = F.gelu(F.layer_norm(y, (512,), gm.double(), be.double(), 1e-5)).reshape(B * T0, 512)
    out = torch.full((B * T0, 512), float("nan"), device=d)
    with _Run(0) as r:
        _ok(_lib().casync_op_hubert_conv0(_p(x), B, S, _p(W), _p(b), _p(gm), _p(be), _p(out), _s()), "conv0")
    return _done(r, _abs(out, ref), 1e-4, f"hubert conv0 B={B} S={S}")


def hb_posconv(B, T):
    """casync_op_hubert_posconv: x + GELU(grouped conv1d(x, k=128, pad 64, 16 groups)[..., :T] + b) vs float64."""
    torch = _t()
    F = torch.nn.functional
    g = _gen("posconv", B, T)
    d = _dev()
    x = torch.randn(B, T, 1024, generator=g).to(d)
    W = (torch.randn(1024, 64, 128, generator=g) / 90.0).to(d)
    b = (torch.randn(1024, generator=g) * 0.1).to(d)
    wp = W.reshape(16, 64, 64, 128).permute(0, 3, 1, 2).contiguous()
    xp = F.pad(x.double().transpose(1, 2), (64, 64)).reshape(B, 16, 64, T + 128)
    Wg = W.double().reshape(16, 64, 64, 128)
    pc = torch.zeros(B, 16, 64, T, dtype=torch.float64, device=d)
    for tap in range(128):
        pc += torch.einsum("goc,bgct->bgot", Wg[..., tap], xp[..., tap:tap + T])
    pc = pc.reshape(B, 1024, T) + b.double()[:, None]
    ref = (x.double() + F.gelu(pc).transpose(1, 2)).reshape(B * T, 1024)
    out = torch.full((B * T, 1024), float("nan"), device=d)
    with _Run(0) as r:
        _ok(_lib().casync_op_hubert_posconv(_p(x), _p(wp), _p(b), _p(out), B, T, _s()), "posconv")
    return _done(r, _abs(out, ref), 1e-4, f"hubert posconv B={B} T={T}")


def hb_attention(B, T, peaked):
    """casync_op_hubert_attention from the fused q|k|v rows vs float64.  peaked: every query's largest score is key T-1,
    the only key of the last (partial) key tile -- the online softmax rescales everything it has summed when it gets there."""
    torch = _t()
    g = _gen("att", B, T, peaked)
    d = _dev()
    qkv = torch.randn(B * T, 3072, generator=g)
    qkv[:, :1024] *= 0.5
    if peaked:
        u = torch.randn(B, 16, 64, generator=g) * 0.35
        q = qkv[:, :1024].reshape(B, T, 16, 64) * 0.3 + u[:, None]
        k = qkv[:, 1024:2048].reshape(B, T, 16, 64) * 0.3
        k[:, T - 1] = 1.6 * u
        qkv[:, :1024] = q.reshape(B * T, 1024)
        qkv[:, 1024:2048] = k.reshape(B * T, 1024)
    qd = qkv.to(d)
    q, k, v = (z.reshape(B, T, 16, 64).transpose(1, 2) for z in qd.double().split(1024, dim=1))
    s = q @ k.transpose(-1, -2)
    if peaked:
        assert bool((s.argmax(-1) == T - 1).all())
    ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * T, 1024)
    out = torch.full((B * T, 1024), float("nan"), device=d)
    with _Run(0) as r:
        _ok(_lib().casync_op_hubert_attention(_p(qd), _p(out), B, T, _s()), "attention")
    return _done(r, _abs(out, ref), 1e-4, f"hubert attention B={B} T={T} peaked={peaked}")


# ------------------------------------------------------------------ depthwise, upsample, layout
def dw3x3(dtype, b, h, w, c, stride, dw_lds=1):
    """casync_op_dw3x3 vs F.conv2d (groups = C) + LeakyReLU in float64; bf16 input rounded, bar 2^-8 (output rounding)."""
    torch = _t()
    F = torch.nn.functional
    g = _gen("dw", dtype, b, h, w, c, stride)
    bf = dtype == 1
    dt = torch.bfloat16 if bf else torch.float32
    d = _dev()
    x = torch.randn(b, c, h, w, generator=g).to(dt).to(d)
    wt = (torch.randn(c, 1, 3, 3, generator=g) / 3).to(d)
    bias = torch.randn(c, generator=g).to(d)
    ref = _lrelu(F.conv2d(x.double().cpu(), wt.double().cpu(), bias.double().cpu(), stride, 1, 1, c)).permute(0, 2, 3, 1)
    wp = wt.reshape(c, 9).T.contiguous()
    xd = x.permute(0, 2, 3, 1).contiguous()
    out = torch.full(tuple(ref.shape), float("nan"), device=d, dtype=dt)
    with _Run(dtype, dw_lds=dw_lds) as r:
        _ok(_lib().casync_op_dw3x3(_p(xd), _p(wp), _p(bias), _p(out), b, h, w, c, stride, _s()), "dw3x3")
    return _done(r, _rel(out, ref), 2 ** -8 if bf else 2e-6, f"dw3x3 dt={dtype} {b}x{h}x{w}x{c} s={stride} lds={dw_lds}")


def dw3x3_ups(frames, hw, c, ldg):
    """casync_op_dw3x3_ups: depthwise 3x3 over lrelu(pre + up2x(g)), g a column slice (ldg > c, NaN beyond), vs float64."""
    torch = _t()
    F = torch.nn.functional
    gen = _gen("dwups", frames, hw, c, ldg)
    d = _dev()
    pre = torch.randn(frames, c, hw, hw, generator=gen).to(d)
    gl = torch.randn(frames, c, hw // 2, hw // 2, generator=gen).to(d)
    wt = (torch.randn(c, 1, 3, 3, generator=gen) / 3).to(d)
    bias = torch.randn(c, generator=gen).to(d)
    e = _lrelu(pre.double() + F.interpolate(gl.double(), scale_factor=2, mode="bilinear", align_corners=True))
    ref = _lrelu(F.conv2d(e.cpu(), wt.double().cpu(), bias.double().cpu(), 1, 1, 1, c)).permute(0, 2, 3, 1)
    gd = torch.full((frames, hw // 2, hw // 2, ldg), float("nan"), device=d)
    gd[..., :c] = gl.permute(0, 2, 3, 1)
    wp = wt.reshape(c, 9).T.contiguous()
    pd = pre.permute(0, 2, 3, 1).contiguous()
    out = torch.full((frames, hw, hw, c), float("nan"), device=d)
    with _Run(0) as r:
        _ok(_lib().casync_op_dw3x3_ups(_p(pd), _p(gd), ldg, _p(wp), _p(bias), _p(out), frames, hw, hw, c, _s()), "dw3x3_ups")
    return _done(r, _rel(out, ref), 3e-6, f"dw3x3_ups {frames}x{hw}x{hw}x{c} ldg={ldg}")


def upsample(dtype, b, h, w, c):
    """casync_op_upsample2x into the first c columns of 2c-wide rows (the other half stays) vs float64 bilinear
    (align_corners=True): 5e-5 abs as tests/test_ops_gpu.py; bf16 input rounded, output within bf16 rounding (2^-8 rel)."""
    torch = _t()
    F = torch.nn.functional
    g = _gen("ups", dtype, b, h, w, c)
    bf = dtype == 1
    dt = torch.bfloat16 if bf else torch.float32
    d = _dev()
    x = torch.randn(b, c, h, w, generator=g).to(dt).to(d)
    ref = F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    out = torch.full((b, 2 * h, 2 * w, 2 * c), 5.0, device=d, dtype=dt)
    xd = x.permute(0, 2, 3, 1).contiguous()
    with _Run(dtype) as r:
        _ok(_lib().casync_op_upsample2x(_p(xd), _p(out), 2 * c, b, h, w, c, _s()), "upsample2x")
    err = _rel(out[..., :c], ref) if bf else _abs(out[..., :c], ref)
    err = max(err, _sentinel(out, 0, c, 5.0))
    return _done(r, err, 2 ** -8 if bf else 5e-5, f"upsample2x dt={dtype} {b}x{h}x{w}x{c}")


def nchw_to_nhwc(dtype, b, c, hw):
    """casync_op_nchw_to_nhwc: bit for bit (bf16: torch's round-to-nearest-even)."""
    torch = _t()
    g = _gen("nchw", dtype, b, c, hw)
    d = _dev()
    x = torch.randn(b, c, hw, generator=g).to(d)
    dt = torch.bfloat16 if dtype == 1 else torch.float32
    out = torch.full((b, hw, c), 3.0, device=d, dtype=dt)
    with _Run(dtype) as r:
        _ok(_lib().casync_op_nchw_to_nhwc(_p(x), _p(out), b, c, hw, _s()), "nchw_to_nhwc")
    ok = torch.equal(out, x.transpose(1, 2).to(dt))
    return _done(r, 0.0 if ok else float("inf"), 0.0, f"nchw_to_nhwc dt={dtype} {b}x{c}x{hw}")


def audio_windows(dtype, nhwc):
    """casync_op_audio_windows vs frame_loop.audio_windows_host (the reference's window rule), bit for bit: indices before
    the start, past the end and inside; nhwc = 1 is the engine's [B,1024,32] image in the op dtype."""
    torch = _t()
    import frame_data
    from calipsync_amd import frame_loop
    feats = frame_data.golden_features(41, seed=5)
    idx = [-9, -3, 0, 1, 7, 8, 20, 33, 38, 40, 41, 50, 12]
    want = torch.from_numpy(frame_loop.audio_windows_host(feats, idx))
    d = _dev()
    fd = torch.from_numpy(feats).to(d)
    idd = torch.tensor(idx, dtype=torch.int32, device=d)
    B = len(idx)
    if nhwc:
        dt = torch.bfloat16 if dtype == 1 else torch.float32
        out = torch.full((B, 1024, 32), 3.0, device=d, dtype=dt)
        want = want.reshape(B, 32, 1024).transpose(1, 2).to(dt)
    else:
        out = torch.full((B, 32, 32, 32), 3.0, device=d)
    with _Run(dtype) as r:
        _ok(_lib().casync_op_audio_windows(_p(fd), 41, _p(idd), _p(out), B, nhwc, _s()), "audio_windows")
    ok = torch.equal(out.cpu(), want)
    return _done(r, 0.0 if ok else float("inf"), 0.0, f"audio_windows dt={dtype} nhwc={nhwc}")


def pred_to_u8(b):
    """casync_op_pred_to_u8: uint8(pred * 255) truncated, NCHW -> HWC, bit for bit."""
    torch = _t()
    g = _gen("pred", b)
    d = _dev()
    pred = torch.rand(b, 3, 160, 160, generator=g)
    pred[0, 0, 0, :4] = torch.tensor([0.0, 1.0, 0.5, 254.5 / 255])
    pd = pred.to(d)
    out = torch.full((b, 160, 160, 3), 7, dtype=torch.uint8, device=d)
    with _Run(0) as r:
        _ok(_lib().casync_op_pred_to_u8(_p(pd), _p(out), b, _s()), "pred_to_u8")
    want = (pred * 255.0).to(torch.uint8).permute(0, 2, 3, 1)
    return _done(r, 0.0 if torch.equal(out.cpu(), want) else float("inf"), 0.0, f"pred_to_u8 B={b}")


# ------------------------------------------------------------------ fused blocks (recipe weights, oracle modules in float64)
@functools.lru_cache(maxsize=None)
def _recipe():
    from calipsync_amd import pack, recipe
    from oracle import unet_oracle
    sd_np = recipe.make_state_dict()
    return unet_oracle.to_torch(sd_np, _t().float64), pack.fold(sd_np)


def _folded(f, prefix, key, dt=None):
    import numpy as np
    t = _t().from_numpy(f[f"{prefix}.{key}"].astype(np.float32)).contiguous().to(_dev())
    return t if dt is None else t.to(dt)


IR_PREFIX = {(32, 32, 1): ("up4.conv.double_conv.1", True), (64, 32, 1): ("up4.conv.double_conv.0", False),
             (128, 32, 1): ("up3.conv.double_conv.0", False), (64, 64, 1): ("down1.maxpool_conv.0.double_conv.1", True),
             (32, 64, 2): ("down1.maxpool_conv.0.double_conv.0", False), (32, 64, 1): ("audio_model.conv1", False),
             (64, 128, 1): ("audio_model.conv2", False), (64, 128, 2): ("down2.maxpool_conv.0.double_conv.0", False)}


def ir_fused(dtype, cin, cout, stride, b, h, w, dwm=1):
    """casync_op_ir_fused (whole inverted residual) vs the oracle's module in float64 on the recipe weights, reading and
    writing channel slices of wider buffers.  fp32: rel 3e-6; bf16 (input rounded; `dwm` = ir_dw_mfma): rel 2e-2 as
    tests/test_ops_gpu.py test_ir_fused_block_bf16."""
    torch = _t()
    from oracle import unet_oracle
    sd, f = _recipe()
    prefix, res = IR_PREFIX[(cin, cout, stride)]
    bf = dtype == 1
    dt = torch.bfloat16 if bf else torch.float32
    es = 2 if bf else 4
    g = _gen("ir", dtype, cin, cout, stride, b, h, w)
    x = torch.randn(b, cin, h, w, generator=g)
    if bf:
        x = x.bfloat16().float()
    ref = unet_oracle.inverted_residual(sd, prefix, x.double(), stride, res).permute(0, 2, 3, 1)
    ho, wo = ref.shape[1], ref.shape[2]
    ld_in, ld_out = cin + 32, cout + 16
    xin = torch.full((b, h, w, ld_in), 3.0)
    xin[..., 32:] = x.permute(0, 2, 3, 1)
    xin = xin.to(dt).to(_dev())
    out = torch.full((b, ho, wo, ld_out), -5.0, device=_dev(), dtype=dt)
    wdt = torch.bfloat16 if bf else None
    w1, b1, wd, bd, w2, b2 = (_folded(f, prefix, "pw1.w", wdt), _folded(f, prefix, "pw1.b"), _folded(f, prefix, "dw.w"),
                              _folded(f, prefix, "dw.b"), _folded(f, prefix, "pw2.w", wdt), _folded(f, prefix, "pw2.b"))
    with _Run(dtype, ir_dw_mfma=dwm) as r:
        _ok(_lib().casync_op_ir_fused(xin.data_ptr() + 32 * es, ld_in, _p(w1), _p(b1), _p(wd), _p(bd), _p(w2), _p(b2),
                                      out.data_ptr() + 16 * es, ld_out, b, h, w, cin, cout, stride, int(res), _s()), "ir_fused")
    err = _max_mean(out[..., 16:], ref, 2e-2, 1.5e-3) if bf else _rel(out[..., 16:], ref)
    err = max(err, _sentinel(out, 16, 16 + cout, -5.0))
    return _done(r, err, 2e-2 if bf else 3e-6, f"ir_fused dt={dtype} {cin}->{cout} s={stride} {b}x{h}x{w} dwm={dwm}")


def ir_fused_up(dtype, cin, b, h, w, mode, dwm=1):
    """The fused Up block (interpolate + cat + first inverted residual) vs the oracle's module in float64 on the recipe
    weights.  mode 'load': casync_op_ir_fused_up (upsample while loading); 'commuted': casync_op_ir_fused_upg over
    G = W1a . lo (fp32 only, G a column slice of a wider buffer).  fp32: rel 5e-6; bf16: rel 2e-2."""
    torch = _t()
    F = torch.nn.functional
    from oracle import unet_oracle
    sd, f = _recipe()
    prefix = {64: "up4.conv.double_conv.0", 128: "up3.conv.double_conv.0"}[cin]
    bf = dtype == 1
    dt = torch.bfloat16 if bf else torch.float32
    es = 2 if bf else 4
    g = _gen("irup", dtype, cin, b, h, w, mode)
    c_lo, cexp = cin // 2, 2 * cin
    lo = torch.randn(b, c_lo, h // 2, w // 2, generator=g)
    skip = torch.randn(b, cin - c_lo, h, w, generator=g)
    if bf:
        lo, skip = lo.bfloat16().float(), skip.bfloat16().float()
    up = F.interpolate(lo.double(), scale_factor=2, mode="bilinear", align_corners=True)
    ref = unet_oracle.inverted_residual(sd, prefix, torch.cat([up, skip.double()], 1), 1, False).permute(0, 2, 3, 1)
    cat = torch.full((b, h, w, cin), 77.0)
    cat[..., c_lo:] = skip.permute(0, 2, 3, 1)
    d = _dev()
    cat = cat.to(dt).to(d)
    lod = lo.permute(0, 2, 3, 1).contiguous().to(dt).to(d)
    wdt = torch.bfloat16 if bf else None
    w1, b1, wd, bd, w2, b2 = (_folded(f, prefix, "pw1.w", wdt), _folded(f, prefix, "pw1.b"), _folded(f, prefix, "dw.w"),
                              _folded(f, prefix, "dw.b"), _folded(f, prefix, "pw2.w", wdt), _folded(f, prefix, "pw2.b"))
    out = torch.full((b, h, w, 48), -5.0, device=d, dtype=dt)
    lib = _lib()
    if mode == "load":
        with _Run(dtype, ir_dw_mfma=dwm) as r:
            _ok(lib.casync_op_ir_fused_up(_p(lod), c_lo, c_lo, _p(cat), cin, _p(w1), _p(b1), _p(wd), _p(bd), _p(w2), _p(b2),
                                          out.data_ptr() + 16 * es, 48, b, h, w, cin, 32, _s()), "ir_fused_up")
    else:
        w1a, w1b = _folded(f, prefix, "pw1a.w"), _folded(f, prefix, "pw1b.w")
        ld_g = cexp + 16
        G = torch.full((b * (h // 2) * (w // 2), ld_g), 55.0, device=d)
        G[:, :cexp] = (lod.double().reshape(-1, c_lo) @ w1a.double().T).float()
        with _Run(0) as r:
            _ok(lib.casync_op_ir_fused_upg(_p(G), ld_g, cat.data_ptr() + c_lo * 4, cin, _p(w1b), _p(b1), _p(wd), _p(bd), _p(w2),
                                           _p(b2), out.data_ptr() + 64, 48, b, h, w, cin, 32, _s()), "ir_fused_upg")
    err = max(_rel(out[..., 16:], ref), _sentinel(out, 16, 48, -5.0))
    return _done(r, err, 2e-2 if bf else 5e-6, f"ir_fused_up dt={dtype} cin={cin} {b}x{h}x{w} {mode} dwm={dwm}")


def pw_dw(dtype, hw, stride, cin, cexp, frames, bn=128, rect_w=0):
    """Expand 1x1 + LeakyReLU + depthwise 3x3 + LeakyReLU in one kernel vs float64: casync_op_pw_dw on square frames,
    casync_op_pw_dw_rect on hw x rect_w frames; operands are column slices of wider buffers, D is written into a
    sentinel-filled one.  fp32: rel 3e-6.  bf16 (operands rounded, E rounded where the kernel rounds it): max 2^-7 and
    mean 2^-11 of max|ref| as tests/test_ops_gpu.py test_pw_dw_fused_bf16; `bn` = fuse_dw_bf16_bn."""
    torch = _t()
    F = torch.nn.functional
    bf = dtype == 1
    dt = torch.bfloat16 if bf else torch.float32
    es = 2 if bf else 4
    h, w = hw, (rect_w or hw)
    g = _gen("pwdw", dtype, hw, stride, cin, cexp, frames, rect_w)
    d = _dev()
    x = torch.randn(frames, cin, h, w, generator=g).to(dt).to(d)
    w1 = (torch.randn(cexp, cin, generator=g) / cin ** 0.5).to(dt).to(d)
    b1 = (torch.randn(cexp, generator=g) * 0.3).to(d)
    wd = (torch.randn(cexp, 1, 3, 3, generator=g) / 3).to(d)
    bd = (torch.randn(cexp, generator=g) * 0.3).to(d)
    e = _lrelu(torch.einsum("oc,bchw->bohw", w1.double(), x.double()) + b1.double()[:, None, None])
    if bf:
        e = e.float().bfloat16().double()
    ref = _lrelu(F.conv2d(e.cpu(), wd.double().cpu(), bd.double().cpu(), stride, 1, 1, cexp)).permute(0, 2, 3, 1)
    ho, wo = ref.shape[1], ref.shape[2]
    lda, ldd = cin + 32, cexp + 16
    xin = torch.full((frames, h, w, lda), 5.0, device=d, dtype=dt)
    xin[..., 32:] = x.permute(0, 2, 3, 1)
    out = torch.full((frames, ho, wo, ldd), -7.0, device=d, dtype=dt)
    wdp = wd.reshape(cexp, 9).T.contiguous()
    lib = _lib()
    with _Run(dtype, fuse_dw_bf16_bn=bn) as r:
        if rect_w:
            _ok(lib.casync_op_pw_dw_rect(xin.data_ptr() + 32 * es, lda, _p(w1), _p(b1), _p(wdp), _p(bd), out.data_ptr() + 16 * es,
                                         ldd, frames, h, w, cin, cexp, _s()), "pw_dw_rect")
        else:
            _ok(lib.casync_op_pw_dw(xin.data_ptr() + 32 * es, lda, _p(w1), _p(b1), _p(wdp), _p(bd), out.data_ptr() + 16 * es, ldd,
                                    frames, hw, stride, cin, cexp, 0, 0, _s()), "pw_dw")
    got = out[..., 16:]
    err = _max_mean(got, ref, 2 ** -7, 2 ** -11) if bf else _rel(got, ref)
    err = max(err, _sentinel(out, 16, 16 + cexp, -7.0))
    shape = f"{h}x{w}" if rect_w else f"{hw}x{hw}"
    return _done(r, err, 2 ** -7 if bf else 3e-6, f"pw_dw{'_rect' if rect_w else ''} dt={dtype} {frames}x{shape} s={stride} "
                                                   f"{cin}->{cexp} bn={bn}")


# ------------------------------------------------------------------ attention, inc, outc
def cross_attention(dtype, b, att_bf16=1):
    """casync_op_cross_attention (100 face x 100 audio positions per frame): Q / K / V / res column slices of wider rows,
    out into a sentinel-filled buffer, vs float64.  fp32: rel 3e-6; bf16 (operands rounded): max 2^-7 of max|ref|."""
    torch = _t()
    g = _gen("xatt", dtype, b)
    bf = dtype == 1
    dt = torch.bfloat16 if bf else torch.float32
    es = 2 if bf else 4
    d = _dev()
    p1q = (torch.randn(b, 100, 576, generator=g) * 0.5).to(dt).to(d)
    kv = (torch.randn(b, 100, 2304, generator=g) * 0.5).to(dt).to(d)
    gamma = torch.tensor([-0.75], device=d)
    q, res = p1q[:, :, 512:], p1q[:, :, :512]
    k, v = kv[:, :, 1152:1216], kv[:, :, 1216:1728]
    att = torch.softmax(q.double() @ k.double().transpose(1, 2), -1)
    ref = gamma.double() * (att @ v.double()) + res.double()
    out = torch.full((b, 100, 520), 3.0, device=d, dtype=dt)
    with _Run(dtype, att_bf16=att_bf16) as r:
        _ok(_lib().casync_op_cross_attention(p1q.data_ptr() + 512 * es, 576, kv.data_ptr() + 1152 * es, 2304, kv.data_ptr() + 1216 * es,
                                             2304, _p(p1q), 576, _p(gamma), _p(out), 520, b, _s()), "cross_attention")
    err = max(_rel(out[..., :512], ref), _sentinel(out, 0, 512, 3.0))
    return _done(r, err, 2 ** -7 if bf else 3e-6, f"cross_attention dt={dtype} B={b} att_bf16={att_bf16}")


def inc(dtype, b, inc_mfma=0):
    """casync_op_inc (the `inc` inverted residual from the NCHW crop) into the upper half of 64-wide rows vs the oracle's
    module in float64: fp32 1e-5 abs as tests/test_ops_gpu.py; bf16 rel 6e-3 (matrix pipe) / 4e-3 (VALU)."""
    torch = _t()
    import numpy as np
    from calipsync_amd import recipe
    from oracle import unet_oracle
    sd, f = _recipe()
    x, _ = recipe.make_inputs(b)
    xt = torch.from_numpy(x)
    ref = unet_oracle.inverted_residual(sd, "inc.inconv.0", xt.double(), 1, False).permute(0, 2, 3, 1)
    d = _dev()
    packed = torch.from_numpy(f["inc.inconv.0.fused"].astype(np.float32)).to(d)
    bf = dtype == 1
    dt = torch.bfloat16 if bf else torch.float32
    es = 2 if bf else 4
    out = torch.full((b, 160, 160, 64), 9.0, device=d, dtype=dt)
    xd = xt.to(d)
    with _Run(dtype, inc_mfma=inc_mfma) as r:
        _ok(_lib().casync_op_inc(_p(xd), _p(packed), out.data_ptr() + 32 * es, 64, b, _s()), "inc")
    err = max((_rel if bf else _abs)(out[..., 32:], ref), _sentinel(out, 32, 64, 9.0))
    return _done(r, err, (6e-3 if inc_mfma else 4e-3) if bf else 1e-5, f"inc dt={dtype} B={b} inc_mfma={inc_mfma}")


def outc(dtype, b):
    """casync_op_outc (1x1 conv 32 -> 3 + sigmoid -> NCHW) from 32 of 48-wide rows vs float64: fp32 2e-6 abs; bf16 input
    rounded (arithmetic fp32), 2e-6 abs."""
    torch = _t()
    g = _gen("outc", dtype, b)
    bf = dtype == 1
    dt = torch.bfloat16 if bf else torch.float32
    d = _dev()
    x = torch.randn(b, 160, 160, 48, generator=g).to(dt).to(d)
    w = (torch.randn(3, 32, generator=g) / 4).to(d)
    bias = torch.randn(3, generator=g).to(d)
    ref = torch.sigmoid(torch.einsum("oc,bhwc->bohw", w.double(), x[..., :32].double()) + bias.double()[None, :, None, None])
    out = torch.full((b, 3, 160, 160), float("nan"), device=d)
    with _Run(dtype) as r:
        _ok(_lib().casync_op_outc(_p(x), 48, _p(w), _p(bias), _p(out), b, _s()), "outc")
    return _done(r, _abs(out, ref), 2e-6, f"outc dt={dtype} B={b}")


# ------------------------------------------------------------------ frame pipeline, bf16 weight image
def frames(with_masks):
    """casync_frame_prepare + casync_frame_paste_back through frame_loop.process_batch_device (7 frames, one clamped at the
    border, one pushed past the bottom) vs the CPU restatement oracle/frame_ops_oracle.py around the same model
    predictions: bit for bit."""
    torch = _t()
    import numpy as np
    from frame_data import make_frames
    from calipsync_amd import frame_loop, recipe
    from calipsync_amd.unet import Model
    from oracle import frame_ops_oracle as fo
    net = Model(6, "hubert").to("cuda:0")
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe.make_state_dict().items()})
    net.eval()
    imgs, lms, masks = make_frames(7, 420, 560, seed=21, with_masks=with_masks)
    lms[3] = lms[3].copy()
    lms[3][:, 0] += 560 - lms[3][31, 0] + 25
    lms[5] = lms[5].copy()
    lms[5][:, 1] += 420 - (lms[5][52, 1] + (lms[5][31, 0] - lms[5][1, 0])) + 12
    wd = torch.from_numpy(np.random.default_rng(8).standard_normal((7, 32, 32, 32)).astype(np.float32)).cuda()
    want = fo.process_batch(imgs, lms, masks, lambda x: net(torch.from_numpy(x).cuda(), wd).cpu().numpy())
    with _Run(0) as r:
        got = frame_loop.process_batch_device(net, imgs, lms, masks, windows=wd)
    same = all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == 7
    changed = any(not np.array_equal(a, im) for a, im in zip(got, imgs))
    return _done(r, 0.0 if same and changed else float("inf"), 0.0, f"frames with_masks={with_masks}")


def frame_ops(name):
    """casync_frame_prepare + casync_frame_paste_back on the batch tests/frame_cases.py builds under `name`, through the C
    ABI alone: geometry records written by hand (every frame, valid or not, has a slot of its own in synth and in the mask
    buffers), masks in allocations of their own, the case's own `pred` in the model's place.  Every stage is held to the
    case's expectation bit for bit -- crops168, x, synth, area (the sharp check on the fill: one pixel of one span changes
    the count), mask_b (row pass of the dilation), mask_a (dilated mask), out_regions -- in buffers with 256 bytes of 0x5A
    either side, which must stay; an invalid frame's synth and mask_b slots stay 0x5A too, its mask_a slot holds the
    entry's zeros and its region comes back as it went in.  `what` names the first stage and frame that differ."""
    torch = _t()
    import numpy as np
    import frame_cases
    c = frame_cases.batch(name)
    B, d = len(c.regions), _dev()
    PAD, FILL = 256, 0x5A
    geom = np.zeros((B, 12), dtype=np.uint32).view(np.int32)         # casync_frame_geom: 12 int32 words per frame
    fmasks = [None if m is None else torch.from_numpy(np.ascontiguousarray(m)).to(d) for m in c.masks]
    reg_off = synth_off = mask_off = 0
    for i, r in enumerate(c.regions):
        h, w = r.shape[:2]
        geom[i, :7] = (reg_off, h, w, c.width[i], int(c.valid[i]), synth_off, mask_off)
        geom[i, 7] = -1
        if fmasks[i] is not None:
            geom[i, 7:10] = (int(c.masks[i].dtype == np.uint8), c.masks[i].shape[0], c.masks[i].shape[1])
            addr = fmasks[i].data_ptr()
            geom[i, 10:12] = np.array([addr & 0xFFFFFFFF, addr >> 32], dtype=np.uint32).view(np.int32)      # low word, high word
        reg_off, synth_off, mask_off = reg_off + h * w * 3, synth_off + c.width[i] ** 2 * 3, mask_off + h * w
    max_h, max_w = int(geom[:, 1].max()), int(geom[:, 2].max())
    max_width = int((geom[:, 3] * geom[:, 4]).max())

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(d)

    def padded(nbytes):
        return torch.full((PAD + nbytes + PAD,), FILL, dtype=torch.uint8, device=d)

    regions_d, geom_d, pts_d, pred_d = up(np.concatenate([r.reshape(-1) for r in c.regions])), up(geom), up(c.pts), up(c.pred)
    n_crop, n_x = 168 * 168 * 3, 6 * 160 * 160 * 4                  # bytes per frame of crops168 (uint8) and of x (float32)
    sizes = {"crops168": B * n_crop, "x": B * n_x, "synth": synth_off, "mask_a": mask_off, "mask_b": mask_off,
             "area": B * 4, "out_regions": reg_off}
    bufs = {k: padded(n) for k, n in sizes.items()}
    ptr = {k: b.data_ptr() + PAD for k, b in bufs.items()}
    lib = _lib()
    with _Run(0) as r:
        _ok(lib.casync_frame_prepare(_p(regions_d), _p(geom_d), B, ptr["crops168"], ptr["x"], _s()), "frame_prepare")
        _ok(lib.casync_frame_paste_back(_p(regions_d), _p(geom_d), _p(pts_d), ptr["crops168"], _p(pred_d), B, max_h, max_w, max_width,
                                        mask_off, ptr["synth"], ptr["mask_a"], ptr["mask_b"], ptr["area"], ptr["out_regions"], _s()),
            "frame_paste_back")
    torch.cuda.synchronize()
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    got = {k: v[PAD:PAD + sizes[k]] for k, v in host.items()}
    bad = []

    def hold(stage, frame, have, want):
        want = np.ascontiguousarray(want)
        have = have.view(want.dtype).reshape(want.shape)
        if not np.array_equal(have, want):
            diff = np.abs(have.astype(np.float64) - want.astype(np.float64))
            where = f"frame {frame} ({c.labels[frame]}, {c.regions[frame].shape[0]}x{c.regions[frame].shape[1]})" if frame >= 0 else "batch"
            bad.append(f"{stage} of {where}: {int((diff > 0).sum())} values differ, max |d| {diff.max():g}")

    for k, v in host.items():
        hold(f"{k} margin", -1, np.concatenate([v[:PAD], v[PAD + sizes[k]:]]), np.full(2 * PAD, FILL, np.uint8))
    for i, reg in enumerate(c.regions):
        h, w = reg.shape[:2]
        n, ns = h * w, c.width[i] ** 2 * 3
        so, mo, ro = int(geom[i, 5]), int(geom[i, 6]), int(geom[i, 0])
        hold("crops168", i, got["crops168"][i * n_crop:(i + 1) * n_crop], c.crops168[i])
        hold("x", i, got["x"][i * n_x:(i + 1) * n_x], c.x[i])
        hold("area (count of the fill)", i, got["area"][4 * i:4 * i + 4], np.array([c.area[i]], np.int32))
        if c.valid[i]:
            hold("synth", i, got["synth"][so:so + ns], c.synth[i])
            hold("mask_b (rows dilated)", i, got["mask_b"][mo:mo + n], c.rows[i])
            hold("mask_a (dilated)", i, got["mask_a"][mo:mo + n], c.final[i])
        else:
            hold("synth of an invalid frame", i, got["synth"][so:so + ns], np.full(ns, FILL, np.uint8))
            hold("mask_b of an invalid frame", i, got["mask_b"][mo:mo + n], np.full(n, FILL, np.uint8))
            hold("mask_a of an invalid frame", i, got["mask_a"][mo:mo + n], np.zeros(n, np.uint8))
        hold("out_regions", i, got["out_regions"][ro:ro + 3 * n], c.out[i])
    what = f"frame_ops {name} ({B} frames): " + (f"{bad[0]} [{len(bad)} checks failed]" if bad else "every stage equal")
    return _done(r, float("inf") if bad else 0.0, 0.0, what)


def bf16_weight_image(batch):
    """f32_to_bf16_kernel (the bf16 image of a bf16 handle's packed weights): two bf16 handles, one loads a packed buffer X
    whose GEMM / fused-block weights (the tensors the bf16 plan reads through the image) carry random low bits and exact
    rounding ties, the other loads X rounded on the host (round to nearest, ties to even).  Every other tensor of X is
    bf16-representable, so the two handles read the same fp32 values there; their forwards must be bit-equal."""
    torch = _t()
    import ctypes
    import numpy as np
    from calipsync_amd import _lib as L
    from calipsync_amd import pack, recipe
    lib = _lib()
    items, total = L.packed_layout("hubert")
    packed = np.asarray(pack.pack(recipe.make_state_dict()), dtype=np.float32)
    assert packed.size == total
    rng = np.random.default_rng(99)
    X = torch.from_numpy(packed.copy())
    rounded = X.bfloat16().float()
    imaged = torch.zeros(total, dtype=torch.bool)
    for name, off, size in items:
        if name.endswith(".w") and not name.endswith(".dw.w") and name != "outc.w":
            imaged[off:off + size] = True
    low = torch.from_numpy(rng.integers(0, 1 << 16, total, dtype=np.int64).astype(np.int32))
    bits = rounded.view(torch.int32)
    noisy = (bits | (low & 0xFFFF)).view(torch.float32)
    tie = (bits | 0x8000).view(torch.float32)
    pick = torch.from_numpy(rng.integers(0, 4, total))
    Xv = torch.where(imaged, torch.where(pick == 0, tie, noisy), rounded)
    Xv = torch.where(torch.isfinite(Xv), Xv, rounded)
    Xr = Xv.bfloat16().float()
    assert int((Xv != Xr).sum()) > 1000 and torch.equal(Xv[~imaged], Xr[~imaged])
    d = _dev()
    x, a = recipe.make_inputs(batch)
    xd, ad = torch.from_numpy(x).to(d), torch.from_numpy(a).to(d)
    outs = []
    with _Run(0) as r:
        for buf in (Xv, Xr):
            h = ctypes.c_void_p()
            _ok(lib.casync_create_ex(0, 1, ctypes.byref(h)), "create_ex")
            try:
                hb = buf.contiguous().numpy()
                _ok(lib.casync_load_weights_host(h, hb.ctypes.data, total), "load_weights_host")
                ws_bytes = lib.casync_workspace_bytes_h(h, batch)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=d)
                out = torch.full((batch, 3, 160, 160), float("nan"), device=d)
                _ok(lib.casync_forward(h, _p(xd), _p(ad), _p(out), batch, _p(ws), ws_bytes, _s()), "forward")
                torch.cuda.synchronize()
                outs.append(out.cpu())
            finally:
                lib.casync_destroy(h)
    same = torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())
    return _done(r, 0.0 if same else float("inf"), 0.0, f"bf16 weight image B={batch}")


# ------------------------------------------------------------------ the ledger
def C(fn, *params):
    return Case(fn, tuple(params))


_ROWS_GAPS = [   # (m, n, k, lda, act, res[, ldc_pad]): every shape the HuBERT forward launches (hb_run), both sides of the
    # 128x64 switch, ragged last tiles
    (1001, 512, 1536, 1024, 0, False), (9001, 512, 1536, 1024, 0, False),     # conv k=3 s=2 over 512 channels (rows overlap)
    (1001, 512, 1024, 1024, 0, False),                                        # conv k=2 s=2
    (1001, 1024, 512, 512, 0, False, 64),                                     # feature projection, C a slice of wider rows
    (1001, 3072, 1024, 1024, 0, False), (4099, 3072, 1024, 1024, 0, False),   # q|k|v
    (1001, 1024, 1024, 1024, 0, True), (4099, 1024, 1024, 1024, 0, True),     # o-proj, residual in place
    (77, 4096, 1024, 1024, 3, False), (1001, 4096, 1024, 1024, 3, False), (4099, 4096, 1024, 1024, 3, False),   # FF1 + GELU
    (1001, 1024, 4096, 4096, 0, True), (4099, 1024, 4096, 4096, 0, True),     # FF2, residual in place
]


def _rows_for(kernel):
    out = []
    for m, n, k, lda, act, res, *pad in _ROWS_GAPS:
        big = ((m + 63) // 64) * (n // 64) >= 1024
        want = ("pw_gemm_gelu_kernel" if act == 3 else "pw_gemm_glds_kernel") + (
            "<float, 128, 64, 2, 2, 2>" if big else "<float, 64, 64, 2, 2, 2>")
        if act != 3:
            want = want[:-1] + ", false>"
        if want == kernel:
            out.append(C(rows_gemm, m, n, k, lda, act, res, *pad))
    return out


# the branch-level batches of tests/frame_cases.py; with no valid frame the entry launches no synth kernel
_FRAME_OPS_SYNTH = [C(frame_ops, n) for n in ("sizes", "polygons", "masks", "invalid_mixed")]
_FRAME_OPS = _FRAME_OPS_SYNTH + [C(frame_ops, "invalid_all")]

F32, BF = 0, 1
LEDGER = {
    # ---- GEMM, fp32: LDS-DMA ring and register-staged kernels, every tile (forced), full epilogue, ragged M
    "pw_gemm_glds_kernel<float, 64, 32, 2, 1, 4, false>": [C(gemm, F32, 777, 160, 96, 4)],
    "pw_gemm_kernel<float, 128, 32, 4, 1>": [C(gemm, F32, 777, 160, 96, 3)],
    "pw_gemm_glds_kernel<float, 64, 64, 2, 2, 2, false>": [C(gemm, F32, 1001, 192, 160, 2)] + _rows_for(
        "pw_gemm_glds_kernel<float, 64, 64, 2, 2, 2, false>"),
    "pw_gemm_kernel<float, 64, 64, 2, 2>": [C(gemm, F32, 1001, 192, 160, 2, 0)],
    "pw_gemm_glds_kernel<float, 128, 64, 2, 2, 2, false>": [C(gemm, F32, 1001, 192, 160, 1)] + _rows_for(
        "pw_gemm_glds_kernel<float, 128, 64, 2, 2, 2, false>"),
    "pw_gemm_kernel<float, 128, 64, 2, 2>": [C(gemm, F32, 1001, 192, 160, 1, 0)],
    "pw_gemm_glds_kernel<float, 128, 128, 2, 2, 3, false>": [C(gemm, F32, 1001, 256, 160, 0)],
    "pw_gemm_kernel<float, 128, 128, 2, 2>": [C(gemm, F32, 1001, 256, 160, 0, 0)],
    "pw_gemm_ups_kernel<float, 64, 64, 2, 2, 2>": [C(gemm_ups, 3, 20, 64, 256), C(gemm_ups, 1, 40, 32, 128)],
    "pw_gemm_glds_kernel<float, 64, 64, 2, 2, 2, true>": [C(conv3x3, F32, 3, 9, 13, 64, 64, 1, 2, 1, -1),
                                                         C(conv3x3, F32, 5, 11, 11, 32, 128, 2, 2, 2, -1)],
    "pw_gemm_glds_kernel<float, 128, 64, 2, 2, 2, true>": [C(conv3x3, F32, 17, 32, 32, 64, 128, 2, 2, 1, 1)],
    # ---- GEMM, bf16
    "pw_gemm_glds_kernel<__bf16, 128, 128, 2, 2, 3, false>": [C(gemm, BF, 1001, 256, 192, 0)],
    "pw_gemm_glds_kernel<__bf16, 128, 128, 2, 2, 2, false>": [C(gemm, BF, 33001, 256, 128, 0, 2, 1)],
    "pw_gemm_kernel<__bf16, 128, 128, 2, 2>": [C(gemm, BF, 1001, 256, 192, 0, 0)],
    "pw_gemm_glds_kernel<__bf16, 128, 64, 2, 2, 2, false>": [C(gemm, BF, 1001, 192, 192, 1)],
    "pw_gemm_kernel<__bf16, 128, 64, 2, 2>": [C(gemm, BF, 1001, 192, 192, 1, 0)],
    "pw_gemm_glds_kernel<__bf16, 64, 64, 2, 2, 2, false>": [C(gemm, BF, 1001, 192, 192, 2)],
    "pw_gemm_kernel<__bf16, 64, 64, 2, 2>": [C(gemm, BF, 1001, 192, 192, 2, 0)],
    "pw_gemm_kernel<__bf16, 128, 32, 4, 1>": [C(gemm, BF, 777, 160, 128, 3)],
    "pw_gemm_glds_kernel<__bf16, 64, 64, 2, 2, 2, true>": [C(conv3x3, BF, 3, 9, 13, 64, 64, 1, 2, 1, -1)],
    "pw_gemm_glds_kernel<__bf16, 128, 64, 2, 2, 2, true>": [C(conv3x3, BF, 17, 32, 32, 64, 128, 2, 2, 1, 1)],
    # ---- HuBERT
    "pw_gemm_gelu_kernel<float, 64, 64, 2, 2, 2>": _rows_for("pw_gemm_gelu_kernel<float, 64, 64, 2, 2, 2>"),
    "pw_gemm_gelu_kernel<float, 128, 64, 2, 2, 2>": _rows_for("pw_gemm_gelu_kernel<float, 128, 64, 2, 2, 2>"),
    "hb_layernorm_kernel<512, false>": [C(hb_layernorm, 512, 0, 37, "strided"), C(hb_layernorm, 512, 0, 1001, "inplace")],
    "hb_layernorm_kernel<512, true>": [C(hb_layernorm, 512, 1, 37, "strided"), C(hb_layernorm, 512, 1, 1001, "inplace")],
    "hb_layernorm_kernel<1024, false>": [C(hb_layernorm, 1024, 0, 37, "strided"), C(hb_layernorm, 1024, 0, 1001, "inplace")],
    "hb_layernorm_kernel<1024, true>": [C(hb_layernorm, 1024, 1, 37, "strided"), C(hb_layernorm, 1024, 1, 1001, "inplace")],
    "hb_conv0_kernel": [C(hb_conv0, 3, 320080), C(hb_conv0, 2, 2007), C(hb_conv0, 1, 401)],
    "hb_posconv_kernel": [C(hb_posconv, 3, t) for t in (63, 64, 65, 191, 192, 193, 1000)],
    "hb_attention_kernel": [C(hb_attention, 3, 1000, False), C(hb_attention, 1, 1001, True), C(hb_attention, 2, 31, False)],
    # ---- depthwise / upsample / layout
    "dw3x3_kernel<float, 1, 4>": [C(dw3x3, F32, 2, 53, 61, 12, 1)],
    "dw3x3_kernel<float, 2, 2>": [C(dw3x3, F32, 3, 21, 13, 8, 2)],
    "dw3x3_kernel<__bf16, 1, 4>": [C(dw3x3, BF, 2, 53, 61, 16, 1)],
    "dw3x3_kernel<__bf16, 2, 2>": [C(dw3x3, BF, 3, 21, 13, 8, 2)],
    "dw3x3_lds_kernel<float, 16>": [C(dw3x3, F32, 3, 10, 10, 2048, 1)],
    "dw3x3_lds_kernel<float, 8>": [C(dw3x3, F32, 3, 40, 40, 512, 1), C(dw3x3, F32, 1, 33, 27, 96, 1)],
    "dw3x3_lds_kernel<__bf16, 16>": [C(dw3x3, BF, 3, 10, 10, 2048, 1)],
    "dw3x3_lds_kernel<__bf16, 8>": [C(dw3x3, BF, 3, 40, 40, 512, 1)],
    "dw3x3_ups_lds_kernel<16>": [C(dw3x3_ups, 3, 10, 64, 68)],
    "dw3x3_ups_lds_kernel<8>": [C(dw3x3_ups, 3, 20, 1024, 1028), C(dw3x3_ups, 1, 40, 512, 516)],
    "upsample2x_kernel<float>": [C(upsample, F32, 3, 10, 10, 256), C(upsample, F32, 2, 3, 5, 4)],
    "upsample2x_kernel<__bf16>": [C(upsample, BF, 3, 10, 10, 256)],
    "nchw_to_nhwc_kernel<float>": [C(nchw_to_nhwc, F32, 3, 32, 1024)],
    "nchw_to_nhwc_kernel<__bf16>": [C(nchw_to_nhwc, BF, 3, 32, 1024)],
    "audio_window_gather_kernel<float, false>": [C(audio_windows, F32, 1)],
    "audio_window_gather_kernel<__bf16, false>": [C(audio_windows, BF, 1)],
    "audio_window_gather_kernel<float, true>": [C(audio_windows, F32, 0)],
    "pred_to_u8_kernel": [C(pred_to_u8, 3)],
    # ---- attention, inc, outc
    "cross_attention_kernel<float>": [C(cross_attention, F32, 3), C(cross_attention, F32, 170)],
    "cross_attention_kernel<__bf16>": [C(cross_attention, BF, 3, 0)],
    "cross_attention_bf16_kernel": [C(cross_attention, BF, 3, 1)],
    "inc_kernel<float>": [C(inc, F32, 3)],
    "inc_kernel<__bf16>": [C(inc, BF, 3, 0)],
    "inc_bf16_kernel": [C(inc, BF, 3, 1)],
    "outc_kernel<float>": [C(outc, F32, 3)],
    "outc_kernel<__bf16>": [C(outc, BF, 3)],
    # ---- expand + depthwise, fp32 (32-channel tiles) and bf16 (64 / 128)
    "pw_dw_kernel<10, 1, 32, 32, 1, 4>": [C(pw_dw, F32, 10, 1, 64, 128, 3)],
    "pw_dw_kernel<10, 2, 32, 16, 1, 2>": [C(pw_dw, F32, 10, 1, 64, 128, 17), C(pw_dw, F32, 10, 1, 48, 96, 3)],
    "pw_dw_kernel<16, 1, 32, 32, 1, 3>": [C(pw_dw, F32, 16, 1, 64, 128, 3)],
    "pw_dw_kernel<16, 1, 32, 16, 1, 2>": [C(pw_dw, F32, 16, 1, 64, 128, 1), C(pw_dw, F32, 16, 1, 16, 32, 2)],
    "pw_dw_kernel<20, 1, 32, 16, 1, 2>": [C(pw_dw, F32, 20, 1, 64, 128, 3)],
    "pw_dw_kernel<20, 1, 32, 16, 2, 2>": [C(pw_dw, F32, 20, 2, 64, 128, 3)],
    "pw_dw_strip_kernel<40, 8, 1, 32, 16>": [C(pw_dw, F32, 40, 1, 64, 128, 3)],
    "pw_dw_strip_kernel<40, 4, 2, 32, 16>": [C(pw_dw, F32, 40, 2, 64, 128, 17)],
    "pw_dw_rect_kernel<16, 32, 32, 16>": [C(pw_dw, F32, 16, 1, 64, 128, f, 128, 32) for f in (1, 2, 17)] + [
        C(pw_dw, F32, 16, 1, 48, 96, 3, 128, 32)],
    "pw_dw_bf16_kernel<10, 2, 128, 1>": [C(pw_dw, BF, 10, 1, 64, 256, 5, 128)],
    "pw_dw_bf16_kernel<10, 2, 64, 1>": [C(pw_dw, BF, 10, 1, 64, 256, 5, 64)],
    "pw_dw_bf16_kernel<16, 1, 128, 1>": [C(pw_dw, BF, 16, 1, 64, 256, 3, 128)],
    "pw_dw_bf16_kernel<16, 1, 64, 1>": [C(pw_dw, BF, 16, 1, 64, 256, 3, 64)],
    "pw_dw_bf16_kernel<20, 1, 64, 1>": [C(pw_dw, BF, 20, 1, 64, 128, 3)],
    "pw_dw_bf16_kernel<20, 1, 64, 2>": [C(pw_dw, BF, 20, 2, 64, 128, 3)],
    "pw_dw_bf16_strip_kernel<40, 8, 1, 64>": [C(pw_dw, BF, 40, 1, 64, 128, 3)],
    "pw_dw_bf16_strip_kernel<40, 4, 2, 64>": [C(pw_dw, BF, 40, 2, 64, 128, 17)],
    "pw_dw_bf16_rect_kernel<16, 32, 64>": [C(pw_dw, BF, 16, 1, 64, 128, f, 128, 32) for f in (1, 2, 17)],
    # ---- fused inverted residual, fp32 (last argument: 0 plain, 1 upsample on load, 2 commuted upsample)
    "ir_fused_kernel<float, 32, 64, 32, 1, 16, 0>": [C(ir_fused, F32, 32, 32, 1, 3, 24, 40)],
    "ir_fused_kernel<float, 64, 128, 32, 1, 16, 0>": [C(ir_fused, F32, 64, 32, 1, 3, 26, 42)],
    "ir_fused_kernel<float, 128, 256, 32, 1, 16, 0>": [C(ir_fused, F32, 128, 32, 1, 3, 26, 42)],
    "ir_fused_kernel<float, 64, 128, 64, 1, 16, 0>": [C(ir_fused, F32, 64, 64, 1, 3, 26, 42)],
    "ir_fused_kernel<float, 32, 64, 64, 2, 16, 0>": [C(ir_fused, F32, 32, 64, 2, 3, 37, 51)],
    "ir_fused_kernel<float, 32, 64, 64, 1, 16, 0>": [C(ir_fused, F32, 32, 64, 1, 3, 26, 42)],
    "ir_fused_kernel<float, 64, 128, 128, 1, 16, 0>": [C(ir_fused, F32, 64, 128, 1, 3, 26, 42)],
    "ir_fused_kernel<float, 64, 128, 128, 2, 16, 0>": [C(ir_fused, F32, 64, 128, 2, 3, 37, 51)],
    "ir_fused_kernel<float, 64, 128, 32, 1, 16, 1>": [C(ir_fused_up, F32, 64, 3, 20, 52, "load")],
    "ir_fused_kernel<float, 128, 256, 32, 1, 16, 1>": [C(ir_fused_up, F32, 128, 3, 32, 48, "load")],
    "ir_fused_kernel<float, 32, 128, 32, 1, 16, 2>": [C(ir_fused_up, F32, 64, 3, 20, 52, "commuted")],
    "ir_fused_kernel<float, 64, 256, 32, 1, 16, 2>": [C(ir_fused_up, F32, 128, 3, 32, 48, "commuted")],
    # ---- frame pipeline, bf16 weight image
    "frame_resize168_kernel": [C(frames, True)] + _FRAME_OPS,
    "crop_to_input_kernel": [C(frames, True)] + _FRAME_OPS,
    "frame_synth_kernel": [C(frames, True)] + _FRAME_OPS_SYNTH,
    "frame_polyfill_kernel": [C(frames, True)] + _FRAME_OPS,
    "frame_polylines_kernel": [C(frames, True)] + _FRAME_OPS,
    "frame_area_kernel": [C(frames, True)] + _FRAME_OPS,
    "frame_dilate_kernel<true>": [C(frames, True)] + _FRAME_OPS,
    "frame_dilate_kernel<false>": [C(frames, True)] + _FRAME_OPS,
    "frame_blend_kernel": [C(frames, True), C(frames, False)] + _FRAME_OPS,
    "f32_to_bf16_kernel": [C(bf16_weight_image, 3)],
}

# fused inverted residual, bf16: depthwise on the matrix pipe (ir_dw_mfma=2) or on the VALU (0)
for (_ci, _co, _st), _hw in {(32, 32, 1): (24, 40), (64, 32, 1): (26, 42), (128, 32, 1): (26, 42), (64, 64, 1): (26, 42),
                             (32, 64, 2): (37, 51), (32, 64, 1): (26, 42), (64, 128, 1): (26, 42), (64, 128, 2): (37, 51)}.items():
    for _dwm in (True, False):
        LEDGER[f"ir_fused_bf16_kernel<{_ci}, {2 * _ci}, {_co}, {_st}, false, {str(_dwm).lower()}>"] = [
            C(ir_fused, BF, _ci, _co, _st, 3, _hw[0], _hw[1], 2 if _dwm else 0)]
for _ci, _hw in ((64, (20, 52)), (128, (32, 48))):
    for _dwm in (True, False):
        LEDGER[f"ir_fused_bf16_kernel<{_ci}, {2 * _ci}, 32, 1, true, {str(_dwm).lower()}>"] = [
            C(ir_fused_up, BF, _ci, 3, _hw[0], _hw[1], "load", 2 if _dwm else 0)]


def cases():
    """[(kernel, index, case)] in ledger order: one GPU test each"""
    return [(name, i, c) for name, cs in LEDGER.items() for i, c in enumerate(cs)]
