"""The ledger of calipsync_amd/lib/obj_hb16/ (the kernels of the bf16 HuBERT handle, csrc/hubert_bf16.hip), under the rule
of tests/kernel_ledger.py: every compiled kernel instance has op-level cases that launch it through its C-ABI entry with
the launch log on and hold it to a float64 reference computed from the SAME bf16-rounded operands.

Bars (the project's bf16 op bars):
  * kernels whose only bf16 step is the output rounding (conv0, LayerNorm, GELU): |d| / (|ref| + 1e-3) <= 2^-8 -- a bf16
    round is 2^-9 relative, the floor leaves room for the fp32 arithmetic near zero; fp32 outputs keep the 1e-4 absolute
    bar of the fp32 HuBERT kernels; the in-place h update is one fp32 add: 1e-6 absolute on values of a few units;
  * attention: max |d| <= 2^-7 max |ref| (the cross_attention bf16 bar);
  * the bf16 rows GEMM: |d| / (|ref| + 1) < 2^-8 (kernel_ledger._bf16_rel1).
ROWS_GEMM lists the shapes of kernel_ledger._ROWS_GAPS that the bf16 forward launches; the GEMM adds no kernel, so each of
its cases names the EXISTING instance of lib/obj/ it must launch.

Nothing here touches a GPU at import.
"""
from __future__ import annotations

from kernel_ledger import (C, _abs, _bf16_rel1, _dev, _done, _gen, _lib, _ok, _p, _rel, _Run, _s, _sentinel, _t)


def _rel_floor(got, ref, floor=1e-3):
    torch = _t()
    got, ref = got.double(), ref.double().to(got.device)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / (ref.abs() + floor)).max())


BAR16 = 2 ** -8


# ------------------------------------------------------------------ attention
def hb16_attention(B, T, peaked):
    """casync_op_hubert16_attention from the fused bf16 q|k|v rows vs float64 on the same operands; `peaked` as
    kernel_ledger.hb_attention (every query's largest score is key T-1, alone in the last key tile).  The output rows sit
    between sentinel rows."""
    torch = _t()
    g = _gen("att16", B, T, peaked)
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
    qd = qkv.bfloat16().to(d)
    q, k, v = (z.reshape(B, T, 16, 64).transpose(1, 2) for z in qd.double().split(1024, dim=1))
    s = q @ k.transpose(-1, -2)
    if peaked:
        assert bool((s.argmax(-1) == T - 1).all())
    ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * T, 1024)
    pad = 8
    out = torch.full((B * T + 2 * pad, 1024), -7.0, device=d, dtype=torch.bfloat16)
    with _Run(0) as r:
        _ok(_lib().casync_op_hubert16_attention(_p(qd), out.data_ptr() + pad * 1024 * 2, B, T, _s()), "attention16")
    err = _rel(out[pad:pad + B * T], ref)
    if not bool((out[:pad].float() == -7.0).all() and (out[pad + B * T:].float() == -7.0).all()):
        err = float("inf")
    return _done(r, err, 2 ** -7, f"hubert16 attention B={B} T={T} peaked={peaked}")


# ------------------------------------------------------------------ LayerNorm
def hb16_layernorm512(out_f32, rows, mode):
    """casync_op_hubert16_layernorm512: bf16 rows in; bf16 out with GELU (out_f32 0) or fp32 out (1).  mode 'strided':
    slices of wider sentinel-filled buffers; 'inplace': in == out (bf16 only), as the conv stack runs it."""
    torch = _t()
    F = torch.nn.functional
    g = _gen("ln512_16", out_f32, rows, mode)
    d = _dev()
    x = (torch.randn(rows, 512, generator=g) * 3 + 1).bfloat16().to(d)
    gm, be = torch.randn(512, generator=g).to(d), torch.randn(512, generator=g).to(d)
    ref = F.layer_norm(x.double(), (512,), gm.double(), be.double(), 1e-5)
    ref = ref if out_f32 else F.gelu(ref)
    odt, oes = (torch.float32, 4) if out_f32 else (torch.bfloat16, 2)
    lib = _lib()
    if mode == "inplace":
        buf = x.clone()
        with _Run(0) as r:
            _ok(lib.casync_op_hubert16_layernorm512(_p(buf), 512, _p(buf), 512, rows, _p(gm), _p(be), 1e-5, 0, 1, _s()), "ln512")
        err = _rel_floor(buf, ref)
    else:
        ldi, ldo = 512 + 32, 512 + 64
        inb = torch.full((rows, ldi), 9.0, device=d, dtype=torch.bfloat16)
        inb[:, 32:] = x
        out = torch.full((rows, ldo), -7.0, device=d, dtype=odt)
        with _Run(0) as r:
            _ok(lib.casync_op_hubert16_layernorm512(inb.data_ptr() + 64, ldi, out.data_ptr() + 16 * oes, ldo, rows, _p(gm), _p(be),
                                                    1e-5, out_f32, 0 if out_f32 else 1, _s()), "ln512")
        err = _abs(out[:, 16:16 + 512], ref) / 1e-4 * BAR16 if out_f32 else _rel_floor(out[:, 16:16 + 512], ref)
        err = max(err, _sentinel(out, 16, 16 + 512, -7.0))
    return _done(r, err, BAR16, f"hubert16 layernorm512 out_f32={out_f32} rows={rows} {mode}")


def hb16_layernorm1024(out_f32, delta, store_h, rows, strided):
    """casync_op_hubert16_layernorm1024: v = h (+ bf16 delta), h = v when store_h, out = LayerNorm(v) as bf16 or fp32.
    strided: h, delta and out are slices of wider sentinel-filled buffers.  The h update is checked too (1e-6 absolute),
    and h must be untouched where it is not to be stored."""
    torch = _t()
    F = torch.nn.functional
    g = _gen("ln1024_16", out_f32, delta, store_h, rows, strided)
    d = _dev()
    h0 = (torch.randn(rows, 1024, generator=g) * 3 + 1).to(d)
    dl = (torch.randn(rows, 1024, generator=g)).bfloat16().to(d)
    gm, be = torch.randn(1024, generator=g).to(d), torch.randn(1024, generator=g).to(d)
    v = h0.double() + (dl.double() if delta else 0.0)
    ref = F.layer_norm(v, (1024,), gm.double(), be.double(), 1e-5)
    pad_h, pad_d, pad_o = (32, 16, 64) if strided else (0, 0, 0)
    odt, oes = (torch.float32, 4) if out_f32 else (torch.bfloat16, 2)
    hb = torch.full((rows, 1024 + 2 * pad_h), 5.0, device=d)
    hb[:, pad_h:pad_h + 1024] = h0
    db = torch.full((rows, 1024 + 2 * pad_d), 3.0, device=d, dtype=torch.bfloat16)
    db[:, pad_d:pad_d + 1024] = dl
    out = torch.full((rows, 1024 + 2 * pad_o), -7.0, device=d, dtype=odt)
    with _Run(0) as r:
        _ok(_lib().casync_op_hubert16_layernorm1024(hb.data_ptr() + 4 * pad_h, hb.shape[1], (db.data_ptr() + 2 * pad_d) if delta else 0,
                                                    db.shape[1], store_h, out.data_ptr() + oes * pad_o, out.shape[1], rows, _p(gm),
                                                    _p(be), 1e-5, out_f32, _s()), "ln1024")
    got = out[:, pad_o:pad_o + 1024]
    err = _abs(got, ref) / 1e-4 * BAR16 if out_f32 else _rel_floor(got, ref)
    want_h = v if (delta and store_h) else h0.double()
    err = max(err, _abs(hb[:, pad_h:pad_h + 1024], want_h) / 1e-6 * BAR16)
    if strided:
        err = max(err, _sentinel(out, pad_o, pad_o + 1024, -7.0), _sentinel(hb, pad_h, pad_h + 1024, 5.0))
    return _done(r, err, BAR16, f"hubert16 layernorm1024 out_f32={out_f32} delta={delta} store_h={store_h} rows={rows} strided={strided}")


# ------------------------------------------------------------------ conv0, GELU, widen
def hb16_conv0(B, S):
    """casync_op_hubert16_conv0 (conv k=10 s=5 + LayerNorm + GELU, bf16 out) vs float64; the rows sit between sentinel rows."""
    torch = _t()
    F = torch.nn.functional
    g = _gen("conv0_16", B, S)
    d = _dev()
    x = torch.randn(B, S, generator=g).to(d)
    W = (torch.randn(512, 10, generator=g) / 3).to(d)
    b, gm, be = (torch.randn(512, generator=g).to(d) for _ in range(3))
    T0 = (S - 10) // 5 + 1
    y = x.double().unfold(1, 10, 5) @ W.double().T + b.double()
    ref = F.gelu(F.layer_norm(y, (512,), gm.double(), be.double(), 1e-5)).reshape(B * T0, 512)
    pad = 4
    out = torch.full((B * T0 + 2 * pad, 512), -7.0, device=d, dtype=torch.bfloat16)
    with _Run(0) as r:
        _ok(_lib().casync_op_hubert16_conv0(_p(x), B, S, _p(W), _p(b), _p(gm), _p(be), out.data_ptr() + pad * 512 * 2, _s()), "conv0_16")
    err = _rel_floor(out[pad:pad + B * T0], ref)
    if not bool((out[:pad].float() == -7.0).all() and (out[pad + B * T0:].float() == -7.0).all()):
        err = float("inf")
    return _done(r, err, BAR16, f"hubert16 conv0 B={B} S={S}")


def hb16_gelu(n):
    """casync_op_hubert16_gelu in place over n bf16 inside a sentinel-filled buffer vs float64 erf GELU."""
    torch = _t()
    g = _gen("gelu16", n)
    d = _dev()
    x = (torch.randn(n, generator=g) * 2.5).bfloat16().to(d)
    ref = torch.nn.functional.gelu(x.double())
    buf = torch.full((n + 32,), -7.0, device=d, dtype=torch.bfloat16)
    buf[16:16 + n] = x
    with _Run(0) as r:
        _ok(_lib().casync_op_hubert16_gelu(buf.data_ptr() + 32, n, _s()), "gelu16")
    err = max(_rel_floor(buf[16:16 + n], ref), _sentinel(buf, 16, 16 + n, -7.0))
    return _done(r, err, BAR16, f"hubert16 gelu n={n}")


def hb16_widen(n):
    """casync_op_hubert16_widen: bf16 -> fp32, exact."""
    torch = _t()
    g = _gen("widen16", n)
    d = _dev()
    x = (torch.randn(n, generator=g) * 2.5).bfloat16().to(d)
    out = torch.full((n + 16,), -7.0, device=d)
    with _Run(0) as r:
        _ok(_lib().casync_op_hubert16_widen(_p(x), out.data_ptr() + 32, n, _s()), "widen16")
    same = bool(torch.equal(out[8:8 + n], x.float())) and _sentinel(out, 8, 8 + n, -7.0) == 0.0
    return _done(r, 0.0 if same else float("inf"), 0.0, f"hubert16 widen n={n}")


# ------------------------------------------------------------------ the bf16 rows GEMM (no kernel of its own)
def rows_gemm_bf16_kernel(m, n):
    """The existing bf16 ring instance launch_rows_gemm_bf16 picks for an m x n output (gemm.hip): the tile with the fewest
    rounds of one tile per CU x (tile area + 6000), the larger tile on ties; 128x128 on the three-stage ring up to one
    tile per CU, on the two-stage ring above."""
    best, best_cost = None, None
    for bm, bn in ((128, 128), (128, 64), (64, 64)):
        if n % bn:
            continue
        g = -(-m // bm) * (n // bn)
        cost = -(-g // 256) * (bm * bn + 6000.0)
        if best is None or cost < best_cost:
            best, best_cost = (bm, bn, g), cost
    bm, bn, g = best
    nst = (3 if g <= 256 else 2) if (bm, bn) == (128, 128) else 2
    return f"pw_gemm_glds_kernel<__bf16, {bm}, {bn}, 2, 2, {nst}, false>"


def rows_gemm_bf16(m, n, k, lda, ldc_pad=0):
    """casync_op_rows_gemm_bf16 at a shape the bf16 HuBERT forward launches: C = A W^T + bias with bf16 A, W, C.  lda < k:
    the A rows overlap (a channels-last conv).  ldc_pad > 0: C is a slice of a wider sentinel-filled buffer."""
    torch = _t()
    g = _gen("rows16", m, n, k, lda)
    d = _dev()
    flat = torch.randn((m - 1) * lda + k, generator=g).bfloat16().to(d)
    W = (torch.randn(n, k, generator=g) / k ** 0.5).bfloat16().to(d)
    b = torch.randn(n, generator=g).to(d)
    a = flat.as_strided((m, k), (lda, 1))
    ref = a.double() @ W.double().T + b.double()
    ldc = n + ldc_pad
    c = torch.full((m, ldc), -7.0, device=d, dtype=torch.bfloat16)
    with _Run(0) as r:
        _ok(_lib().casync_op_rows_gemm_bf16(_p(flat), lda, _p(W), _p(b), _p(c), ldc, m, n, k, _s()), "rows_gemm_bf16")
    err = _bf16_rel1(c[:, :n], ref)
    if ldc_pad:
        err = max(err, _sentinel(c, 0, n, -7.0))
    return _done(r, err, BAR16, f"rows_gemm_bf16 {m}x{n}x{k} lda={lda} ldc={ldc}")


ROWS_GEMM = [   # (m, n, k, lda[, ldc_pad]): kernel_ledger._ROWS_GAPS without the feature projection (fp32 in this handle)
    (1001, 512, 1536, 1024), (9001, 512, 1536, 1024),      # conv k=3 s=2 over 512 channels (rows overlap)
    (1001, 512, 1024, 1024, 64),                           # conv k=2 s=2, C a slice of wider rows
    (1001, 3072, 1024, 1024), (4099, 3072, 1024, 1024),    # q|k|v
    (1001, 1024, 1024, 1024), (4099, 1024, 1024, 1024),    # out-proj (the delta)
    (77, 4096, 1024, 1024), (1001, 4096, 1024, 1024), (4099, 4096, 1024, 1024),   # FF1
    (1001, 1024, 4096, 4096), (4099, 1024, 4096, 4096),    # FF2 (the delta)
]


def rows_gemm_cases():
    """[(existing kernel it must launch, case)]"""
    return [(rows_gemm_bf16_kernel(s[0], s[1]), C(rows_gemm_bf16, *s)) for s in ROWS_GEMM]


# ------------------------------------------------------------------ the ledger of lib/obj_hb16/
LEDGER = {
    "hb16_attention_kernel": [C(hb16_attention, 3, 1000, False), C(hb16_attention, 1, 1001, True), C(hb16_attention, 2, 31, False),
                              C(hb16_attention, 1, 1, False)],
    "hb16_layernorm512_kernel<false, true>": [C(hb16_layernorm512, 0, 37, "strided"), C(hb16_layernorm512, 0, 1001, "inplace")],
    "hb16_layernorm512_kernel<true, false>": [C(hb16_layernorm512, 1, 37, "strided"), C(hb16_layernorm512, 1, 1001, "strided")],
    "hb16_layernorm1024_kernel<false>": [C(hb16_layernorm1024, 0, 0, 1, 37, True), C(hb16_layernorm1024, 0, 1, 1, 1001, False),
                                         C(hb16_layernorm1024, 0, 1, 1, 37, True), C(hb16_layernorm1024, 0, 1, 0, 37, True)],
    "hb16_layernorm1024_kernel<true>": [C(hb16_layernorm1024, 1, 1, 0, 1001, False), C(hb16_layernorm1024, 1, 0, 0, 37, True),
                                        C(hb16_layernorm1024, 1, 1, 1, 37, True)],
    "hb16_conv0_kernel": [C(hb16_conv0, 3, 320080), C(hb16_conv0, 2, 2007), C(hb16_conv0, 1, 401)],
    "hb16_gelu_kernel": [C(hb16_gelu, 1001 * 4096), C(hb16_gelu, 8)],
    "hb16_widen_kernel": [C(hb16_widen, 1001 * 512), C(hb16_widen, 8)],
}


def cases():
    """[(kernel, index, case)] in ledger order: one GPU test each"""
    return [(name, i, c) for name, cs in LEDGER.items() for i, c in enumerate(cs)]
