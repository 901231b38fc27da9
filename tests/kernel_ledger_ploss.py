"""The ledger of calipsync_amd/lib/obj_ploss/ (the kernels of the trainer's loss, csrc/ploss.hip), under the rule of
tests/kernel_ledger.py: every compiled kernel has op-level cases that launch it through its casync_op_ploss_* entry with the
launch log on.  Kernels that move, mask or compare data are held bit for bit against numpy / torch on the CPU (the error is the
number of differing floats, inf where a sentinel behind the output changed, the bar 0); the two kernels that sum products (the
stem in both directions) are held, on max and on mean error against float64, to 4x the error of fp32 torch on the CPU doing the
same conv (the error is the larger of the two ratios over 4, the bar 1).  tests/test_ploss_gpu.py runs the same helpers on the
shapes the issue names.  Nothing here touches a GPU at import."""
from __future__ import annotations

import numpy as np

import vgg_ref
from kernel_ledger import C, _done, _gen, _lib, _Run, _s, _t

PAD = 64
SENTINEL = -777.0


def _padded(n):
    """a sentinel-filled device buffer with PAD floats behind the n the kernel may write -> (buffer, view of the n)"""
    torch = _t()
    buf = torch.full((n + PAD,), SENTINEL, dtype=torch.float32, device="cuda:0")
    return buf, buf[:n]


def _intact(buf, n):
    return bool((buf[n:] == SENTINEL).all())


def _differ(got, want):
    """floats of `got` (a device or host tensor) whose bits (up to the sign of zero) differ from `want` (host)"""
    torch = _t()
    return float((got.cpu() != torch.as_tensor(want)).sum())


def ratio4(got, ref64, ref32):
    """max and mean error of got against ref64, over 4x the same of ref32 -> the larger ratio (the bar is 1), with the figures"""
    torch = _t()
    got, ref32 = got.cpu().double(), ref32.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf"), "not finite"
    e, r = (got - ref64).abs(), (ref32 - ref64).abs()
    floor = 2.0 ** -24 * float(ref64.abs().max())            # fp32 torch exact to the last bit everywhere: one rounding of the largest value
    r_max, r_mean = max(float(r.max()), floor), max(float(r.mean()), floor / 16)
    ratios = float(e.max()) / r_max, float(e.mean()) / r_mean
    return max(ratios) / 4.0, f"max {float(e.max()):.3e} ({ratios[0]:.2f}x fp32 torch), mean {float(e.mean()):.3e} ({ratios[1]:.2f}x)"


# ------------------------------------------------------------------------------------------------ the kernels
def run_stem(x, w, bias):
    """x [B,3,H,W], w [64,3,3,3], bias [64] (host tensors) -> (out [B,H,W,64] on the device, sentinel intact)"""
    b, _, h, wd = x.shape
    rows = w.permute(2, 3, 1, 0).reshape(27, 64).contiguous()
    buf, out = _padded(b * h * wd * 64)
    xd, rd, bd = x.cuda(), rows.cuda(), bias.cuda()          # (held: a temporary's block would be handed to the next upload)
    st = _lib().casync_op_ploss_stem(xd.data_ptr(), rd.data_ptr(), bd.data_ptr(), out.data_ptr(), b, h, wd, _s())
    assert st == 0, st
    _t().cuda.synchronize()
    return out.reshape(b, h, wd, 64), _intact(buf, out.numel())


def stem(b, h, wd):
    torch = _t()
    F = torch.nn.functional
    g = _gen("ploss stem", b, h, wd)
    x = torch.rand(b, 3, h, wd, generator=g)
    w = torch.randn(64, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5
    bias = torch.randn(64, generator=g) * 0.05
    with _Run(0) as r:
        out, ok = run_stem(x, w, bias)
    ref64 = vgg_ref.nhwc(F.relu(F.conv2d(x.double(), w.double(), bias.double(), padding=1)))
    ref32 = vgg_ref.nhwc(F.relu(F.conv2d(x, w, bias, padding=1)))
    err, what = ratio4(out, ref64, ref32)
    return _done(r, err if ok else float("inf"), 1.0, f"stem B={b} {h}x{wd}: {what}")


def run_pool(a):
    """a [B,H,W,C] host -> (out [B,H/2,W/2,C] device, intact)"""
    b, h, wd, c = a.shape
    buf, out = _padded(b * (h // 2) * (wd // 2) * c)
    ad = a.cuda()
    st = _lib().casync_op_ploss_pool(ad.data_ptr(), out.data_ptr(), b, h, wd, c, _s())
    assert st == 0, st
    _t().cuda.synchronize()
    return out.reshape(b, h // 2, wd // 2, c), _intact(buf, out.numel())


def activation(b, h, wd, c, *key):
    """a post-ReLU activation [B,H,W,C] with what the pool adjoint must get right: about a third zeros, values drawn from 16
    levels (so windows with two equal positive maxima are common), the windows at (0, 0) all zero and at (0, 1) (where there is
    one) four equal positive values"""
    torch = _t()
    g = _gen("ploss activation", b, h, wd, c, *key)
    a = torch.randint(0, 16, (b, h, wd, c), generator=g).float() * 0.25
    a = torch.where(torch.rand(b, h, wd, c, generator=g) < 0.33, torch.zeros(()), a)
    a[:, 0:2, 0:2] = 0.0
    if wd >= 4:
        a[:, 0:2, 2:4] = 1.5
    return a


def pool(b, h, wd, c):
    torch = _t()
    a = activation(b, h, wd, c, "pool") - 1.0       # negatives too
    with _Run(0) as r:
        out, ok = run_pool(a)
    want = vgg_ref.nhwc(torch.nn.functional.max_pool2d(vgg_ref.nchw(a), 2, 2))
    return _done(r, _differ(out, want) if ok else float("inf"), 0.0, f"floor pool B={b} {h}x{wd}x{c}")


def run_wflip(w, cout, cin):
    buf, out = _padded(9 * cout * cin)
    wd = w.cuda()
    st = _lib().casync_op_ploss_weight_transform(wd.data_ptr(), out.data_ptr(), cout, cin, _s())
    assert st == 0, st
    _t().cuda.synchronize()
    return out, _intact(buf, out.numel())


def wflip(cout, cin):
    torch = _t()
    from calipsync_amd import losses
    w = torch.randn(9 * cout * cin, generator=_gen("ploss wflip", cout, cin))
    with _Run(0) as r:
        out, ok = run_wflip(w, cout, cin)
        back, ok2 = run_wflip(out.clone(), cin, cout)
    err = _differ(out, losses.weight_transform(w.numpy(), cout, cin)) + _differ(back, w)
    return _done(r, err if ok and ok2 else float("inf"), 0.0, f"weight transform {cout} x 9 x {cin}, and back")


def run_split(x, rows, c):
    buf, out = _padded(rows * c)
    xd = x.cuda()
    st = _lib().casync_op_ploss_split(xd.data_ptr(), out.data_ptr(), rows, c, _s())
    assert st == 0, st
    _t().cuda.synchronize()
    return out.reshape(c // 64, rows, 64), _intact(buf, rows * c)


def split(rows, c):
    torch = _t()
    x = torch.randn(rows, c, generator=_gen("ploss split", rows, c))
    with _Run(0) as r:
        out, ok = run_split(x, rows, c)
    want = x.reshape(rows, c // 64, 64).permute(1, 0, 2).contiguous()
    return _done(r, _differ(out, want) if ok else float("inf"), 0.0, f"{c // 64} slices of {rows} x {c}")


def run_combine(part, bias, relu):
    g, n, c = part.shape[0], part[0].numel(), part.shape[-1]
    buf, out = _padded(n)
    pd, bd = part.cuda(), None if bias is None else bias.cuda()
    st = _lib().casync_op_ploss_combine(pd.data_ptr(), g, None if bd is None else bd.data_ptr(), out.data_ptr(), n, c, int(relu), _s())
    assert st == 0, st
    _t().cuda.synchronize()
    return out.reshape(part.shape[1:]), _intact(buf, n)


def combine(g, rows, c, with_bias, relu):
    """((p0 + p1) + (p2 + p3)) + bias, ReLU: each fp32 sum rounded on its own, so numpy's float32 sums are the same bits"""
    torch = _t()
    gen = _gen("ploss combine", g, rows, c, with_bias, relu)
    part = torch.randn(g, rows, c, generator=gen)
    bias = torch.randn(c, generator=gen) if with_bias else None
    with _Run(0) as r:
        out, ok = run_combine(part, bias, relu)
    want = part[0] + part[1]
    if g == 4:
        want = want + (part[2] + part[3])
    if with_bias:
        want = want + bias
    if relu:
        want = torch.where(want > 0, want, torch.zeros(()))
    return _done(r, _differ(out, want) if ok else float("inf"), 0.0, f"{g} partial outputs of {rows} x {c}, bias {with_bias}, ReLU {relu}")


def run_relu_bwd(g, a):
    n = g.numel()
    buf, out = _padded(n)
    out.copy_(g.reshape(-1))
    ad = a.cuda()
    st = _lib().casync_op_ploss_relu_bwd(out.data_ptr(), ad.data_ptr(), n, _s())
    assert st == 0, st
    _t().cuda.synchronize()
    return out.reshape(g.shape), _intact(buf, n)


def relu_bwd(n):
    torch = _t()
    gen = _gen("ploss relu_bwd", n)
    g = torch.randn(n, generator=gen)
    a = torch.randn(n, generator=gen)
    a[::5] = 0.0
    a[1::7] = -0.0
    with _Run(0) as r:
        out, ok = run_relu_bwd(g, a)
    return _done(r, _differ(out, vgg_ref.relu_mask(g, a)) if ok else float("inf"), 0.0, f"ReLU adjoint of {n}")


def run_pool_bwd(gp, a):
    """gp [B,H/2,W/2,C], a [B,H,W,C] host -> (g [B,H,W,C] device, intact); the output starts as NaN: every element must be written"""
    torch = _t()
    b, h, wd, c = a.shape
    buf, out = _padded(a.numel())
    out.fill_(float("nan"))
    gd, ad = gp.cuda(), a.cuda()
    st = _lib().casync_op_ploss_pool_bwd(gd.data_ptr(), ad.data_ptr(), out.data_ptr(), b, h, wd, c, _s())
    assert st == 0, st
    torch.cuda.synchronize()
    return out.reshape(a.shape), _intact(buf, a.numel())


def pool_bwd(b, h, wd, c):
    torch = _t()
    a = activation(b, h, wd, c, "pool_bwd")
    gp = torch.randn(b, h // 2, wd // 2, c, generator=_gen("ploss pool_bwd g", b, h, wd, c))
    with _Run(0) as r:
        out, ok = run_pool_bwd(gp, a)
    want = vgg_ref.nhwc(vgg_ref.pool_adjoint(vgg_ref.nchw(gp), vgg_ref.nchw(a)))
    # torch's own max_pool2d backward agrees on where the gradient goes (its > rule); the ReLU mask is ours
    an = vgg_ref.nchw(a).requires_grad_(True)
    torch.nn.functional.max_pool2d(an, 2, 2).backward(vgg_ref.nchw(gp))
    assert torch.equal(vgg_ref.relu_mask(an.grad, an.detach()), vgg_ref.nchw(want)), "the restatement disagrees with torch's pool backward"
    return _done(r, _differ(out, want) if ok else float("inf"), 0.0, f"pool + ReLU adjoint B={b} {h}x{wd}x{c}")


def run_stem_bwd(g1, w, pred, label, s, perc_scale, pix_scale):
    """g1 [B,H,W,64], w [64,3,3,3]; pred / label [B,3,H,W] or None -> (grad_pred [B,3,H,W] device, intact)"""
    torch = _t()
    b, h, wd, _ = g1.shape
    rows = w.permute(2, 3, 1, 0).reshape(27, 64).contiguous().cuda()
    buf, out = _padded(b * 3 * h * wd)
    sd = torch.tensor(s, dtype=torch.float32, device="cuda:0")
    pd, ld = (None, None) if pred is None else (pred.cuda(), label.cuda())
    gd = g1.cuda()
    st = _lib().casync_op_ploss_stem_bwd(gd.data_ptr(), rows.data_ptr(), None if pd is None else pd.data_ptr(),
                                         None if ld is None else ld.data_ptr(), sd.data_ptr(), out.data_ptr(), b, h, wd, perc_scale, pix_scale, _s())
    assert st == 0, st
    torch.cuda.synchronize()
    return out.reshape(b, 3, h, wd), _intact(buf, out.numel())


def pixel_pair(b, h, wd, *key):
    """(pred, label) with pred == label on about a quarter of the pixels"""
    torch = _t()
    g = _gen("ploss pixel pair", b, h, wd, *key)
    label = torch.rand(b, 3, h, wd, generator=g)
    pred = torch.where(torch.rand(b, 3, h, wd, generator=g) < 0.25, label, torch.rand(b, 3, h, wd, generator=g))
    return pred, label


def stem_bwd(b, h, wd):
    """the sign term alone (g1 = 0) bit for bit, then the conv term alone (no pixel term) to the 4x bar, then both with s = 4 against
    s = 1: exactly 4x the bits"""
    torch = _t()
    F = torch.nn.functional
    g = _gen("ploss stem_bwd", b, h, wd)
    w = torch.randn(64, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5
    g1 = torch.randn(b, h, wd, 64, generator=g)
    g1 = torch.where(torch.rand(b, h, wd, 64, generator=g) < 0.4, torch.zeros(()), g1)          # masked, as the chain hands it over
    pred, label = pixel_pair(b, h, wd)
    pix_scale, perc_scale, s = np.float32(1.0 / pred.numel()), np.float32(0.2 / (b * 256 * max(h // 4, 1) * max(wd // 4, 1))), np.float32(0.75)
    with _Run(0) as r:
        sign_only, ok1 = run_stem_bwd(torch.zeros_like(g1), w, pred, label, float(s), float(perc_scale), float(pix_scale))
        conv_only, ok2 = run_stem_bwd(g1, w, None, None, 1.0, 1.0, 0.0)
        both1, ok3 = run_stem_bwd(g1, w, pred, label, 1.0, float(perc_scale), float(pix_scale))
        both4, ok4 = run_stem_bwd(g1, w, pred, label, 4.0, float(perc_scale), float(pix_scale))
    want_sign = s * (pix_scale * np.sign(pred.numpy() - label.numpy()).astype(np.float32))
    exact = _differ(sign_only, want_sign) + _differ(both4, 4.0 * both1.cpu())
    ref64 = F.conv_transpose2d(vgg_ref.nchw(g1).double(), w.double(), padding=1)
    ref32 = F.conv_transpose2d(vgg_ref.nchw(g1), w, padding=1)
    err, what = ratio4(conv_only, ref64, ref32)
    ok = ok1 and ok2 and ok3 and ok4 and exact == 0
    return _done(r, err if ok else float("inf"), 1.0, f"stem adjoint B={b} {h}x{wd}: sign term and x4 {exact:.0f} floats differ; conv term {what}")


def run_sqdiff(fp, fl):
    torch = _t()
    n = fp.numel()
    parts = _lib().casync_ploss_partials(n // 4)
    buf, d = _padded(n)
    part = torch.full((parts + 8,), -1.0, dtype=torch.float64, device="cuda:0")
    pd, ld = fp.cuda(), fl.cuda()
    st = _lib().casync_op_ploss_sqdiff(pd.data_ptr(), ld.data_ptr(), d.data_ptr(), n, part.data_ptr(), _s())
    assert st == 0, st
    torch.cuda.synchronize()
    return d, part[:parts], _intact(buf, n) and bool((part[parts:] == -1.0).all())


def sqdiff(n):
    torch = _t()
    g = _gen("ploss sqdiff", n)
    fp, fl = torch.randn(n, generator=g), torch.randn(n, generator=g)
    with _Run(0) as r:
        d, part, ok = run_sqdiff(fp, fl)
        d2, part2, _ = run_sqdiff(fp, fl)
    want = fp - fl
    total = float((want.double() ** 2).sum())
    rel = abs(float(part.sum()) - total) / total
    exact = _differ(d, want) + float((part != part2).sum()) + float((d != d2).sum())
    return _done(r, rel if ok and exact == 0 else float("inf"), 1e-13, f"d and sum d^2 of {n} in {part.numel()} partial sums: {exact:.0f} floats differ")


def run_absdiff(pred, label):
    torch = _t()
    n = pred.numel()
    parts = _lib().casync_ploss_partials(n)
    part = torch.full((parts + 8,), -1.0, dtype=torch.float64, device="cuda:0")
    pd, ld = pred.cuda(), label.cuda()
    st = _lib().casync_op_ploss_absdiff(pd.data_ptr(), ld.data_ptr(), n, part.data_ptr(), _s())
    assert st == 0, st
    torch.cuda.synchronize()
    return part[:parts], bool((part[parts:] == -1.0).all())


def absdiff(n):
    torch = _t()
    g = _gen("ploss absdiff", n)
    pred, label = torch.rand(n, generator=g), torch.rand(n, generator=g)
    with _Run(0) as r:
        part, ok = run_absdiff(pred, label)
        part2, _ = run_absdiff(pred, label)
    total = float((pred - label).abs().double().sum())
    rel = abs(float(part.sum()) - total) / total
    return _done(r, rel if ok and bool((part == part2).all()) else float("inf"), 1e-13, f"sum |pred - label| of {n} in {part.numel()} partial sums")


def run_finish(part_sq, count_sq, part_abs, count_abs, w_pix, w_perc):
    torch = _t()
    buf, out = _padded(3)
    ps = torch.as_tensor(part_sq, dtype=torch.float64).cuda()
    pa = None if part_abs is None else torch.as_tensor(part_abs, dtype=torch.float64).cuda()
    st = _lib().casync_op_ploss_finish(ps.data_ptr(), ps.numel(), count_sq, None if pa is None else pa.data_ptr(), 0 if pa is None else pa.numel(),
                                       count_abs, w_pix, w_perc, out.data_ptr(), _s())
    assert st == 0, st
    torch.cuda.synchronize()
    return out, _intact(buf, 3)


def finish(n_sq, n_abs):
    """partial sums that are small integers (their float64 sum is exact in any order): the three values bit for bit"""
    rng = np.random.default_rng(n_sq * 1031 + n_abs)
    ps, pa = rng.integers(0, 1 << 20, n_sq).astype(np.float64), rng.integers(0, 1 << 20, max(n_abs, 1)).astype(np.float64)
    count_sq, count_abs, w_pix, w_perc = 3 * 256 * 40 * 40, 3 * 3 * 160 * 160, np.float32(1.0), np.float32(0.1)
    with _Run(0) as r:
        out, ok = run_finish(ps, count_sq, pa if n_abs else None, count_abs, float(w_pix), float(w_perc))
    perc = np.float32(ps.sum() / count_sq)
    pix = np.float32(pa.sum() / count_abs) if n_abs else np.float32(0.0)
    want = np.asarray([w_pix * pix + w_perc * perc, pix, perc], dtype=np.float32)
    return _done(r, _differ(out, want) if ok else float("inf"), 0.0, f"losses from {n_sq} + {n_abs} partial sums")


# odd sizes, sizes that are no multiple of a workgroup's items, more than one workgroup; the reductions also past their 1024
# workgroups (a second round of the grid-stride loop)
LEDGER = {
    "ploss_stem_kernel": [C(stem, 1, 4, 4), C(stem, 3, 7, 9), C(stem, 2, 13, 19)],
    "ploss_pool_kernel": [C(pool, 1, 4, 4, 64), C(pool, 2, 7, 9, 64), C(pool, 3, 10, 13, 128)],
    "ploss_wflip_kernel": [C(wflip, 64, 64), C(wflip, 128, 64), C(wflip, 256, 128)],
    "ploss_split_kernel": [C(split, 1, 128), C(split, 35, 256), C(split, 9 * 128, 128), C(split, 1031, 64)],
    "ploss_combine_kernel": [C(combine, 2, 1, 128, True, True), C(combine, 4, 35, 256, True, False), C(combine, 4, 1031, 128, False, False),
                             C(combine, 2, 77, 64, False, True)],
    "ploss_relu_bwd_kernel": [C(relu_bwd, 4), C(relu_bwd, 6 * 1024 + 4)],
    "ploss_pool_bwd_kernel": [C(pool_bwd, 1, 4, 4, 64), C(pool_bwd, 2, 7, 9, 64), C(pool_bwd, 3, 10, 13, 128), C(pool_bwd, 1, 5, 6, 128)],
    "ploss_stem_bwd_kernel": [C(stem_bwd, 1, 4, 4), C(stem_bwd, 3, 7, 9), C(stem_bwd, 2, 13, 19)],
    "ploss_sqdiff_kernel": [C(sqdiff, 4), C(sqdiff, 2 * 256 * 3 * 5), C(sqdiff, 1024 * 1024 + 1024 * 4 * 3 + 8)],
    "ploss_absdiff_kernel": [C(absdiff, 1), C(absdiff, 3 * 7 * 9), C(absdiff, 1024 * 256 + 1024 * 3 + 5)],
    "ploss_finish_kernel": [C(finish, 1, 0), C(finish, 300, 7), C(finish, 1024, 1024)],
}


def cases():
    """[(kernel, index, case)] in ledger order: one GPU test each"""
    return [(name, i, c) for name, cs in LEDGER.items() for i, c in enumerate(cs)]


def launched_by(case):
    """the kernels a case is listed under: what its entry launches"""
    return {name for name, cs in LEDGER.items() if case in cs}
