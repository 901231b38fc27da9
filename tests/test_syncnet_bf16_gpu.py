"""-m gpu: the bf16 precision of the SyncNet_color engine end to end.  Every tap and both embeddings stay within 2 x the max
and 1.25 x the mean of the reference's own bf16-autocast error against float64 (tests/golden/syncnet_bf16_bar.npz,
tests/syncnet_bf16_bars.py), the bars of the bf16 S3FD and U-Net; the fixture test prints the engine's ratios with those of the
equal-contract model (tests/syncnet_bf16_model.py) beside them.  The rest are the properties the fp32 handle is held to."""
import numpy as np
import pytest
import torch

import syncnet_bf16_bars as bars
import syncnet_bf16_model
from calipsync_amd import _lib, frame_loop, recipe, syncnet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = bars.CASES


@pytest.fixture(scope="module")
def nets():
    return {m: syncnet.SyncNetColor(m, DEV, recipe.make_syncnet_state_dict(m), precision="bf16") for m in CASES}


@pytest.fixture(scope="module")
def pairs():
    """B = 5 hubert pairs on the device: made once, shared, never changed"""
    x, a = recipe.make_syncnet_inputs(5, "hubert")
    return torch.from_numpy(x).to(DEV), torch.from_numpy(a).to(DEV)


@pytest.fixture(scope="module")
def model_ratios():
    """the equal-contract model's ratios to autocast on the fixtures' inputs (CPU, float64 sums): computed once"""
    out, bar = {}, bars.bars()
    for mode, b in CASES.items():
        x, a = (torch.from_numpy(v) for v in recipe.make_syncnet_inputs(b, mode))
        a_emb, f_emb, stages = syncnet_bf16_model.forward(syncnet.fold(recipe.make_syncnet_state_dict(mode), mode), x, a, mode)
        errs = bars.errors(mode, a_emb.numpy(), f_emb.numpy(), {k: v.numpy() for k, v in stages.items()}, bars.fixture(mode))
        out[mode] = bars.ratios(mode, errs, bar)
    return out


@pytest.mark.parametrize("mode", list(CASES))
def test_every_tap_and_both_embeddings_within_the_autocast_bars(nets, model_ratios, mode):
    fx, bar, b, net = bars.fixture(mode), bars.bars(), CASES[mode], nets[mode]
    assert net.precision == net.engine.precision == "bf16" and _lib.load().casync_syncnet_precision(net.engine._h) == 1
    x, a = (torch.from_numpy(v).to(DEV) for v in recipe.make_syncnet_inputs(b, mode))
    a_emb, f_emb = net(x, a)
    assert a_emb.shape == f_emb.shape == (b, syncnet.EMBED_DIM) and a_emb.dtype == f_emb.dtype == torch.float32
    taps = {}
    for name, (c, h, w) in zip(syncnet.STAGES, syncnet.stage_shapes(mode)):
        t = net.engine.tap(name, x if name.startswith("face") else a)
        assert tuple(t.shape) == (b, c, h, w) and t.dtype == torch.float32, name
        last = name in syncnet_bf16_model.LAST
        assert bool(torch.equal(t.bfloat16().float(), t)) != last, name          # bf16 values widened, but the two fp32 stores
        taps[name] = t.cpu().numpy()
    rat = bars.ratios(mode, bars.errors(mode, a_emb.cpu().numpy(), f_emb.cpu().numpy(), taps, fx), bar)
    for n, (mx, mean) in rat.items():
        mm, mn = model_ratios[mode][n]
        print(f"{mode} {n:9s} engine / autocast: max {mx:.3f} mean {mean:.3f}   model / autocast: max {mm:.3f} mean {mn:.3f}   "
              f"engine / model: max {mx / mm:.3f} mean {mean / mn:.3f}")
    assert not bars.failures(rat), bars.failures(rat)


@pytest.mark.parametrize("mode", list(CASES))
def test_similarity_within_twice_the_cosine_bound(nets, mode):
    fx, bar, b = bars.fixture(mode), bars.bars(), CASES[mode]
    x, a = (torch.from_numpy(v).to(DEV) for v in recipe.make_syncnet_inputs(b, mode))
    cos = nets[mode].similarity(x, a)
    assert cos.shape == (b,) and cos.dtype == torch.float32
    d = np.abs(cos.cpu().numpy().astype(np.float64) - fx["cos64"]).max()
    print(f"{mode}: cos {cos.cpu().numpy()} max|engine - fp64| {d:.3e}, bound {float(bar[f'{mode}.cos_bound']):.3e}, "
          f"autocast's own {float(bar[f'{mode}.cos_err']):.3e}")
    assert d <= 2.0 * float(bar[f"{mode}.cos_bound"])


def test_a_frame_of_a_batch_has_the_bits_of_the_frame_alone(nets, pairs):
    net = nets["hubert"]
    x, a = pairs
    a3, f3 = (t.clone() for t in net(x[:3].contiguous(), a[:3].contiguous()))
    for i in range(3):
        ai, fi = net(x[i:i + 1], a[i:i + 1])
        assert torch.equal(ai[0], a3[i]) and torch.equal(fi[0], f3[i]), i
    order = [0, 1, 2, 1, 0]
    a5, f5 = net(x[order].contiguous(), a[order].contiguous())
    for k, i in enumerate(order):
        assert torch.equal(a5[k], a3[i]) and torch.equal(f5[k], f3[i]), (k, i)
    for stage in ("face.13", "face.15", "audio.7", "audio.12"):           # wide and narrow tiles, both encoders
        src = x if stage.startswith("face") else a
        deep = net.engine.tap(stage, src[:3].contiguous()).clone()
        assert torch.equal(net.engine.tap(stage, src[1:2])[0], deep[1]), stage


def test_a_batch_above_256_runs_in_passes_with_the_same_bits(nets, pairs):
    """257 frames: a pass of 256 (64-channel tiles everywhere) and a pass of one (16-channel tiles in the tails), each frame with
    the bits of the B = 5 forward"""
    net = nets["hubert"]
    x, a = pairs
    a5, f5 = (t.clone() for t in net(x, a))
    idx = [i % 5 for i in range(257)]
    a257, f257 = net(x[idx].contiguous(), a[idx].contiguous())
    want = torch.tensor(idx, device=DEV)
    assert torch.equal(a257, a5[want]) and torch.equal(f257, f5[want])


def test_two_runs_are_bit_equal(nets, pairs):
    net = nets["hubert"]
    a0, f0 = (t.clone() for t in net(*pairs))
    a1, f1 = net(*pairs)
    assert torch.equal(a0, a1) and torch.equal(f0, f1)
    assert bool(torch.isfinite(a0).all() and torch.isfinite(f0).all())


def test_the_two_channel_tiles_return_the_same_bits():
    """casync_op_sync16_conv3 with 64 and with 16 channels per workgroup on one input: an output's bits do not depend on the tile"""
    lib = _lib.load()
    g = torch.Generator().manual_seed(16)
    b, h, w, cin, cout = 2, 5, 7, 64, 128
    x = torch.randn(b, h, w, cin, generator=g).bfloat16().to(DEV)
    wt = (torch.randn(cout, 9 * cin, generator=g) / 24).bfloat16().to(DEV)
    bias = torch.randn(cout, generator=g).to(DEV)
    outs = []
    for tile in (64, 16):
        out = torch.full((b * h * w, cout), -7.0, dtype=torch.bfloat16, device=DEV)
        _lib.check(lib.casync_op_sync16_conv3(x.data_ptr(), wt.data_ptr(), bias.data_ptr(), x.data_ptr() if cin == cout else None,
                                              out.data_ptr(), b, h, w, cin, cout, 1, 1, 1, tile, torch.cuda.current_stream().cuda_stream),
                   "sync16_conv3")
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and bool((outs[0] >= 0).all()) and bool((outs[0] > 0).any())
    with pytest.raises(RuntimeError, match="tile"):
        _lib.check(lib.casync_op_sync16_conv3(x.data_ptr(), wt.data_ptr(), bias.data_ptr(), None, outs[0].data_ptr(), b, h, w, cin, cout,
                                              1, 1, 1, 32, torch.cuda.current_stream().cuda_stream), "sync16_conv3")


def test_the_fp32_handle_keeps_its_bits_beside_a_bf16_handle(pairs):
    x, a = pairs
    sd = recipe.make_syncnet_state_dict("hubert")
    fp32 = syncnet.SyncNetColor("hubert", DEV, sd)
    assert fp32.precision == "fp32" and _lib.load().casync_syncnet_precision(fp32.engine._h) == 0
    before = [t.clone() for t in fp32(x[:2], a[:2])]
    tap_before = fp32.engine.tap("audio.9", a[:2]).clone()
    bf16 = syncnet.SyncNetColor("hubert", DEV, sd, precision="bf16")
    got16 = [t.clone() for t in bf16(x[:2], a[:2])]
    after = fp32(x[:2], a[:2])
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert torch.equal(fp32.engine.tap("audio.9", a[:2]), tap_before)
    assert not torch.equal(got16[0], before[0]) and not torch.equal(got16[1], before[1])      # another arithmetic


def test_offset_curve_and_score_clip_are_the_curve_of_the_handles_own_embeddings(nets, pairs):
    net = nets["hubert"]
    x, _ = pairs
    faces = torch.cat([x, x[:1].flip(3)]).contiguous()       # 6 frames
    feats = np.stack([recipe.normal01(recipe.SYNCNET_INPUT_SEED, 0x9000000 + t, 2048).astype(np.float32).reshape(2, 1024)
                      for t in range(11)])
    idx = [0, 1, 2, 3, 4, 5]
    windows = torch.from_numpy(frame_loop.audio_windows_host(feats, idx)).to(DEV)
    a_emb, f_emb = net(faces, windows)
    want = syncnet.curve_of(syncnet.shift_similarity(f_emb, a_emb, 2))
    for got in (net.offset_curve(faces, windows, 2), net.score_clip(faces, torch.from_numpy(feats).to(DEV), idx, 2)):
        assert got.sim.shape == (5, 6) and torch.equal(got.sim, want.sim) and torch.equal(got.curve, want.curve)
        assert got.curve.dtype == torch.float64 and got.counts.tolist() == [4, 5, 6, 5, 4] and got.best_shift == want.best_shift
    assert torch.equal(net.similarity(faces, windows), want.sim[2])
    with pytest.raises(ValueError, match="hubert"):
        nets["wenet"].score_clip(faces, torch.from_numpy(feats).to(DEV), idx, 2)


def test_exact_workspace_suffices_and_a_short_one_is_refused(nets, pairs):
    eng = nets["hubert"].engine
    x, a = pairs
    need = eng.workspace_bytes(2)
    assert need % 256 == 0 and need == eng.workspace_bytes(1) * 2 == 2 * 2 * 160 * 160 * 32 * 2
    pad = 4096
    ws = torch.full((need // 4 + pad,), -7.0, device=DEV)
    want = [t.clone() for t in eng.forward(x[:2], a[:2])]
    got = eng.forward(x[:2], a[:2], workspace=ws[:need // 4])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool((ws[need // 4:] == -7.0).all())
    with pytest.raises(RuntimeError, match="workspace"):
        eng.forward(x[:2], a[:2], workspace=ws[:need // 4 - 64])
    with pytest.raises(RuntimeError, match="workspace"):
        eng.tap("face.3", x[:2], workspace=ws[:need // 4 - 64])


def test_wrong_inputs_raise(nets, pairs):
    net = nets["hubert"]
    x, a = pairs
    with pytest.raises(ValueError, match="contiguous"):
        net(x.transpose(2, 3), a)
    with pytest.raises(ValueError, match="face_sequences"):
        net(x[:, :, :159], a)
    with pytest.raises(ValueError, match="face_sequences"):
        net(torch.zeros(5, 6, 160, 160, device=DEV), a)
    with pytest.raises(ValueError, match="audio windows"):
        net(x, a[:4])
    with pytest.raises(ValueError, match="float32"):
        net(x.bfloat16(), a)                                   # the bf16 handle still takes float32 inputs
    with pytest.raises(ValueError, match="float32"):
        net(x, a.double())
    with pytest.raises(ValueError, match="float32"):
        net(x.cpu(), a)
    with pytest.raises(ValueError, match="audio_sequences"):
        nets["wenet"](x, a)                                    # a hubert-shaped window into the wenet network
    with pytest.raises(ValueError, match="stage"):
        net.engine.tap(31, x)
