"""-m gpu: the SyncNet_color engine end to end.  The bar everywhere is 4 x ref_err, the reference's own float32 error against
float64 on the same data (tests/golden/make_syncnet_golden.py): the engine may be as wrong as the reference is, with room for
another summation order (MFMA k-order in place of the host's) and the maximum over 33 comparisons.  The fixture test prints
the measured ratios."""
import os

import numpy as np
import pytest
import torch

from calipsync_amd import frame_loop, recipe, syncnet
from conftest import GOLDEN, sample_indices

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = {"hubert": 3, "wenet": 2}


@pytest.fixture(scope="module")
def nets():
    return {m: syncnet.SyncNetColor(m, DEV, recipe.make_syncnet_state_dict(m)) for m in CASES}


@pytest.fixture(scope="module")
def pairs():
    """B = 5 hubert pairs on the device: made once, shared, never changed"""
    x, a = recipe.make_syncnet_inputs(5, "hubert")
    return torch.from_numpy(x).to(DEV), torch.from_numpy(a).to(DEV)


def _fx(mode):
    return np.load(os.path.join(GOLDEN, f"syncnet_{mode}_b{CASES[mode]}.npz"))


@pytest.mark.parametrize("mode", list(CASES))
def test_every_tap_and_both_embeddings_within_four_reference_errors(nets, mode):
    fx, b, net = _fx(mode), CASES[mode], nets[mode]
    x, a = (torch.from_numpy(v).to(DEV) for v in recipe.make_syncnet_inputs(b, mode))
    a_emb, f_emb = net(x, a)
    assert a_emb.shape == f_emb.shape == (b, syncnet.EMBED_DIM)
    ratios = {"audio_emb": np.abs(a_emb.cpu().numpy().astype(np.float64) - fx["audio_emb64"]).max() / float(fx["ref_err.audio_emb"]),
              "face_emb": np.abs(f_emb.cpu().numpy().astype(np.float64) - fx["face_emb64"]).max() / float(fx["ref_err.face_emb"])}
    for name, (c, h, w) in zip(syncnet.STAGES, syncnet.stage_shapes(mode)):
        t = net.engine.tap(name, x if name.startswith("face") else a)
        assert tuple(t.shape) == (b, c, h, w) == tuple(fx[f"{name}.shape"]), name
        flat = t.cpu().numpy().reshape(-1).astype(np.float64)                 # NCHW, as the fixture samples it
        d = np.abs(flat[sample_indices(flat.size)] - fx[f"{name}.samples"]).max()
        ratios[name] = d / float(fx[f"ref_err.{name}"])
        stats = np.array([flat.sum(), np.abs(flat).sum(), (flat * flat).sum(), flat.min(), flat.max()])
        bar = 4.0 * float(fx[f"ref_err.{name}"])
        # sums of n values each within the bar; the extremes within the bar; sum of squares: 2 |x| d
        top = max(abs(fx[f"{name}.stats"][3]), abs(fx[f"{name}.stats"][4]))
        tol = np.array([flat.size * bar, flat.size * bar, 2 * top * flat.size * bar, bar, bar])
        assert (np.abs(stats - fx[f"{name}.stats"]) <= tol).all(), (name, stats, fx[f"{name}.stats"])
    for k, v in ratios.items():
        print(f"{mode} {k:9s} max|engine - fp64| / ref_err = {v:.3f}")
    bad = {k: round(v, 3) for k, v in ratios.items() if not v <= 4.0}
    assert not bad, bad


@pytest.mark.parametrize("mode", list(CASES))
def test_similarity_matches_the_reference_cosines(nets, mode):
    fx, b = _fx(mode), CASES[mode]
    x, a = (torch.from_numpy(v).to(DEV) for v in recipe.make_syncnet_inputs(b, mode))
    cos = nets[mode].similarity(x, a)
    assert cos.shape == (b,) and cos.dtype == torch.float32
    d = np.abs(cos.cpu().numpy().astype(np.float64) - fx["cos64"]).max()
    print(f"{mode}: cos {cos.cpu().numpy()} max|engine - fp64| {d:.3e}, ref_err {float(fx['ref_err.cos']):.3e}")
    assert d <= 4.0 * float(fx["ref_err.cos"])
    # the cosine of a random face and a random window is about 0.33 and moves from pair to pair: mixed-up frames would show
    assert len(set(np.round(fx["cos64"], 4))) == b


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
    deep = net.engine.tap("face.13", x[:3].contiguous()).clone()
    assert torch.equal(net.engine.tap("face.13", x[1:2])[0], deep[1])


def test_a_batch_above_256_runs_in_passes_with_the_same_bits(nets, pairs):
    """257 frames: a pass of 256 and a pass of one, each frame with the bits of the B = 5 forward"""
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


def test_a_model_output_is_scored_where_it_lies(nets, pairs, recipe_sd):
    from calipsync_amd.unet import Model
    unet = Model(6, "hubert").to(DEV)
    unet.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe_sd.items()})
    unet.eval()
    x6, a = (torch.from_numpy(v).to(DEV) for v in recipe.make_inputs(2))
    pred = unet(x6, a)
    got = nets["hubert"](pred, a)
    want = nets["hubert"](pred.clone().contiguous(), a.clone())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool(torch.isfinite(got[1]).all())


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
        net(x.double(), a)
    with pytest.raises(ValueError, match="float32"):
        net(x.cpu(), a)
    with pytest.raises(ValueError, match="audio_sequences"):
        nets["wenet"](x, a)                                    # a hubert-shaped window into the wenet network


def test_score_clip_equals_the_curve_of_hand_gathered_windows(nets, pairs):
    net = nets["hubert"]
    x, _ = pairs
    faces = torch.cat([x, x[:1].flip(3)]).contiguous()       # 6 frames
    feats = np.stack([recipe.normal01(recipe.SYNCNET_INPUT_SEED, 0x9000000 + t, 2048).astype(np.float32).reshape(2, 1024)
                      for t in range(11)])
    idx = [0, 1, 2, 3, 4, 5]
    got = net.score_clip(faces, torch.from_numpy(feats).to(DEV), idx, 2)
    windows = torch.from_numpy(frame_loop.audio_windows_host(feats, idx)).to(DEV)
    want = net.offset_curve(faces, windows, 2)
    assert got.sim.shape == (5, 6) and torch.equal(got.sim, want.sim) and torch.equal(got.curve, want.curve)
    assert got.curve.dtype == torch.float64 and got.counts.tolist() == [4, 5, 6, 5, 4] and got.best_shift == want.best_shift
    sim = got.sim.cpu()
    assert float(sim[0, 0]) == 0.0 and float(sim[0, 1]) == 0.0 and float(sim[4, 5]) == 0.0 and float(sim[4, 4]) == 0.0
    assert torch.allclose(got.curve.cpu(), sim.double().sum(1) / got.counts.double(), rtol=0, atol=1e-15)   # (another order of 6 adds)
    with pytest.raises(ValueError, match="hubert"):
        nets["wenet"].score_clip(faces, torch.from_numpy(feats).to(DEV), idx, 2)


def test_shifts_without_a_pair_count_zero_and_are_never_best(nets, pairs):
    net = nets["hubert"]
    x, a = pairs
    c = net.offset_curve(x[:2].contiguous(), a[:2].contiguous(), 3)
    assert c.counts.tolist() == [0, 0, 1, 2, 1, 0, 0] and c.sim.shape == (7, 2)
    curve = c.curve.cpu()
    assert curve[[0, 1, 5, 6]].tolist() == [0.0] * 4
    vals = {s: float(curve[s + 3]) for s in (-1, 0, 1)}
    assert c.best_shift in vals and vals[c.best_shift] == max(vals.values())


def test_exact_workspace_suffices_and_a_short_one_is_refused(nets, pairs):
    eng = nets["hubert"].engine
    x, a = pairs
    need = eng.workspace_bytes(2)
    assert need % 256 == 0 and need == eng.workspace_bytes(1) * 2
    pad = 4096
    ws = torch.full((need // 4 + pad,), -7.0, device=DEV)
    want = [t.clone() for t in eng.forward(x[:2], a[:2])]
    got = eng.forward(x[:2], a[:2], workspace=ws[:need // 4])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool((ws[need // 4:] == -7.0).all())
    with pytest.raises(RuntimeError, match="workspace"):
        eng.forward(x[:2], a[:2], workspace=ws[:need // 4 - 64])
