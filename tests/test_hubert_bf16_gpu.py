"""The bf16 HuBERT engine on the MI355X: against the reference's fp32 fixtures at the reference-autocast bars
(tests/hubert_bf16_bars.py), against the CPU model of its contract (printed, not barred: two summation orders of one
contract differ by most of its distance to fp32), its behaviour on short and batched inputs, beside an fp32 handle, and
end to end through VideoStreamManager."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hubert_bf16_bars as bars
import hubert_bf16_model
import hubert_ref
from calipsync_amd import _lib, hubert
from gpu_util import dev

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def eng2():
    return hubert.HubertEngine(hubert_ref.recipe_state_dict(2), 2, precision="bf16")


@pytest.fixture(scope="module")
def eng24():
    return hubert.HubertEngine(hubert_ref.recipe_state_dict(24), 24, precision="bf16")


def engine_features(eng, wave_np):
    x = torch.from_numpy(hubert.normalize(wave_np))[None]

    def enc(chunks):
        out = eng(torch.cat(chunks).to(dev()))
        return [out[i].cpu() for i in range(len(chunks))]
    return hubert.chunked_features(x, enc)


def fixture_case(case, eng, fixture):
    g = np.load(os.path.join(GOLDEN, fixture))
    wave_np = hubert_ref.golden_wave(int(g["samples"]), int(g["seed"]))
    flat = engine_features(eng, wave_np).numpy().reshape(-1, 1024)
    x = torch.from_numpy(hubert.normalize(wave_np))[None, :hubert.CHUNK].to(dev())
    conv, l0 = eng(x, stage=1), eng(x, stage=2)
    assert conv.dtype == torch.float32 and l0.dtype == torch.float32
    bad = bars.check_case(case, bars.load(), g, flat, conv[0].cpu().numpy().reshape(-1), l0[0].cpu().numpy().reshape(-1))
    assert not bad, bad
    return wave_np


def test_engine_meets_the_reference_bars_24_layers(eng24):
    fixture_case("l24", eng24, "hubert_l24.npz")


def test_engine_meets_the_reference_bars_2_layers_and_differs_from_its_cpu_model_by(eng2):
    wave_np = fixture_case("l2", eng2, "hubert_l2.npz")
    # engine vs the CPU model of the same contract at taps 1-3 and at the output: recorded in DESIGN section 8b, not barred
    P = hubert.packed_tensors(hubert_ref.recipe_state_dict(2), 2)
    w = torch.from_numpy(hubert.normalize(wave_np))[None]
    taps = {}
    with torch.no_grad():
        model_out = hubert_bf16_model.forward(P, 2, w, taps)
        taps1 = {}
        hubert_bf16_model.forward(P, 2, w, taps1, n_layers=1)
    wd = w.to(dev())
    for name, got, ref in (("tap 1 (conv stack)", eng2(wd, stage=1), taps["conv"]), ("tap 2 (layer-0 input)", eng2(wd, stage=2), taps["layer0_in"]),
                           ("tap 3 after 1 layer", eng2(wd, stage=3, n_layers=1), taps1["after1"]),
                           ("tap 3 after 2 layers", eng2(wd, stage=3, n_layers=2), taps["after2"]), ("output", eng2(wd), model_out)):
        d = (got.cpu() - ref).abs()
        print(f"engine vs CPU model, {name}: max {float(d.max()):.3e} mean {float(d.mean()):.3e}")
        assert bool(torch.isfinite(got).all())


def test_stage_3_tap_includes_the_pending_delta(eng2):
    """The out-proj / FF2 result waits as a bf16 delta for the next LayerNorm kernel; the tap must not miss it: the final
    LayerNorm of the tap after all layers is the forward's output."""
    P = hubert.packed_tensors(hubert_ref.recipe_state_dict(2), 2)
    w = torch.from_numpy(hubert.normalize(hubert_ref.golden_wave(16000, 31)))[None].to(dev())
    out, tap = eng2(w).cpu(), eng2(w, stage=3, n_layers=2).cpu()
    ref = F.layer_norm(tap.double(), (1024,), torch.from_numpy(P["enc.ln.g"]).double(), torch.from_numpy(P["enc.ln.b"]).double(), 1e-5)
    assert (out.double() - ref).abs().max() <= 1e-4
    assert eng2(w, stage=3, n_layers=0).cpu().equal(eng2(w, stage=2).cpu())


@pytest.mark.parametrize("n", [400, 401, 720, 2000])
def test_short_waveforms_at_batch_2(eng2, n):
    P = hubert.packed_tensors(hubert_ref.recipe_state_dict(2), 2)
    w = torch.stack([torch.from_numpy(hubert.normalize(hubert_ref.golden_wave(n, s))) for s in (21, 22)])
    ref = hubert_ref.forward(P, 2, w)
    got = eng2(w.to(dev())).cpu()
    assert got.shape == ref.shape and got.shape[1] == hubert.tokens(n)
    bad = bars.check_rows(f"n={n}", got.numpy(), ref.numpy(), bars.load())
    assert not bad, bad


def test_batch_of_three_is_deterministic_and_meets_the_bars(eng2):
    P = hubert.packed_tensors(hubert_ref.recipe_state_dict(2), 2)
    w = torch.stack([torch.from_numpy(hubert.normalize(hubert_ref.golden_wave(16000, s))) for s in (31, 32, 33)])
    ref = hubert_ref.forward(P, 2, w)
    wd = w.to(dev())
    a, b = eng2(wd), eng2(wd)
    assert torch.equal(a, b)
    bad = bars.check_rows("batch of 3 x 1 s", a.cpu().numpy(), ref.numpy(), bars.load())
    for i in range(3):
        one = eng2(wd[i:i + 1])[0]
        bad += bars.check_rows(f"single {i}", one.cpu().numpy()[None], ref[i:i + 1].numpy(), bars.load())
        d = (one - a[i]).abs()
        print(f"batch of 3 vs single, row {i}: max {float(d.max()):.3e} mean {float(d.mean()):.3e} (not barred: the tile follows the batch)")
    assert not bad, bad


def test_fp32_handle_is_bit_equal_beside_a_bf16_handle():
    sd = hubert_ref.recipe_state_dict(2)
    w = torch.stack([torch.from_numpy(hubert.normalize(hubert_ref.golden_wave(16000, s))) for s in (31, 32)]).to(dev())
    e32 = hubert.HubertEngine(sd, 2)
    before = e32(w).clone()
    e16 = hubert.HubertEngine(sd, 2, precision="bf16")
    mid = e32(w).clone()
    o16 = e16(w).clone()
    after = e32(w).clone()
    torch.cuda.synchronize()
    assert torch.equal(before, mid) and torch.equal(before, after)
    assert not torch.equal(o16, before) and float((o16 - before).abs().max()) < 0.2
    assert torch.equal(e16(w), o16)
    lib = _lib.load()
    b32, b16 = lib.casync_hubert_workspace_bytes_h(e32._h, 2, 16000), lib.casync_hubert_workspace_bytes_h(e16._h, 2, 16000)
    assert b32 == lib.casync_hubert_workspace_bytes(2, 16000) and 0 < b16 < b32


def test_a_workspace_that_is_too_small_is_an_error_status(eng2):
    lib = _lib.load()
    w = torch.from_numpy(hubert.normalize(hubert_ref.golden_wave(16000, 31)))[None].to(dev())
    need = lib.casync_hubert_workspace_bytes_h(eng2._h, 1, 16000)
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    out = torch.full((1, hubert.tokens(16000), 1024), 7.0, device=dev())
    strm = torch.cuda.current_stream().cuda_stream
    st = lib.casync_hubert_forward(eng2._h, w.data_ptr(), 1, 16000, out.data_ptr(), ws.data_ptr(), need - 1, strm)
    assert st < 0 and b"workspace" in lib.casync_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert lib.casync_hubert_forward(eng2._h, w.data_ptr(), 1, 16000, out.data_ptr(), ws.data_ptr(), need, strm) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, eng2(w))


def test_video_stream_manager_with_bf16_features(tmp_path):
    """VideoStreamManager(hubert_precision="bf16") from a checkpoint directory and a WAV: as many frames as the fp32 run;
    the mean absolute pixel difference between the two is printed (recorded in DESIGN, not barred)."""
    from test_hubert import write_checkpoint
    from frame_data import write_dataset
    from calipsync_amd import mjpeg_avi, recipe
    from calipsync_amd.frame_synth import VideoStreamManager
    from calipsync_amd.unet import Model
    net = Model(6, "hubert").to("cuda:0")
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe.make_state_dict().items()})
    net.eval()
    ckpt = write_checkpoint(str(tmp_path / "hubert"), 2)
    data = tmp_path / "data"
    write_dataset(str(data), 6, 270, 360, seed=4)
    x = (hubert_ref.golden_wave(16000, 41) * 32767).astype("<i2")
    wav = str(tmp_path / "a.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(x.tobytes())
    outs = {}
    for prec in ("fp32", "bf16"):
        vsm = VideoStreamManager(str(data), None, hubert_path=ckpt, device="cuda:0", batch_size=4, seed=9, net=net, hubert_precision=prec)
        outs[prec] = vsm.process_single_file(wav, str(tmp_path / f"{prec}.mp4"))
    f32 = hubert.HubertExtractor(ckpt).extract_from_file(wav)
    f16 = hubert.HubertExtractor(ckpt, precision="bf16").extract_from_file(wav)
    assert f32.shape == f16.shape == (24, 2, 1024)
    print(f"features bf16 vs fp32: max {np.abs(f16 - f32).max():.3e} mean {np.abs(f16 - f32).mean():.3e}")
    if outs["fp32"].endswith(".avi"):
        fa, fb = mjpeg_avi.read_mjpeg_avi(outs["fp32"])[1], mjpeg_avi.read_mjpeg_avi(outs["bf16"])[1]
        assert len(fa) == len(fb) == 24
        diff = np.mean([np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).mean() for a, b in zip(fa, fb)])
        print(f"frames bf16 vs fp32 features: mean absolute pixel difference {diff:.4f} of 255")
    else:
        assert os.path.getsize(outs["fp32"]) > 0 and os.path.getsize(outs["bf16"]) > 0
