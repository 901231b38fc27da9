"""HuBERT feature extractor on the MI355X: the engine against the reference's fixtures, against the CPU
restatement, each new kernel through its op entry against float64 torch, determinism, and the offline driver
end to end from a checkpoint directory and a WAV file."""
import os
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hubert_ref
from calipsync_amd import _lib, hubert
from gpu_util import dev, ok, ptr, stream

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


@pytest.fixture(scope="module")
def eng2():
    return hubert.HubertEngine(hubert_ref.recipe_state_dict(2), 2)


@pytest.fixture(scope="module")
def eng24():
    return hubert.HubertEngine(hubert_ref.recipe_state_dict(24), 24)


def engine_features(eng, wave_np):
    x = torch.from_numpy(hubert.normalize(wave_np))[None]

    def enc(chunks):
        out = eng(torch.cat(chunks).to(dev()))
        return [out[i].cpu() for i in range(len(chunks))]
    return hubert.chunked_features(x, enc)


def test_engine_matches_reference_24_layers(eng24):
    g = golden("hubert_l24.npz")
    wave_np = hubert_ref.golden_wave(int(g["samples"]), int(g["seed"]))
    flat = engine_features(eng24, wave_np).numpy().reshape(-1, 1024)
    assert flat.shape[0] * 1024 == int(np.prod(g["out_shape"]))
    d_rows = np.abs(flat[g["rows"]] - g["row_val"])
    d_val = np.abs(flat.reshape(-1)[g["idx"]] - g["val"])
    print(f"24 layers vs reference: rows max {d_rows.max():.3e} mean {d_rows.mean():.3e}; strided max {d_val.max():.3e} "
          f"mean {d_val.mean():.3e}")
    assert max(d_rows.max(), d_val.max()) <= 1e-3 and max(d_rows.mean(), d_val.mean()) <= 1e-4
    assert np.abs(np.linalg.norm(flat.astype(np.float64), axis=1) - g["norms"]).max() <= 1e-2
    # debug intermediates of chunk 0
    x = torch.from_numpy(hubert.normalize(wave_np))[None, :hubert.CHUNK].to(dev())
    conv = eng24(x, stage=1)[0].cpu().numpy().reshape(-1)
    l0 = eng24(x, stage=2)[0].cpu().numpy().reshape(-1)
    dc, dl = np.abs(conv[g["conv_idx"]] - g["conv_val"]), np.abs(l0[g["l0_idx"]] - g["l0_val"])
    print(f"conv stack max {dc.max():.3e} mean {dc.mean():.3e}; layer-0 input max {dl.max():.3e} mean {dl.mean():.3e}")
    assert dc.max() <= 1e-3 and dc.mean() <= 1e-4 and dl.max() <= 1e-3 and dl.mean() <= 1e-4


def test_engine_matches_reference_2_layers(eng2):
    g = golden("hubert_l2.npz")
    wave_np = hubert_ref.golden_wave(int(g["samples"]), int(g["seed"]))
    got = engine_features(eng2, wave_np).numpy()
    d = np.abs(got - g["out"])
    print(f"2 layers vs reference: max {d.max():.3e} mean {d.mean():.3e}")
    assert d.max() <= 1e-3 and d.mean() <= 1e-4
    x = torch.from_numpy(hubert.normalize(wave_np))[None].to(dev())
    conv = eng2(x, stage=1)[0].cpu().numpy().reshape(-1)
    l0 = eng2(x, stage=2)[0].cpu().numpy().reshape(-1)
    assert np.abs(conv[g["conv_idx"]] - g["conv_val"]).max() <= 1e-3
    assert np.abs(l0[g["l0_idx"]] - g["l0_val"]).max() <= 1e-3


@pytest.mark.parametrize("n", [400, 401, 720, 2000])
def test_engine_matches_restatement_at_batch_2_and_short_tails(eng2, n):
    P = hubert.packed_tensors(hubert_ref.recipe_state_dict(2), 2)
    w = torch.stack([torch.from_numpy(hubert.normalize(hubert_ref.golden_wave(n, s))) for s in (21, 22)])
    taps = {}
    ref = hubert_ref.forward(P, 2, w, taps, n_layers=1)
    ref_full = hubert_ref.forward(P, 2, w)
    got = eng2(w.to(dev())).cpu()
    assert got.shape == ref_full.shape
    assert (got - ref_full).abs().max() <= 1e-3
    assert (eng2(w.to(dev()), stage=3, n_layers=1).cpu() - ref).abs().max() <= 1e-3


def test_forward_is_deterministic_and_batching_agrees(eng2):
    w = torch.stack([torch.from_numpy(hubert.normalize(hubert_ref.golden_wave(16000, s))) for s in (31, 32, 33)]).to(dev())
    a, b = eng2(w), eng2(w)
    assert torch.equal(a, b)
    for i in range(3):
        assert (eng2(w[i:i + 1])[0] - a[i]).abs().max() <= 1e-4


def test_op_layernorm():
    g = torch.randn(1024, dtype=torch.float64)
    be = torch.randn(1024, dtype=torch.float64)
    for cols in (512, 1024):
        for gelu in (0, 1):
            x = torch.randn(37, cols, dtype=torch.float64) * 3 + 1
            out = torch.empty(37, cols, device=dev())
            xd, gd, bd = (t.float().contiguous().to(dev()) for t in (x, g[:cols], be[:cols]))   # (held: the kernel reads them later)
            ok(_lib.load().casync_op_hubert_layernorm(ptr(xd), cols, ptr(out), cols, 37, cols, ptr(gd), ptr(bd), 1e-5, gelu, stream()))
            ref = F.layer_norm(x.float().double(), (cols,), g[:cols].float().double(), be[:cols].float().double(), 1e-5)
            ref = F.gelu(ref) if gelu else ref
            assert (out.cpu().double() - ref).abs().max() <= 1e-4, (cols, gelu)


@pytest.mark.parametrize("T", [1, 31, 100, 1000, 1001])
def test_op_attention(T):
    B = 2
    qkv = torch.randn(B * T, 3072, dtype=torch.float64)
    qkv[:, :1024] *= 0.5
    out = torch.empty(B * T, 1024, device=dev())
    qd = qkv.float().to(dev())
    ok(_lib.load().casync_op_hubert_attention(ptr(qd), ptr(out), B, T, stream()))
    q, k, v = (z.reshape(B, T, 16, 64).transpose(1, 2) for z in qkv.float().double().split(1024, dim=1))
    ref = (torch.softmax(q @ k.transpose(-1, -2), -1) @ v).transpose(1, 2).reshape(B * T, 1024)
    assert (out.cpu().double() - ref).abs().max() <= 1e-4


@pytest.mark.parametrize("T", [1, 50, 300])
def test_op_posconv(T):
    B = 2
    x = torch.randn(B, T, 1024, dtype=torch.float64)
    W = torch.randn(1024, 64, 128, dtype=torch.float64) / 90.0
    b = torch.randn(1024, dtype=torch.float64) * 0.1
    wp = W.float().reshape(16, 64, 64, 128).permute(0, 3, 1, 2).contiguous()
    out = torch.empty(B * T, 1024, device=dev())
    xd, wd, bd = x.float().to(dev()), wp.to(dev()), b.float().to(dev())
    ok(_lib.load().casync_op_hubert_posconv(ptr(xd), ptr(wd), ptr(bd), ptr(out), B, T, stream()))
    xf, Wf, bf = x.float().double(), W.float().double(), b.float().double()
    pc = F.conv1d(xf.transpose(1, 2), Wf, bf, padding=64, groups=16)[:, :, :-1]
    ref = (xf + F.gelu(pc).transpose(1, 2)).reshape(B * T, 1024)
    assert (out.cpu().double() - ref).abs().max() <= 1e-4


@pytest.mark.parametrize("tin,k,act,res", [(31, 3, 0, False), (1000, 3, 0, False), (401, 2, 0, False), (77, 3, 3, True)])
def test_op_rows_gemm_overlapping_rows(tin, k, act, res):
    """A channels-last conv (stride 2, kernel k, 512 channels) as a GEMM whose A rows overlap: lda = 1024 < K = 512 k."""
    x = torch.randn(tin, 512, dtype=torch.float64)
    W = torch.randn(512, 512, k, dtype=torch.float64) / np.sqrt(512 * k)
    b = torch.randn(512, dtype=torch.float64)
    tout = (tin - k) // 2 + 1
    r = torch.randn(tout, 512, dtype=torch.float64)
    wk = W.float().permute(0, 2, 1).reshape(512, k * 512).contiguous().to(dev())
    xd, rd, bd = x.float().to(dev()), r.float().to(dev()), b.float().to(dev())
    out = torch.empty(tout, 512, device=dev())
    ok(_lib.load().casync_op_rows_gemm(ptr(xd), 1024, ptr(wk), ptr(bd), ptr(out), 512, tout, 512, 512 * k, act,
                                       ptr(rd) if res else 0, 512 if res else 0, stream()))
    ref = F.conv1d(x.float().double().t()[None], W.float().double(), b.float().double(), stride=2)[0].t()
    ref = F.gelu(ref) if act == 3 else ref
    ref = ref + r.float().double() if res else ref
    assert (out.cpu().double() - ref).abs().max() <= 1e-4


def test_op_conv0():
    S, B = 2005, 2
    x = torch.randn(B, S, dtype=torch.float64)
    W = torch.randn(512, 1, 10, dtype=torch.float64) / 3
    b, g, be = (torch.randn(512, dtype=torch.float64) for _ in range(3))
    T0 = (S - 10) // 5 + 1
    out = torch.empty(B * T0, 512, device=dev())
    d = [t.float().contiguous().to(dev()) for t in (x, W.reshape(512, 10), b, g, be)]
    ok(_lib.load().casync_op_hubert_conv0(ptr(d[0]), B, S, ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), ptr(out), stream()))
    y = F.conv1d(x.float().double()[:, None], W.float().double(), b.float().double(), stride=5).transpose(1, 2)
    ref = F.gelu(F.layer_norm(y, (512,), g.float().double(), be.float().double(), 1e-5)).reshape(B * T0, 512)
    assert (out.cpu().double() - ref).abs().max() <= 1e-4


def test_video_stream_manager_takes_a_checkpoint_directory(tmp_path):
    """VideoStreamManager(data, None, hubert_path=<checkpoint dir>) extracts the features of a WAV on the engine; the
    frames equal those of the same features passed as .npy."""
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
    vsm = VideoStreamManager(str(data), None, hubert_path=ckpt, device="cuda:0", batch_size=4, seed=9, net=net)
    out_a = vsm.process_single_file(wav, str(tmp_path / "a.mp4"))
    feats = hubert.HubertExtractor(ckpt).extract_from_file(wav)
    assert feats.shape == (24, 2, 1024)
    np.save(str(tmp_path / "f.npy"), feats)
    vsm2 = VideoStreamManager(str(data), None, device="cuda:0", batch_size=4, seed=9, net=net)
    out_b = vsm2.process_single_file(str(tmp_path / "f.npy"), str(tmp_path / "b.mp4"))
    if out_a.endswith(".avi"):
        fa, fb = mjpeg_avi.read_mjpeg_avi(out_a)[1], mjpeg_avi.read_mjpeg_avi(out_b)[1]
        assert len(fa) == len(fb) == 24 and all(np.array_equal(a, b) for a, b in zip(fa, fb))
    else:
        assert os.path.getsize(out_a) > 0 and os.path.getsize(out_b) > 0
