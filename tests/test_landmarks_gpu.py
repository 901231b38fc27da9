"""-m gpu: the PFLD_GhostOne landmark engine end to end.  The bar everywhere is 4 x ref_err, the reference's own float32
error against float64 on the same data: the 4 covers another summation order (six branches folded into one kernel, MFMA
trees in place of serial sums) and taking the maximum over 17 comparisons.  The first test prints the measured ratios."""
import os

import numpy as np
import pytest
import torch

import pfld_ref
from calipsync_amd import landmarks, recipe
from conftest import GOLDEN, sample_indices

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def sd():
    return recipe.make_pfld_state_dict()


@pytest.fixture(scope="module")
def eng(sd):
    return landmarks.PFLDEngine(sd, DEV)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "pfld_b3.npz"))


@pytest.fixture(scope="module")
def u8():
    return recipe.make_pfld_inputs(5)


def _float(u8):
    return torch.from_numpy((np.asarray(u8, dtype=np.float32) / 255.0).transpose(0, 3, 1, 2).copy())


@pytest.fixture(scope="module")
def restated(sd):
    """pfld_ref in float64 and float32 on B = 5 crops and on one other crop: computed once, shared, never changed"""
    out = {}
    for name, crops in (("b5", recipe.make_pfld_inputs(5)), ("b1", recipe.make_pfld_inputs(1, seed=recipe.PFLD_INPUT_SEED + 100))):
        x = _float(crops)
        y64, _ = pfld_ref.forward(landmarks.fold(sd, dtype=np.float64), x.double())
        y32, _ = pfld_ref.forward(landmarks.fold(sd), x)
        out[name] = (crops, y64.numpy(), float((y32.double() - y64).abs().max()))
    return out


def test_fixture_output_and_every_tap_within_four_reference_errors(eng, fx):
    crops = recipe.make_pfld_inputs(3)
    y = eng.forward_u8(crops).cpu().numpy().astype(np.float64)
    ratios = {"out": np.abs(y - fx["out64"]).max() / float(fx["ref_err.out"])}
    for name, (h, w, c) in zip(landmarks.STAGES, landmarks.STAGE_SHAPES):
        t = eng.forward_u8(crops, stage=name)
        assert tuple(t.shape) == ((3, c) if name == "conv_out" else (3, h, w, c))      # (the last tap is the [B,220] output)
        t = t.reshape(3, h, w, c)
        flat = t.permute(0, 3, 1, 2).contiguous().cpu().numpy().reshape(-1).astype(np.float64)     # the fixture samples NCHW
        assert tuple(fx[f"{name}.shape"]) == (3, c, h, w)
        d = np.abs(flat[sample_indices(flat.size)] - fx[f"{name}.samples"]).max()
        ratios[name] = d / float(fx[f"ref_err.{name}"])
    for k, v in ratios.items():
        print(f"{k:9s} max|engine - fp64| / ref_err = {v:.3f}")
    bad = {k: round(v, 3) for k, v in ratios.items() if not v <= 4.0}
    assert not bad, bad
    # the last tap is the output itself
    assert torch.equal(eng.forward_u8(crops, stage="conv_out").reshape(3, 220), eng.forward_u8(crops))


def test_float_and_uint8_inputs_agree_bit_for_bit(eng, u8):
    assert torch.equal(eng.forward(_float(u8)), eng.forward_u8(u8))


def test_two_runs_are_bit_equal(eng, u8):
    a = eng.forward_u8(u8).clone()
    for _ in range(2):
        assert torch.equal(eng.forward_u8(u8), a)


def test_a_frame_of_a_batch_equals_the_frame_alone(eng, u8):
    whole = eng.forward_u8(u8).clone()
    for i in range(5):
        assert torch.equal(eng.forward_u8(u8[i:i + 1])[0], whole[i]), i
    deep = eng.forward_u8(u8, stage="conv5_4").clone()
    assert torch.equal(eng.forward_u8(u8[3:4], stage="conv5_4")[0], deep[3])


@pytest.mark.parametrize("which", ["b1", "b5"])
def test_other_batches_match_the_restatement(eng, restated, which):
    crops, y64, ref_err = restated[which]
    d = np.abs(eng.forward_u8(crops).cpu().numpy().astype(np.float64) - y64).max()
    print(f"{which}: max|engine - fp64| {d:.3e}, ref_err {ref_err:.3e}, ratio {d / ref_err:.3f}")
    assert d <= 4.0 * ref_err


@pytest.mark.parametrize("b", [1, 3])
def test_exact_workspace_suffices_and_nothing_is_written_past_the_output(eng, u8, b):
    need = eng.workspace_bytes(b)
    assert need % 4 == 0
    pad = 4096
    ws = torch.full((need // 4 + pad,), -7.0, device=DEV)
    out = torch.full((b * 220 + pad,), -7.0, device=DEV)
    want = eng.forward_u8(u8[:b]).clone()
    eng.forward_u8(u8[:b], out=out, workspace=ws[:need // 4])
    assert torch.equal(out[:b * 220].reshape(b, 220), want)
    assert bool((out[b * 220:] == -7.0).all()) and bool((ws[need // 4:] == -7.0).all())
    with pytest.raises(RuntimeError, match="workspace"):
        eng.forward_u8(u8[:b], workspace=ws[:need // 4 - 64])


def test_landmark_integers_match_the_reference(eng, fx, sd):
    det = landmarks.LandmarkDetector.__new__(landmarks.LandmarkDetector)
    det.mean_face, det.face_detector, det.pfld_backbone = fx["mean_face"], None, eng
    sizes, offsets = [tuple(int(v) for v in s) for s in fx["sizes"]], [tuple(int(v) for v in o) for o in fx["offsets"]]
    got = np.stack(det.landmarks_from_crops(recipe.make_pfld_inputs(3), sizes, offsets))
    assert got.shape == (3, 110, 2) and got.dtype == np.int32
    v64 = (fx["out64"] + fx["mean_face"].astype(np.float64)).reshape(3, -1, 2) * fx["sizes"].astype(np.float64)[:, None, :] \
        + fx["offsets"].astype(np.float64)[:, None, :]
    delta = 4.0 * float(fx["ref_err.out"]) * fx["sizes"].astype(np.float64)[:, None, :]
    near = np.abs(v64 - np.round(v64)) <= delta
    assert near.mean() <= 0.02, f"{int(near.sum())} of {near.size} coordinates lie within the float bar of an integer"
    assert np.array_equal(got[~near], fx["landmarks"][~near])
    assert np.abs(got[near] - fx["landmarks"][near]).max(initial=0) <= 1


def test_a_unet_forward_after_a_pfld_forward_is_still_right(eng, u8, recipe_sd, golden):
    from calipsync_amd.unet import Model
    net = Model(6, "hubert").to(DEV)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe_sd.items()})
    net.eval()
    x, a = recipe.make_inputs(2)
    xd, ad = torch.from_numpy(x).to(DEV), torch.from_numpy(a).to(DEV)
    want = eng.forward_u8(u8).clone()
    alone = net(xd, ad).clone()
    y = eng.forward_u8(u8)
    out = net(xd, ad)
    y2 = eng.forward_u8(u8)
    torch.cuda.synchronize()
    assert torch.equal(y, want) and torch.equal(y2, want)
    assert np.abs(out.cpu().numpy() - golden["out.full"]).max() < 1e-3
    assert torch.equal(out, alone)
