"""mode='wenet' (AudioConvWenet, reference module/unet.py:109-144) on the host side, no GPU: the 577-key manifest, the
packed layout the engine and the packer agree on, the BatchNorm fold of conv3, and the CPU forward of tests/wenet_ref.py
against the reference's own numbers (tests/golden/unet_wenet_b2.npz, tests/golden/make_wenet_golden.py)."""
import os

import numpy as np
import pytest
import torch

from calipsync_amd import _lib, arch, pack, recipe
from calipsync_amd.unet import Model, WenetModel
from conftest import GOLDEN, sample_indices

import wenet_ref


@pytest.fixture(scope="module")
def golden_w():
    return np.load(os.path.join(GOLDEN, "unet_wenet_b2.npz"))


@pytest.fixture(scope="module")
def sd_w():
    return recipe.make_state_dict(mode="wenet")


def test_manifest_matches_the_reference_state_dict():
    with open(os.path.join(GOLDEN, "state_dict_manifest_wenet.txt")) as f:
        rows = [ln.split(" ", 1) for ln in f.read().splitlines()]
    ours = arch.manifest("wenet")
    assert len(rows) == len(ours) == 577
    for (key, rest), (k, shape, dtype, _role) in zip(rows, ours):
        assert key == k
        assert rest == f"{tuple(shape)} {dtype}"


def test_parameter_count(golden_w):
    n = sum(int(np.prod(s)) if s else 1 for _k, s, _d, role in arch.manifest("wenet")
            if role not in ("bn_mean", "bn_var", "bn_count"))
    assert n == 20_592_849 == int(golden_w["n_parameters"][0])


def test_no_bn7_and_hubert_unchanged():
    keys = [k for k, *_ in arch.manifest("wenet")]
    assert not any(k.startswith("audio_model.bn7") for k in keys)
    hub = [k for k, *_ in arch.manifest()]
    assert len(hub) == 582 and [k for k in hub if not k.startswith("audio_model.bn7")] == keys
    assert arch.manifest() == arch.manifest("hubert")
    with pytest.raises(ValueError):
        arch.manifest("conformer")


def test_python_and_c_layouts_agree(sd_w):
    items, total = _lib.packed_layout("wenet")
    names = [n for n, _o, _s in items]
    assert "audio_model.bn7.s" not in names and "audio_model.bn7.t" not in names
    sizes = dict((n, s) for n, _o, s in items)
    assert sizes["audio_model.conv3.w"] == 256 * 9 * 256
    assert sizes["audio_model.conv1.pw1.w"] == 512 * 256 and sizes["audio_model.conv2.pw2.w"] == 256 * 512
    folded = pack.fold(sd_w, "wenet")
    assert set(folded) == set(names)
    for n, _o, s in items:
        assert folded[n].size == s, n
    buf = pack.pack(sd_w, mode="wenet")
    assert buf.shape == (total,) and np.isfinite(buf).all()
    # the HuBERT layout through the new per-mode entries is the old one
    assert _lib.packed_layout("hubert") == _lib.packed_layout()
    lib = _lib.load()
    assert lib.casync_packed_count_m(0) == lib.casync_packed_count() and lib.casync_packed_total_m(0) == lib.casync_packed_total()
    assert lib.casync_packed_count_m(7) == 0 and lib.casync_packed_total_m(7) == -1


def test_fold_of_conv3_is_exact(sd_w):
    """conv3 + bias + bn3, folded in float64, reproduces the unfolded (1, 2)-strided conv + BN."""
    f = pack.fold(sd_w, "wenet")
    w = f["audio_model.conv3.w"].reshape(256, 3, 3, 256).transpose(0, 3, 1, 2)   # [N][(ky,kx,cin)] -> OIHW
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((1, 256, 16, 32)))
    got = torch.nn.functional.conv2d(x, torch.from_numpy(w.copy()), torch.from_numpy(f["audio_model.conv3.b"]), (1, 2), 1)
    sd = {k: torch.from_numpy(v.astype(np.float64)) for k, v in sd_w.items() if v.dtype != np.int64}
    ref = torch.nn.functional.conv2d(x, sd["audio_model.conv3.weight"], sd["audio_model.conv3.bias"], (1, 2), 1)
    ref = torch.nn.functional.batch_norm(ref, sd["audio_model.bn3.running_mean"], sd["audio_model.bn3.running_var"],
                                         sd["audio_model.bn3.weight"], sd["audio_model.bn3.bias"], False, 0.0, arch.BN_EPS)
    assert got.shape == (1, 256, 16, 16)
    assert float((got - ref).abs().max()) < 1e-10


def test_recipe_makes_relu_matter(golden_w):
    """A clear share of the conv3 / conv5 pre-activations is negative: a LeakyReLU in place of the ReLU shows at 1e-3."""
    neg3, neg5 = golden_w["negative_preact"]
    assert neg3 > 0.3 and neg5 > 0.3


def test_recipe_wenet_inputs():
    x, a = recipe.make_inputs(2, mode="wenet")
    assert x.shape == (2, 6, 160, 160) and a.shape == (2, 256, 16, 32)
    x2, _ = recipe.make_inputs(2)
    assert np.array_equal(x, x2)


def test_wenet_ref_reproduces_the_reference(golden_w, sd_w):
    x, a = recipe.make_inputs(2, mode="wenet")
    taps = {}
    out = wenet_ref.forward({k: torch.from_numpy(v.copy()) for k, v in sd_w.items()}, torch.from_numpy(x),
                            torch.from_numpy(a), taps)
    assert float(np.abs(out.numpy()[0] - golden_w["out.frame0"]).max()) <= 1e-5
    for name in ("out", "audio_conv1", "audio_conv2", "audio_conv3", "audio_conv4", "audio_conv5", "a", "tx", "kx", "fuse", "u4"):
        t = taps[name].numpy()
        assert tuple(golden_w[f"{name}.shape"]) == t.shape, name
        ref = golden_w[f"{name}.samples"]
        got = t.reshape(-1)[sample_indices(t.size)]
        assert np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max())) <= 1e-5, name
    assert (taps["audio_conv3"] == 0).float().mean() > 0.3     # ReLU: exact zeros


def test_model_wenet_constructs_and_loads_strictly(sd_w):
    m = WenetModel(6)
    assert m.mode == "wenet" and len(m.state_dict()) == 577
    res = m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_w.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    with pytest.raises(RuntimeError):     # a HuBERT checkpoint is not a wenet one
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe.make_state_dict().items()}, strict=True)
    buf = m.packed_weights_host()
    assert buf.shape == (_lib.packed_layout("wenet")[1],)
    assert WenetModel(6, "wenet", precision="bf16").precision == "bf16"
    for bad in ("conformer", "hubert"):
        with pytest.raises(NotImplementedError):
            WenetModel(6, bad)


def test_bad_audio_shape_is_rejected():
    m = WenetModel(6)
    x = torch.zeros(1, 6, 160, 160)
    with pytest.raises(RuntimeError, match="256,16,32"):
        m._check_inputs(x, torch.zeros(1, 32, 32, 32))
    h = Model(6, "hubert")
    with pytest.raises(RuntimeError, match="32,32,32"):
        h._check_inputs(x, torch.zeros(1, 256, 16, 32))



def test_model_stays_hubert_only():
    """``Model`` keeps its contract (any mode but 'hubert' raises); its error names the class that takes WeNet checkpoints."""
    with pytest.raises(NotImplementedError, match="WenetModel"):
        Model(6, "wenet")
    assert isinstance(WenetModel(6), Model) and Model(6).mode == "hubert"
