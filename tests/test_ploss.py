"""The loss handle without a GPU (include/casync_ploss.h, calipsync_amd/losses.py): the packed layout built from a vgg19-style
state dict, the key names, the refusal of any criterion but a mean-reduction MSELoss, the numpy twin of the weight transform,
saved / scratch sizes, and the library's exports against the header."""
import os
import re

import numpy as np
import pytest
import torch

import vgg_ref
from calipsync_amd import _lib, losses, recipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "casync_ploss.h")


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return [m.group(1) for m in re.finditer(r"\b(casync_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)]


def test_the_library_exports_what_the_header_declares():
    lib = _lib.load()                                     # loads without a GPU
    names = declared()
    assert len(names) == len(set(names)) == 28
    assert sorted(names) == sorted(_lib.EXPORTS_PLOSS)
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.casync_abi_version() == 13                 # additive: the ABI number stays
    main = open(os.path.join(ROOT, "include", "casync_hip.h")).read()
    assert "ploss" not in main
    assert sum(1 for n in names if n.startswith("casync_op_ploss_")) == 11         # one entry per kernel of csrc/ploss.hip


def test_the_restatement_has_the_vgg19_names():
    m = vgg_ref.Vgg19Features15()
    assert list(m.state_dict()) == [k for k, _ in losses.manifest()]
    assert [k for k, _ in losses.manifest()] == [f"features.{i}.{leaf}" for i in (0, 2, 5, 7, 10, 12, 14) for leaf in ("weight", "bias")]
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(losses.manifest())          # the module's table against ...
    chans = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256)]                # ... the numbers themselves
    assert [tuple(m.state_dict()[f"features.{i}.weight"].shape) for i in (0, 2, 5, 7, 10, 12, 14)] == [(co, ci, 3, 3) for ci, co in chans]
    assert [(ci, co) for _, _, ci, co in losses.VGG_CONVS] == chans
    assert len(m.features) == 15 and isinstance(m.features[14], torch.nn.Conv2d) and isinstance(m.features[13], torch.nn.ReLU)
    assert [i for i, layer in enumerate(m.features) if isinstance(layer, torch.nn.MaxPool2d)] == [4, 9]
    sd = recipe.make_vgg19_state_dict()
    assert list(sd) == [k for k, _ in losses.manifest()]
    assert all(np.array_equal(sd[k], recipe.make_vgg19_state_dict()[k]) for k in sd)     # seeded
    t = vgg_ref.model(sd).taps(torch.from_numpy(recipe.make_loss_inputs(1, 16, 16)[0]).double())
    tops = {k: float(v.abs().max()) for k, v in t.items()}
    assert all(0.5 < v < 8.0 for v in tops.values()), tops                               # O(1) through the seven convs


def test_the_packed_layout_from_a_state_dict_with_extra_keys():
    sd = recipe.make_vgg19_state_dict()
    items, total = _lib.ploss_layout()
    names = [n for n, _, _ in items]
    assert names == [f"{n}.{leaf}" for _, n, _, _ in losses.VGG_CONVS for leaf in ("w", "b")]
    assert all(off % 64 == 0 for _, off, _ in items) and total % 64 == 0
    full = dict(sd)
    full["features.16.weight"] = np.zeros((512, 256, 3, 3), np.float32)      # the rest of vgg19: ignored
    full["classifier.0.bias"] = np.zeros(4096, np.float32)
    buf = losses.pack(full)
    assert buf.dtype == np.float32 and buf.size == total and np.array_equal(buf, losses.pack(sd))
    got = _lib.unpack_named(buf, (items, total))
    w = sd["features.5.weight"]                                               # conv2_1: [cout][ky][kx][cin]
    assert np.array_equal(got["conv2_1.w"].reshape(128, 3, 3, 64), w.transpose(0, 2, 3, 1))
    w = sd["features.0.weight"]                                               # conv1_1: [(ky,kx,cin)][64]
    assert np.array_equal(got["conv1_1.w"].reshape(3, 3, 3, 64), w.transpose(2, 3, 1, 0))
    assert np.array_equal(got["conv3_3.b"], sd["features.14.bias"])
    for key in ("features.7.weight", "features.14.bias"):
        with pytest.raises(ValueError, match=re.escape(key)):
            losses.pack({k: v for k, v in sd.items() if k != key})
    bad = dict(sd)
    bad["features.2.weight"] = np.zeros((64, 64, 1, 1), np.float32)
    with pytest.raises(ValueError, match="features.2.weight"):
        losses.pack(bad)


def test_only_a_mean_mse_criterion_is_taken():
    sd = recipe.make_vgg19_state_dict()
    for crit in (torch.nn.L1Loss(), torch.nn.MSELoss(reduction="sum"), torch.nn.MSELoss(reduction="none"), None, "mse"):
        with pytest.raises(ValueError, match="MSELoss"):
            losses.PerceptualLoss(crit, state_dict=sd)             # raised before any device call: this machine may have no GPU
    with pytest.raises(ValueError, match="one of them"):
        losses.TrainingLoss()
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses._check_pair("t", torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match=r"float32 \[B,3,H,W\]"):
        losses._check_pair("t", torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8))


def test_the_weight_transform_twin():
    rng = np.random.default_rng(5)
    for _, _name, cin, cout in losses.VGG_CONVS[1:]:
        w = rng.standard_normal(cout * 9 * cin).astype(np.float32)
        t = losses.weight_transform(w, cout, cin)
        assert t.shape == w.shape and np.array_equal(losses.weight_transform(t, cin, cout), w)        # twice: the identity
        w4, t4 = w.reshape(cout, 3, 3, cin), t.reshape(cin, 3, 3, cout)
        assert t4[5, 0, 2, 7] == w4[7, 2, 0, 5] and t4[1, 1, 1, 2] == w4[2, 1, 1, 1]
    # the backward-data pass of the conv IS the conv on the transformed matrix, channel axes swapped
    cin, cout = 8, 12
    w = torch.randn(cout, cin, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    g = torch.randn(2, cout, 5, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    rows = w.permute(0, 2, 3, 1).reshape(-1).numpy()
    wt = torch.from_numpy(losses.weight_transform(rows, cout, cin).reshape(cin, 3, 3, cout)).permute(0, 3, 1, 2)
    want = torch.nn.functional.conv_transpose2d(g, w, padding=1)
    assert torch.allclose(torch.nn.functional.conv2d(g, wt, padding=1), want, rtol=0, atol=1e-12)


def test_saved_and_scratch_grow_with_the_batch_and_refuse_by_size():
    lib = _lib.load()
    for fn in (lib.casync_ploss_saved_bytes, lib.casync_ploss_scratch_bytes):
        sizes = [fn(b, 160, 160) for b in (1, 2, 3, 16, 64, 327)]
        assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(set(sizes)), sizes
        assert fn(1, 4, 4) > 0 and fn(1, 3, 160) == 0 and fn(1, 160, 3) == 0 and fn(0, 160, 160) == 0
        assert fn(328, 160, 160) == 0                    # [B,160,160,64] fp32 reaches 2 GiB at B = 328
    # saved: a1_1, a1_2, a2_1, a2_2, a3_1, a3_2, d of the prediction
    assert lib.casync_ploss_saved_bytes(2, 160, 160) == 4 * 2 * (2 * 160 * 160 * 64 + 2 * 80 * 80 * 128 + 3 * 40 * 40 * 256)
    assert lib.casync_ploss_partials(1) == 1 and lib.casync_ploss_partials(257) == 2 and lib.casync_ploss_partials(1 << 40) == 1024
    for backward, stages in ((0, losses.FORWARD_STAGES), (1, losses.BACKWARD_STAGES)):
        eng = losses.PerceptualEngine.__new__(losses.PerceptualEngine)
        for s in range(len(stages)):
            assert lib.casync_ploss_tap_floats(backward, 2, 10, 14, s) == int(np.prod(eng.tap_shape(bool(backward), s, 2, 10, 14))), (backward, s)
        assert lib.casync_ploss_tap_floats(backward, 2, 10, 14, len(stages)) == 0
