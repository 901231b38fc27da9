"""PFLD_GhostOne landmark network, host side (no GPU): checkpoint forms, the RepVGG fold, the packed layout, and the
LipDetector arithmetic, against tests/golden/pfld_b3.npz (made by tests/golden/make_pfld_golden.py from the reference)."""
import os

import numpy as np
import pytest
import torch

import pfld_ref
from calipsync_amd import landmarks, recipe
from conftest import GOLDEN, sample_indices


def _manifest(name):
    out = []
    with open(os.path.join(GOLDEN, name)) as f:
        for line in f:
            key, rest = line.split(" ", 1)
            shape = rest[:rest.rindex(")") + 1]
            out.append((key, tuple(int(v) for v in shape.strip("()").split(",") if v.strip())))
    return out


@pytest.fixture(scope="module")
def sd():
    return recipe.make_pfld_state_dict()


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "pfld_b3.npz"))


def test_recipe_has_the_reference_keys_and_shapes(sd):
    want = _manifest("state_dict_manifest_pfld.txt")
    assert len(want) == 2090
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert landmarks.check_state_dict(sd) == "train"


def test_fold_and_restatement_match_the_reference_in_float64(sd, fixture):
    """fold (float64, not rounded) + tests/pfld_ref.py in float64 against the reference's own float64 run: pins both"""
    u8 = recipe.make_pfld_inputs(3)
    x = torch.from_numpy((np.asarray(u8, dtype=np.float32) / 255.0).transpose(0, 3, 1, 2).copy()).double()
    y, stages = pfld_ref.forward(landmarks.fold(sd, dtype=np.float64), x)
    ref = fixture["out64"]
    assert np.abs(y.numpy() - ref).max() <= 1e-9 * np.abs(ref).max()
    assert len(stages) == len(landmarks.STAGES) == 16
    for name, t, (h, w, c) in zip(landmarks.STAGES, stages, landmarks.STAGE_SHAPES):
        a = t.numpy()
        assert tuple(fixture[f"{name}.shape"]) == a.shape == (3, c, h, w), name
        flat = a.reshape(-1)
        top = max(abs(fixture[f"{name}.stats"][3]), abs(fixture[f"{name}.stats"][4]))
        assert np.abs(flat[sample_indices(flat.size)] - fixture[f"{name}.samples"]).max() <= 1e-9 * top, name
        stats = np.array([flat.sum(), np.abs(flat).sum(), (flat * flat).sum(), flat.min(), flat.max()])
        assert np.allclose(stats, fixture[f"{name}.stats"], rtol=1e-9, atol=1e-9 * flat.size), name


def test_inference_form_keys_match_the_reference(sd):
    want = _manifest("state_dict_manifest_pfld_inference.txt")
    assert len(want) == 107
    inf = landmarks.to_inference_form(sd)
    assert sorted((k, tuple(v.shape)) for k, v in inf.items()) == sorted(want)
    assert landmarks.manifest("inference") == want
    assert landmarks.check_state_dict(inf) == "inference"


def test_both_forms_pack_to_the_same_buffer(sd):
    from calipsync_amd import build
    build.build()
    a = landmarks.pack(sd)
    b = landmarks.pack(landmarks.to_inference_form(sd))
    assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
    un = landmarks.unpack(a)
    named = landmarks.packed_tensors(sd)
    assert set(un) == set(named)
    for k, v in named.items():
        assert np.array_equal(un[k], v.reshape(-1)), k
    # zero padding of the MFMA granule: conv5_2's first pointwise conv is 72 -> 126, packed [80][128]
    w = un["conv5_2.g1.pw.w"].reshape(80, 128)
    assert not w[72:].any() and not w[:, 126:].any() and w[:72, :126].all()


@pytest.mark.parametrize("form", ["train", "inference"])
def test_check_state_dict_names_the_key(sd, form):
    base = sd if form == "train" else landmarks.to_inference_form(sd)
    key = "conv4_2.ghost_conv.2.cheap_operation.rbr_conv.3.bn.running_var" if form == "train" else "conv4_2.ghost_conv.2.cheap_operation.reparam_conv.bias"
    gone = {k: v for k, v in base.items() if k != key}
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        landmarks.check_state_dict(gone)
    renamed = dict(gone)
    renamed[key + "_x"] = base[key]
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        landmarks.check_state_dict(renamed)
    extra = dict(base)
    extra["stn.fc.weight"] = np.zeros(3, np.float32)
    with pytest.raises(ValueError, match="unexpected key stn"):
        landmarks.check_state_dict(extra)
    wide = dict(base)
    wide["conv_out.weight"] = np.zeros((136, 256, 1, 1), np.float32)      # another landmark count
    with pytest.raises(ValueError, match="conv_out.weight"):
        landmarks.check_state_dict(wide)
    assert landmarks.check_state_dict(base) == form


def test_num_batches_tracked_is_ignored(sd):
    """a train-form checkpoint saved without the counters, or with some of them, is the same checkpoint"""
    counters = [k for k in sd if k.endswith("num_batches_tracked")]
    assert counters
    bare = {k: v for k, v in sd.items() if k not in counters}
    assert len(bare) == 2090 - len(counters) and landmarks.check_state_dict(bare) == "train"
    some = {k: v for k, v in sd.items() if k not in counters[::2]}
    assert landmarks.check_state_dict(some) == "train"
    want, got = landmarks.fold(sd), landmarks.fold(bare)
    assert set(want) == set(got) and all(np.array_equal(want[k], got[k]) for k in want)
    # the counters are all that may be missing
    key = "conv3_1.ghost_conv.0.primary_conv.rbr_conv.0.bn.running_mean"
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        landmarks.check_state_dict({k: v for k, v in bare.items() if k != key})


class _Stub:
    def __init__(self, y):
        self.y, self.calls = y, 0

    def forward_u8(self, crops):
        self.calls += 1
        assert crops.shape == (len(self.y), 192, 192, 3) and crops.dtype == np.uint8
        return torch.from_numpy(self.y.copy())


def _detector(fixture, monkeypatch):
    stub = _Stub(fixture["out32"])
    monkeypatch.setattr(landmarks.LandmarkDetector, "_make_engine", staticmethod(lambda sd, device: stub))
    return landmarks.LandmarkDetector(state_dict={}, mean_face=fixture["mean_face"]), stub


def test_landmark_arithmetic_reproduces_the_reference_integers(fixture, monkeypatch):
    det, stub = _detector(fixture, monkeypatch)
    got = det.landmarks_from_crops(recipe.make_pfld_inputs(3), [tuple(s) for s in fixture["sizes"]], [tuple(o) for o in fixture["offsets"]])
    assert len(got) == 3 and all(g.dtype == np.int32 and g.shape == (110, 2) for g in got)
    assert np.array_equal(np.stack(got), fixture["landmarks"])


def test_detect_landmarks_batches_all_crops_into_one_forward(fixture, monkeypatch, tmp_path):
    det, stub = _detector(fixture, monkeypatch)
    imgs = [np.full((300, 400, 3), 7, np.uint8), np.zeros((50, 60, 3), np.uint8), np.full((500, 500, 3), 9, np.uint8)]
    res = det.detect_landmarks(imgs, boxes=[[(100, 80, 120, 150)], [], [(10, 10, 200, 200), (250, 250, 100, 90)]])
    assert stub.calls == 1 and res[1] is None and len(res[0]) == 1 and len(res[2]) == 2
    crop, (ox, oy) = det._crop(imgs[0], (100, 80, 120, 150))
    pre = (fixture["out32"][0] + fixture["mean_face"]).reshape(-1, 2)
    pre[:, 0] = pre[:, 0] * crop.shape[1] + ox
    pre[:, 1] = pre[:, 1] * crop.shape[0] + oy
    assert np.array_equal(res[0][0], pre.astype(np.int32))
    with pytest.raises(ValueError, match="no boxes"):
        det.detect_landmarks(imgs)
    path = tmp_path / "0.lms"
    landmarks.write_lms(str(path), res[0][0])
    assert np.array_equal(np.loadtxt(path, dtype=np.int32), res[0][0])


@pytest.mark.parametrize("box,edge", [((-30, 40, 100, 100), "left"), ((40, -30, 100, 100), "top"), ((230, 40, 100, 100), "right"),
                                      ((40, 150, 100, 100), "bottom"), ((-20, -20, 340, 240), "all"), ((60, 50, 80, 100), "none")])
def test_crop_pads_with_zeros_at_every_edge(box, edge):
    """lip_detector.py:46-75: the 1.05 x square; outside the image the crop is zero and the offset goes negative"""
    rng = np.random.default_rng(3)
    img = rng.integers(1, 255, (200, 300, 3), dtype=np.uint8)
    crop, (ox, oy) = landmarks.LandmarkDetector._crop(img, box)
    x, y, w, h = box
    size = int(max(w, h) * 1.05)
    x1, y1 = (2 * x + w) // 2 - size // 2, (2 * y + h) // 2 - size // 2
    assert crop.shape == (size, size, 3) and (ox, oy) == (x1, y1)
    want = np.zeros((size, size, 3), np.uint8)
    for j in range(size):
        for i in range(size):
            if 0 <= y1 + j < 200 and 0 <= x1 + i < 300:
                want[j, i] = img[y1 + j, x1 + i]
    assert np.array_equal(crop, want)
    assert (want == 0).any() == (edge != "none")


def test_no_cpu_fallback(sd):
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="device"):
        landmarks.PFLDEngine(sd)
