"""The host side of the trainer's batches (calipsync_amd/train_data.py), no GPU: the dataset's box rule, the rectangle, the
sampler, the errors raised before anything reaches a device, the new header and its symbol, and the audio windows against the
reference's own ``MyDataset.get_audio_features`` (tests/golden/train_windows.npz, written by tests/golden/make_train_golden.py)."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import stream_contract
import train_data_ref as ref
import workspace_contract
from calipsync_amd import _lib, frame_loop, train_data

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "casync_train.h")


def lms_for(xmin, ymin, xmax, dtype=np.float64):
    l = np.zeros((110, 2), dtype=dtype)
    l[1][0], l[52][1], l[31][0] = xmin, ymin, xmax
    return l


# ------------------------------------------------------------------------------------------------ the box rule
@pytest.mark.parametrize("xmin,ymin,xmax,want", [
    (100, 50, 190, (50, 100, 90, 90)),           # inside
    (100, 250, 190, (250, 100, 50, 90)),         # ymax = 340 > 300: cut at the bottom
    (350, 50, 440, (50, 350, 90, 50)),           # xmax = 440 > 400: cut at the right
    (350, 250, 440, (250, 350, 50, 50)),         # both
    (310, 210, 400, (210, 310, 90, 90)),         # ends on the last row and column
    (399, 299, 400, (299, 399, 1, 1)),           # the last pixel
    (0, 0, 1, (0, 0, 1, 1)),
])
def test_box_rule_hand_cases(xmin, ymin, xmax, want):
    got = train_data.dataset_crop_box(lms_for(xmin, ymin, xmax), 300, 400)
    assert got == want and all(type(v) is int for v in got)
    img = np.zeros((300, 400, 3), np.uint8)
    assert ref.region(img, lms_for(xmin, ymin, xmax)).shape[:2] == want[2:]         # what numpy slicing cuts


@pytest.mark.parametrize("xmin,ymin,xmax", [
    (-1, 50, 90),        # xmin < 0: numpy would wrap
    (100, -1, 190),      # ymin < 0
    (100, 50, 100),      # width 0
    (100, 50, 60),       # width < 0
    (400, 50, 490),      # xmin == W
    (100, 300, 190),     # ymin == H
])
def test_box_rule_unusable_frames(xmin, ymin, xmax):
    assert train_data.dataset_crop_box(lms_for(xmin, ymin, xmax), 300, 400) is None


def test_box_rule_truncates_like_the_file_parse_and_differs_from_the_inference_box():
    assert train_data.dataset_crop_box(lms_for(100.9, 50.9, 190.2), 300, 400) == (50, 100, 90, 90)
    assert train_data.dataset_crop_box(lms_for(100, 50, 190, np.int32), 300, 400) == (50, 100, 90, 90)
    low = lms_for(100, 250, 190)
    ymin, ymax, xmin, xmax, width = frame_loop.crop_box(low, 300, 400)           # the inference rule shifts the square up
    assert (ymin, ymax, xmin, xmax) == (210, 300, 100, 190)
    assert train_data.dataset_crop_box(low, 300, 400) == (250, 100, 50, 90)      # the dataset's is cut
    right = lms_for(350, 50, 440)
    ymin, ymax, xmin, xmax, width = frame_loop.crop_box(right, 300, 400)         # ... and keeps the height where it clamps x
    assert (ymax - ymin, xmax - xmin) == (90, 50)
    assert train_data.dataset_crop_box(right, 300, 400) == (50, 350, 90, 50)
    assert frame_loop.crop_box(lms_for(-5, 50, 85), 300, 400)[2] == 0 and train_data.dataset_crop_box(lms_for(-5, 50, 85), 300, 400) is None


def test_read_lms_parses_integer_and_float_text(tmp_path):
    pts = np.arange(220, dtype=np.int64).reshape(110, 2) * 3 - 7
    a, b = tmp_path / "a.lms", tmp_path / "b.lms"
    np.savetxt(a, pts, fmt="%d")
    b.write_text("\n".join(f"{x + 0.75:.6f} {y - 0.25:.3f}" for x, y in pts) + "\n")
    got = train_data.read_lms(str(a))
    assert got.dtype == np.int32 and np.array_equal(got, pts)
    want = np.array((pts + [0.75, -0.25]).astype(np.float32), dtype=np.int32)       # towards zero
    assert np.array_equal(train_data.read_lms(str(b)), want) and (want[:3] == [[-6, -4], [0, 1], [5, 7]]).all()


# ------------------------------------------------------------------------------------------------ the rectangle
def test_rectangle_extents():
    real = np.full((160, 160, 3), 255, np.uint8)
    cat, img_real = ref.tensors(real, real // 5)
    assert cat.shape == (6, 160, 160) and img_real.shape == (3, 160, 160) and cat.dtype == img_real.dtype == np.float32
    masked = cat[3:]
    for x, y in ((5, 5), (154, 149)):
        assert (masked[:, y, x] == 0).all(), (x, y)
    for x, y in ((4, 5), (155, 149), (5, 4), (5, 150)):
        assert (masked[:, y, x] == 1).all(), (x, y)
    assert int((masked[0] == 0).sum()) == 150 * 145
    assert (img_real == 1).all() and (cat[:3] == np.float32(51) / np.float32(255)).all()


# ------------------------------------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("n_img,n_items", [(12, 11), (12, 16), (5, 39), (40, 7)])
def test_one_epoch_visits_every_item_once_and_never_pairs_a_frame_with_itself_by_draw(n_img, n_items):
    s = train_data.TrainSampler(n_img, n_items, batch_size=4, seed=11)
    for _ in range(3):
        batches = s.epoch()
        items = np.concatenate([b[0] for b in batches])
        refs = np.concatenate([b[1] for b in batches])
        assert sorted(items.tolist()) == list(range(n_items))
        assert refs.min() >= 0 and refs.max() < n_items
        t = s.frame_of(items)
        assert (refs != t).all()                       # the reference excludes the index it has clamped (dataset.py:137, 142)
        if n_items <= n_img:
            assert (refs != items).all() and (t == items).all()
        assert t.max() <= n_img - 1 and s.frame_of(refs).max() <= n_img - 1
        assert all(ref.frames_of(int(i), int(e), n_img) == (int(a), int(b)) for i, e, a, b in zip(items, refs, t, s.frame_of(refs)))
    if n_items > n_img:
        assert (s.frame_of(np.arange(n_img, n_items)) == n_img - 1).all()


def test_reference_items_cover_everything_but_the_target():
    s = train_data.TrainSampler(6, 5, batch_size=5, shuffle=False, seed=0)
    seen = {i: set() for i in range(5)}
    for _ in range(200):
        (items, refs), = s.epoch()
        assert items.tolist() == [0, 1, 2, 3, 4]
        for i, e in zip(items, refs):
            seen[int(i)].add(int(e))
    assert all(seen[i] == set(range(5)) - {i} for i in range(5)), seen


def test_same_seed_same_epochs_and_len():
    a, b, c = (train_data.TrainSampler(9, 23, batch_size=5, seed=s) for s in (3, 3, 4))
    ea = [a.epoch() for _ in range(3)]
    eb = [b.epoch() for _ in range(3)]
    flat = lambda e: [np.concatenate([np.concatenate(x) for x in ep]).tolist() for ep in e]
    assert flat(ea) == flat(eb) and flat(ea) != flat([c.epoch() for _ in range(3)])
    assert flat(ea)[0] != flat(ea)[1]                                              # a new permutation per epoch
    assert len(a) == 5 and [len(x[0]) for x in ea[0]] == [5, 5, 5, 5, 3]
    d = train_data.TrainSampler(9, 23, batch_size=5, drop_last=True, seed=3)
    assert len(d) == 4 and [len(x[0]) for x in d.epoch()] == [5, 5, 5, 5]
    assert len(train_data.TrainSampler(9, 20, batch_size=5)) == len(train_data.TrainSampler(9, 20, batch_size=5, drop_last=True)) == 4
    assert [x[0].tolist() for x in train_data.TrainSampler(9, 5, batch_size=2, shuffle=False).epoch()] == [[0, 1], [2, 3], [4]]


class _HostClip:
    """what TrainingBatches reads from a ResidentClip before it uploads anything; the device is out of reach"""

    def __init__(self, n, H=300, W=400, lms=None, source_index=None):
        self.landmarks = [lms_for(100, 50, 190) if lms is None else lms] * n
        self.H, self.W, self.n, self.source_index = H, W, n, source_index
        self.frames = object()

    def __len__(self):
        return self.n

    @property
    def device(self):
        raise AssertionError("the constructor reached for the device")


def test_every_refusal_comes_before_any_device_call(monkeypatch):
    def no_library():
        raise AssertionError("the constructor loaded the library")
    monkeypatch.setattr(_lib, "load", no_library)
    feats = np.zeros((20, 2, 1024), np.float32)
    with pytest.raises(NotImplementedError):
        train_data.TrainingBatches(_HostClip(12), np.zeros((20, 256, 16), np.float32), mode="wenet")
    with pytest.raises(NotImplementedError):
        train_data.TrainingBatches(_HostClip(12), feats, mode="wenet")
    with pytest.raises(ValueError, match=r"frame\(s\) \[3\]"):
        clip = _HostClip(12)
        clip.landmarks = list(clip.landmarks)
        clip.landmarks[3] = lms_for(-2, 50, 88)
        train_data.TrainingBatches(clip, feats)
    with pytest.raises(ValueError, match="fewer than 16 rows"):
        train_data.TrainingBatches(_HostClip(12), np.zeros((4, 2, 1024), np.float32))
    for steps in (1, 2):                                                           # T - 1 < 2
        with pytest.raises(ValueError, match="T - 1 >= 2"):
            train_data.TrainingBatches(_HostClip(12), np.zeros((steps, 2, 1024), np.float32))
    with pytest.raises(ValueError, match="dropped frames"):
        train_data.TrainingBatches(_HostClip(3, source_index=[0, 2, 3]), feats)
    with pytest.raises(ValueError, match=r"\[T,2,1024\]"):
        train_data.TrainingBatches(_HostClip(12), np.zeros((20, 1024), np.float32))
    # an unusable frame the epoch never reaches does not count; a clip that kept every frame passes its source_index
    clip = _HostClip(12, source_index=list(range(12)))
    clip.landmarks = list(clip.landmarks)
    clip.landmarks[11] = lms_for(-2, 50, 88)
    with pytest.raises(AssertionError, match="reached for the device"):            # everything checked: the upload is next
        train_data.TrainingBatches(clip, np.zeros((9, 2, 1024), np.float32))


# ------------------------------------------------------------------------------------------------ header and library
@pytest.fixture(scope="module")
def lib():
    from calipsync_amd import build
    build.build()
    return _lib.load()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(casync_[a-z0-9_]+)\s*\(", text)), text


def test_train_header_is_c99_with_the_plain_c_host(lib, tmp_path):
    exe = tmp_path / "abi_host"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-include", "casync_train.h",
                    os.path.join(REPO, "tests", "c", "abi_host.c"), "-ldl", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), _lib.lib_path()], check=True, capture_output=True, text=True).stdout
    assert out.startswith("abi 13 ")
    alone = tmp_path / "alone.c"                                                  # ... and on its own, the entry's type spelt out
    alone.write_text('#include "casync_train.h"\nint (*p)(const uint8_t*, int, int, int, const int32_t*, int, float*, float*, casync_stream) = '
                     "casync_op_train_batch;\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-c", str(alone), "-o",
                    str(tmp_path / "alone.o")], check=True)


def test_every_symbol_of_the_train_header_is_exported_and_the_abi_is_still_13(lib):
    declared, text = _declared()
    assert declared == set(_lib.EXPORTS_TRAIN) == {"casync_op_train_batch"}
    assert not declared & set(_lib.EXPORTS)                       # tests/test_abi.py closes casync_hip.h over EXPORTS
    for name in declared:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert lib.casync_abi_version() == _lib.ABI_VERSION == 13
    assert "CASYNC_ABI_VERSION" not in text and '#include "casync_hip.h"' in text          # additive: the version is not redefined


def test_the_train_header_closes_its_stream_and_workspace_sets():
    import test_train_stream_contract_gpu as gpu_side
    entries = stream_contract.stream_entries(path=HEADER)
    assert entries == ["casync_op_train_batch"]
    covered = [e for a in gpu_side.ADAPTERS for e in a.entries]
    assert sorted(covered) == sorted(entries)
    assert workspace_contract.workspace_entries(path=HEADER) == []
    assert "casync_op_train_batch" not in stream_contract.stream_entries()          # casync_hip.h itself is unchanged


# ------------------------------------------------------------------------------------------------ the audio windows
def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def test_audio_windows_equal_the_references_own():
    g = np.load(os.path.join(REPO, "tests", "golden", "train_windows.npz"))
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "train_windows.npz")) < 100_000
    assert g["clips"].tolist() == [8, 16, 17, 40]
    full = 0
    for t in g["clips"].tolist():
        feats = ref.train_features(t)
        assert np.array_equal(_sha(feats), g[f"T{t}.features_sha256"])
        rows = g[f"T{t}.rows"]
        assert rows.shape == (t - 1,) and (rows == 16).all()
        windows = frame_loop.audio_windows_host(feats, list(range(t - 1)))
        for idx in range(t - 1):
            assert train_data.window_rows(t, idx) == rows[idx], (t, idx)
            assert np.array_equal(_sha(windows[idx]), g[f"T{t}.window_sha256"][idx]), (t, idx)
            if f"T{t}.idx{idx}.full" in g:
                full += 1
                assert np.array_equal(windows[idx], g[f"T{t}.idx{idx}.full"])
    assert full == 6
    # the counts the constructor refuses, from the same method: the reference's reshape(32, 32, 32) raises there
    assert g["short_clips"].tolist() == [3, 5, 7]
    for t in g["short_clips"].tolist():
        rows = g[f"T{t}.rows"]
        assert rows.shape == (t - 1,) and (rows != 16).any()
        assert [train_data.window_rows(t, i) for i in range(t - 1)] == rows.tolist(), t
