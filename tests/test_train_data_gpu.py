"""-m gpu: the trainer's batch kernel (csrc/train_ops.hip, casync_op_train_batch) against the numpy restatement
(tests/train_data_ref.py) bit for bit, against the pinned inference path (casync_frame_prepare), its refusals, and the loader
around it (calipsync_amd/train_data.py) against the restatement plus the reference's own audio windows
(tests/golden/train_windows.npz).  Outputs sit between sentinel floats, which must survive.

The kernel cases are those of tests/kernel_ledger_train.py (one run per process, shared with tests/test_kernel_ledger_train_gpu.py):
  frames 211 x 317 (a row of 951 bytes, no multiple of 16) and 720 x 720; square regions of width 1, 2, 3, 83-85, 167-169 (168 is a
  copy), 336 (the exact-2x branch), 337 and 701; regions cut at the bottom edge, at the right edge and at both, a box that ends on
  the last row and column, a 336-wide region of 200 rows (not the 2x branch); target and reference the same frame and box; one
  frame; batches of 1 and of 65 (one more than a launch's block of records); outputs that start off a 16-byte boundary; and one
  record whose frame starts above byte 2^31 of an uninitialised store."""
import hashlib
import os

import numpy as np
import pytest
import torch

import gpu_util
import kernel_ledger_train as kl
import train_data_ref as ref
from calipsync_amd import _lib, train_data
from kernel_ledger import C

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ the kernel
def test_the_cases_hold_what_they_are_named_for():
    small, large = kl.boxes(211, 317), kl.boxes(720, 720)
    assert {w for _, _, h, w in large if h == w} >= set(kl.WIDTHS) and {w for _, _, h, w in small if h == w} >= {1, 2, 3, 83, 84, 85, 167, 168, 169}
    assert (211 * 317 * 3) % 16 != 0 and (317 * 3) % 16 != 0
    for H, W, bx in ((211, 317, small), (720, 720, large)):
        assert any(y + h == H and x + w < W and h < w for y, x, h, w in bx)             # cut at the bottom
        assert any(x + w == W and y + h < H and w < h for y, x, h, w in bx)             # cut at the right
        assert any(y + h == H and x + w == W and h != w for y, x, h, w in bx)           # at both
        assert any(y + h == H and x + w == W and h == w for y, x, h, w in bx)           # a square ending on the last row and column
    assert (200, 336) in {(h, w) for _, _, h, w in large}
    rec = kl.records(211, 317, 3)
    assert (rec[-1, 0:5] == rec[-1, 5:10]).all() and (rec[:-1, 0] != rec[:-1, 5]).any()
    assert {tuple(r[1:5]) for r in rec} == {tuple(r[6:10]) for r in rec[:-1]} | {tuple(rec[0, 1:5])}   # every box on both sides


@pytest.mark.parametrize("case", [C(kl.shapes, 211, 317, 3), C(kl.shapes, 720, 720, 2), C(kl.shapes, 211, 317, 1), C(kl.many, 211, 317, 3, 1),
                                  C(kl.many, 211, 317, 3, kl.RECORDS_PER_LAUNCH + 1), C(kl.shapes, 211, 317, 3, 1), C(kl.shapes, 720, 720, 2, 3),
                                  C(kl.many, 211, 317, 2, kl.RECORDS_PER_LAUNCH + 1, 2)], ids=repr)
def test_kernel_equals_the_restatement_bit_for_bit(case):
    assert case in {c for _, _, c in kl.cases()}
    out = case.run()
    print(f"{out.what}: {out.err:.0f} floats differ")
    assert out.err == 0, out.what


def test_a_frame_that_starts_above_byte_2_31():
    H = W = 720
    last = (1 << 31) // (H * W * 3) + 1                                    # 1381: its first byte is past 2^31
    assert last * H * W * 3 > 1 << 31 > (last - 1) * H * W * 3
    store = torch.empty((last + 1, H, W, 3), dtype=torch.uint8, device=DEV)          # uninitialised: only two frames are written
    two = kl.noise_frames(2, H, W, "high")
    store[last].copy_(torch.from_numpy(two[0]))
    store[0].copy_(torch.from_numpy(two[1]))
    rec = np.asarray([(last, 100, 150, 337, 337, 0, 383, 20, 337, 700, 0, 0), (0, 0, 0, 720, 720, last, 719, 719, 1, 1, 0, 0)], dtype=np.int32)
    assert kl.differing({last: two[0], 0: two[1]}, rec, frames_dev=store) == 0
    del store
    torch.cuda.empty_cache()


def test_equals_the_inference_path_where_target_and_reference_coincide():
    """reference = target, boxes inside the frame: img_concat is the x casync_frame_prepare gives for the same regions"""
    H, W = 400, 420
    frames = kl.noise_frames(2, H, W, "prepare")
    boxes = [(0, 10, 20, 83, 83), (1, 5, 7, 168, 168), (0, 30, 40, 336, 336), (1, 50, 60, 337, 337), (1, 399, 419, 1, 1)]
    rec = np.zeros((len(boxes), 12), np.int32)
    rec[:, 0:5] = rec[:, 5:10] = boxes
    regions = [np.ascontiguousarray(frames[f][y:y + h, x:x + w]).reshape(-1) for f, y, x, h, w in boxes]
    geom = np.zeros((len(boxes), 12), np.int32)
    geom[:, 0] = np.cumsum([0] + [r.size for r in regions[:-1]])
    geom[:, 1], geom[:, 2], geom[:, 3], geom[:, 4], geom[:, 7] = rec[:, 3], rec[:, 4], rec[:, 4], 1, -1
    reg_dev, geom_dev = torch.from_numpy(np.concatenate(regions)).to(DEV), torch.from_numpy(geom).to(DEV)
    crops = torch.empty((len(boxes), 168, 168, 3), dtype=torch.uint8, device=DEV)
    x = torch.empty((len(boxes), 6, 160, 160), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().casync_frame_prepare(reg_dev.data_ptr(), geom_dev.data_ptr(), len(boxes), crops.data_ptr(), x.data_ptr(), _stream()),
               "casync_frame_prepare")
    cat, real = train_data.train_batch(torch.from_numpy(frames).to(DEV), rec)
    assert torch.equal(cat.view(torch.int32), x.view(torch.int32))
    assert torch.equal(real.view(torch.int32), x[:, :3].contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ refusals
GOOD = (1, 10, 20, 60, 60, 2, 5, 7, 84, 84, 0, 0)


def _with(word, value, row=GOOD):
    r = list(row)
    r[word] = value
    return tuple(r)


REFUSED = {
    "null frames": dict(frames=0), "null records": dict(rec=0), "null img_concat": dict(cat=0), "null img_real": dict(real=0),
    "H 0": dict(H=0), "W -1": dict(W=-1), "batch -1": dict(batch=-1),
    "target frame -1": dict(rows=[_with(0, -1)]), "target frame n": dict(rows=[_with(0, 3)]), "reference frame n": dict(rows=[_with(5, 3)]),
    "reference frame -2": dict(rows=[_with(5, -2)]),
    "h 0": dict(rows=[_with(3, 0)]), "w 0": dict(rows=[_with(4, 0)]), "rh -3": dict(rows=[_with(8, -3)]), "rw 0": dict(rows=[_with(9, 0)]),
    "y0 -1": dict(rows=[_with(1, -1)]), "x0 -1": dict(rows=[_with(2, -1)]), "past the bottom": dict(rows=[_with(1, 38)]),
    "past the right": dict(rows=[_with(2, 72)]), "reference past the bottom": dict(rows=[_with(6, 14)]),
    "reference past the right": dict(rows=[_with(7, 48)]), "h overflows int": dict(rows=[_with(3, 2 ** 31 - 1)]),
    "second record": dict(rows=[GOOD, _with(4, 0)]),
    "first record of the second launch": dict(rows=[GOOD] * kl.RECORDS_PER_LAUNCH + [_with(0, 3)]),
}


@pytest.fixture(scope="module")
def small_clip():
    return torch.from_numpy(kl.noise_frames(3, 97, 131, "refusals")).to(DEV)


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals_launch_nothing_and_leave_the_outputs_untouched(name, small_clip):
    kw = REFUSED[name]
    rows = np.asarray(kw.get("rows", [GOOD]), dtype=np.int32)
    b = kw.get("batch", len(rows))
    outs = [torch.full((2 * kl.PAD + len(rows) * c * 25600,), kl.SENTINEL, dtype=torch.float32, device=DEV) for c in (6, 3)]
    with gpu_util.launched() as names:
        st = _lib.load().casync_op_train_batch(kw.get("frames", small_clip.data_ptr()), 3, kw.get("H", 97), kw.get("W", 131),
                                               kw.get("rec", rows.ctypes.data), b, kw.get("cat", outs[0].data_ptr() + 4 * kl.PAD),
                                               kw.get("real", outs[1].data_ptr() + 4 * kl.PAD), _stream())
    torch.cuda.synchronize()
    assert st == -1, name                                                            # CASYNC_ERR_ARG
    assert "train_batch" in _lib.load().casync_last_error().decode()
    assert not names, names
    assert all(bool((o == kl.SENTINEL).all()) for o in outs), name


def test_batch_zero_returns_zero_and_the_good_record_is_good(small_clip):
    rows = np.asarray([GOOD], dtype=np.int32)
    st, cat, real, intact = kl.call(small_clip, 3, 97, 131, rows[:0])
    assert st == 0 and intact and cat.shape[0] == 0
    assert kl.differing(small_clip.cpu().numpy(), rows, frames_dev=small_clip) == 0
    cat, real = train_data.train_batch(small_clip, rows[:0])
    assert cat.shape == (0, 6, 160, 160) and real.shape == (0, 3, 160, 160) and cat.is_cuda
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train_data.train_batch(small_clip.cpu(), rows)
    with pytest.raises(RuntimeError, match="status -1"):
        train_data.train_batch(small_clip, np.asarray([_with(0, 3)], dtype=np.int32))


# ------------------------------------------------------------------------------------------------ the loader
def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


@pytest.fixture(scope="module")
def clip12():
    """12 frames of 120 x 160 with 17 feature steps (items 12 .. 15 show the last frame); frame 5's box is cut at the bottom"""
    import frame_data
    from calipsync_amd.resident_clip import ResidentClip
    imgs, lms, _ = frame_data.make_frames(12, 120, 160, seed=41)
    lms[5][52][1] = 101.5
    assert train_data.dataset_crop_box(lms[5], 120, 160)[2] == 19
    clip = ResidentClip(imgs, lms, None, DEV)
    yield clip, imgs, lms, ref.train_features(17)
    clip.close()


def _same(got, want):
    return got.dtype == torch.float32 and got.is_cuda and np.array_equal(got.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def test_batch_for_equals_the_restatement_and_the_fixture_windows(clip12):
    clip, imgs, lms, feats = clip12
    g = np.load(os.path.join(REPO, "tests", "golden", "train_windows.npz"))
    loader = train_data.TrainingBatches(clip, feats, batch_size=4, seed=2)
    assert len(loader) == 4
    items, refs = [0, 5, 11, 12, 15, 7, 5], [3, 14, 5, 0, 13, 15, 5]
    cat, real, audio = loader.batch_for(items, refs)
    want_cat, want_real = ref.batch(imgs, lms, items, refs)
    assert _same(cat, want_cat) and _same(real, want_real)
    assert audio.shape == (7, 32, 32, 32) and audio.dtype == torch.float32 and audio.is_cuda
    windows = audio.cpu().numpy()
    for k, item in enumerate(items):
        t = min(item, 11)                                              # dataset.py:137 clamps idx before :172 takes the window
        assert np.array_equal(_sha(windows[k]), g["T17.window_sha256"][t]), (k, item)
    assert np.array_equal(windows[4], g["T17.idx15.full"]) is False and np.array_equal(windows[4], windows[2])
    with pytest.raises(IndexError):
        loader.batch_for([16], [0])
    with pytest.raises(ValueError):
        loader.batch_for([1, 2], [0])


def test_an_unshuffled_epoch_equals_batch_for_over_range(clip12):
    clip, imgs, lms, feats = clip12
    loader = train_data.TrainingBatches(clip, torch.from_numpy(feats).to(DEV), batch_size=5, shuffle=False, seed=9)
    plan = train_data.TrainSampler(12, 16, batch_size=5, shuffle=False, seed=9).epoch()
    assert [p[0].tolist() for p in plan] == [list(range(0, 5)), list(range(5, 10)), list(range(10, 15)), [15]]
    got = list(loader)
    assert len(got) == len(loader) == 4
    for (cat, real, audio), (items, refs) in zip(got, plan):
        want = loader.batch_for(items, refs)
        assert torch.equal(cat, want[0]) and torch.equal(real, want[1]) and torch.equal(audio, want[2])
        assert cat.shape == (len(items), 6, 160, 160) and real.shape == (len(items), 3, 160, 160) and audio.shape == (len(items), 32, 32, 32)
    second = list(loader)                                              # the next epoch draws other reference frames
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(got, second)) and all(torch.equal(a[1], b[1]) for a, b in zip(got, second))


def test_clip_from_dataset_dir_host_and_device_decode_give_the_same_batches(tmp_path):
    from PIL import Image
    import frame_data
    imgs, lms, _ = frame_data.make_frames(5, 96, 128, seed=43)
    os.makedirs(tmp_path / "full_body_img")
    os.makedirs(tmp_path / "landmarks")
    for i, (img, l) in enumerate(zip(imgs, lms)):
        smooth = np.ascontiguousarray(np.repeat(np.repeat(img[::4, ::4], 4, 0), 4, 1))                 # blocks: a JPEG keeps some of it
        Image.fromarray(smooth[:, :, ::-1]).save(tmp_path / "full_body_img" / f"{i}.jpg", quality=95)
        np.savetxt(tmp_path / "landmarks" / f"{i}.lms", l.astype(np.int32), fmt="%d")
    feats = ref.train_features(8)
    items, refs = [0, 4, 6, 2], [3, 0, 1, 6]
    batches, decoded = {}, None
    for decode in ("host", "device"):
        clip = train_data.clip_from_dataset_dir(str(tmp_path), DEV, decode=decode)
        assert len(clip) == 5 and (clip.H, clip.W) == (96, 128) and clip.landmarks[3].dtype == np.int32
        batches[decode] = train_data.TrainingBatches(clip, feats, batch_size=4).batch_for(items, refs)
        if decode == "host":
            decoded = clip.frames.cpu().numpy()
        torch.cuda.synchronize()
        clip.close()
    for a, b in zip(batches["host"], batches["device"]):
        assert torch.equal(a, b)
    pil = [np.asarray(Image.open(tmp_path / "full_body_img" / f"{i}.jpg").convert("RGB"))[:, :, ::-1] for i in range(5)]
    assert np.array_equal(decoded, np.stack(pil))
    want_cat, want_real = ref.batch(decoded, [l.astype(np.int32) for l in lms], items, refs)
    assert _same(batches["host"][0], want_cat) and _same(batches["host"][1], want_real)
    with pytest.raises(ValueError):
        train_data.clip_from_dataset_dir(str(tmp_path), DEV, decode="gpu")


def test_one_batch_through_the_model_equals_the_host_built_batch(clip12):
    import stream_contract
    clip, imgs, lms, feats = clip12
    net = stream_contract._unet("fp32")
    loader = train_data.TrainingBatches(clip, feats, batch_size=3, seed=4)
    items, refs = [2, 5, 13], [9, 1, 4]
    cat, real, audio = loader.batch_for(items, refs)
    want_cat, _ = ref.batch(imgs, lms, items, refs)
    from calipsync_amd import frame_loop
    host_audio = frame_loop.audio_windows_host(feats, [min(i, 11) for i in items])
    with torch.no_grad():
        got = net(cat, audio)
        want = net(torch.from_numpy(want_cat).to(DEV), torch.from_numpy(host_audio).to(DEV))
    assert got.shape == real.shape == (3, 3, 160, 160) and torch.equal(got, want)
