"""-m gpu: a clip resident on the device (calipsync_amd/resident_clip.py) against today's host-staged path
(frame_loop.process_batch_device) and the oracle (oracle/frame_ops_oracle.process_batch).  These are byte moves around
unchanged kernels: every comparison is exact."""
import gc
import os

import numpy as np
import pytest
import torch

from calipsync_amd import frame_loop, landmarks, recipe, resident_clip
from calipsync_amd.frame_synth import FrameSynthesizer
from calipsync_amd.resident_clip import ResidentClip
from frame_data import make_frames, write_dataset
from oracle import frame_ops_oracle as fo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def gpu_net(recipe_sd):
    from calipsync_amd.unet import Model
    m = Model(6, "hubert").to(DEV)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe_sd.items()})
    return m.eval()


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == np.uint8
        assert np.array_equal(g, w), (i, int(np.count_nonzero(g != w)))


def _border_frames(with_masks):
    imgs, lms, masks = make_frames(7, 420, 560, seed=21, with_masks=with_masks)
    lms[3] = lms[3].copy()
    lms[3][:, 0] += 560 - lms[3][31, 0] + 25            # frame 3: crop box clamped at the right border -> unchanged frame
    lms[5] = lms[5].copy()
    lms[5][:, 1] += 420 - (lms[5][52, 1] + (lms[5][31, 0] - lms[5][1, 0])) + 12   # frame 5: box pushed past the bottom
    return imgs, lms, masks


@pytest.mark.parametrize("with_masks", [False, True])
def test_resident_batch_equals_the_host_staged_path_and_the_oracle(gpu_net, with_masks):
    imgs, lms, masks = _border_frames(with_masks)
    wd = torch.from_numpy(np.random.default_rng(8).standard_normal((7, 32, 32, 32)).astype(np.float32)).cuda()
    clip = ResidentClip(imgs, lms, masks, DEV)
    assert len(clip) == 7 and tuple(clip.frames.shape) == (7, 420, 560, 3) and clip.frames.is_cuda and len(clip.landmarks) == 7
    for indices in (list(range(7)), [5, 6, 5, 4], [2, 2]):
        w = wd[:len(indices)]
        pick = lambda seq: [seq[i] for i in indices]

        def predict(x):
            return gpu_net(torch.from_numpy(x).cuda(), w).cpu().numpy()
        oracle = fo.process_batch(pick(imgs), pick(lms), pick(masks), predict)
        host = frame_loop.process_batch_device(gpu_net, pick(imgs), pick(lms), pick(masks), windows=w)
        pending = clip.submit(gpu_net, indices, windows=w)
        got = pending.result()
        _same(got, host)
        _same(got, oracle)
        on_device = pending.result_device()
        assert on_device.is_cuda and tuple(on_device.shape) == (len(indices), 420, 560, 3) and on_device.dtype == torch.uint8
        _same(list(on_device.cpu().numpy()), got)                                  # device and host results agree
        assert any(not np.array_equal(g, im) for g, im in zip(got, pick(imgs)))    # something was synthesised
        if 3 in indices:
            assert np.array_equal(got[indices.index(3)], imgs[3])                  # the shape-mismatch fallback
    # the download can be left out and asked for later
    late = clip.submit(gpu_net, [1, 0], windows=wd[:2], download=False)
    _same(late.result(), frame_loop.process_batch_device(gpu_net, [imgs[1], imgs[0]], [lms[1], lms[0]], [masks[1], masks[0]], windows=wd[:2]))
    _same(clip.fetch([6, 0, 6]).result(), [imgs[6], imgs[0], imgs[6]])
    assert all(np.array_equal(a, b) for a, b in zip(imgs, _border_frames(with_masks)[0]))       # inputs intact
    clip.close()


def test_masks_of_both_types_and_sizes_give_the_host_staged_pixels(gpu_net):
    rng = np.random.default_rng(31)
    imgs, lms, _ = make_frames(5, 300, 400, seed=13)
    u8 = [rng.integers(0, 256, (300, 400) if i % 2 else (100, 150), dtype=np.uint8) for i in range(5)]
    u8[2] = None
    f32 = [None if m is None else m.astype(np.float32) / 255.0 for m in u8]        # infer_api.py:68-70
    mixed = [m8 if i % 2 else mf for i, (m8, mf) in enumerate(zip(u8, f32))]
    wd = torch.from_numpy(rng.standard_normal((5, 32, 32, 32)).astype(np.float32)).cuda()
    want = frame_loop.process_batch_device(gpu_net, imgs, lms, f32, windows=wd)
    assert any(not np.array_equal(a, b) for a, b in zip(want, frame_loop.process_batch_device(gpu_net, imgs, lms, [None] * 5, windows=wd)))
    for masks in (u8, f32, mixed):
        clip = ResidentClip(imgs, lms, masks, DEV)
        assert len(clip._masks) == 4 and len({m.data_ptr() for m in clip._masks}) == 4          # an allocation each
        assert [m.dtype for m in clip._masks] == [torch.uint8 if m.dtype == np.uint8 else torch.float32 for m in masks if m is not None]
        _same(clip.submit(gpu_net, range(5), windows=wd).result(), want)
        _same(clip.submit(gpu_net, [4, 3, 2, 1, 0], windows=wd).result(),
              frame_loop.process_batch_device(gpu_net, imgs[::-1], lms[::-1], f32[::-1], windows=wd))
        clip.close()


def _dataset_with_an_empty_box(root):
    imgs, lms = write_dataset(root, 10, 270, 360, seed=4)
    bad = lms[2].copy()
    bad[31, 0] = bad[1, 0] - 4                                                      # xmax < xmin: cv2.resize would fail
    np.savetxt(os.path.join(root, "positions", "000002.txt"), bad)
    return imgs


def test_a_batch_with_an_empty_crop_box_returns_the_stored_frames(gpu_net, tmp_path):
    imgs = _dataset_with_an_empty_box(str(tmp_path))
    feats = np.random.default_rng(5).standard_normal((11, 2, 1024)).astype(np.float32)
    runs = {}
    for resident in (False, True):
        fs = FrameSynthesizer(None, str(tmp_path), device=DEV, batch_size=4, seed=9, net=gpu_net, resident=resident)
        runs[resident] = list(fs.iterate_synthesized_frames(feats, 0, True))
    assert len(runs[True]) == len(runs[False]) == 11
    changed = 0
    for start in range(0, 11, 4):
        batch = runs[True][start:start + 4]
        for a, b in zip(batch, runs[False][start:start + 4]):
            assert (a["index"], a["physical_index"]) == (b["index"], b["physical_index"])
            assert np.array_equal(a["frame"], b["frame"])
        if any(o["physical_index"] == 2 for o in batch):
            assert all(np.array_equal(o["frame"], imgs[o["physical_index"]]) for o in batch)
        else:
            changed += sum(not np.array_equal(o["frame"], imgs[o["physical_index"]]) for o in batch)
    assert any(o["physical_index"] == 2 for o in runs[True]) and changed
    clip = fs._clip
    assert clip.geometry.empty.tolist() == [i == 2 for i in range(10)]
    wd = torch.zeros((3, 32, 32, 32), device=DEV)
    _same(clip.submit(gpu_net, [0, 2, 1], windows=wd).result(), [imgs[0], imgs[2], imgs[1]])


@pytest.mark.parametrize("in_flight", [0, 1])
def test_frame_synthesizer_resident_equals_not_resident(gpu_net, tmp_path, in_flight):
    imgs, _ = write_dataset(str(tmp_path), 10, 270, 360, seed=4)
    feats = np.random.default_rng(5).standard_normal((11, 2, 1024)).astype(np.float32)
    make = lambda resident: FrameSynthesizer(None, str(tmp_path), device=DEV, batch_size=4, seed=9, net=gpu_net,
                                             batches_in_flight=in_flight, resident=resident)
    for sync in (True, False):
        off, on = make(False), make(True)
        assert on.resident and not off.resident and on._clip is None
        want = list(off.iterate_synthesized_frames(feats, 0, sync))
        got = list(on.iterate_synthesized_frames(feats, 0, sync))
        assert [o["index"] for o in got] == [o["index"] for o in want] == list(range(11))
        assert [o["physical_index"] for o in got] == [o["physical_index"] for o in want]
        _same([o["frame"] for o in got], [o["frame"] for o in want])
        stored = [np.array_equal(o["frame"], imgs[o["physical_index"]]) for o in got]
        assert (not all(stored)) if sync else all(stored)                       # synthesised / pass-through
        assert len(on._clip) == 10 and on.total_frames == 10
        clip = on._clip
        more = list(on.iterate_synthesized_frames(feats[:5], 0, sync))          # the clip is kept for the life of the object
        assert on._clip is clip and len(more) == 5
    # a clip made elsewhere: no directory
    fs = FrameSynthesizer(None, None, device=DEV, batch_size=4, seed=9, net=gpu_net, batches_in_flight=in_flight, clip=clip)
    assert fs.resident and fs.total_frames == 10
    _same([o["frame"] for o in fs.iterate_synthesized_frames(feats, 0, True)],
          [o["frame"] for o in make(False).iterate_synthesized_frames(feats, 0, True)])
    with pytest.raises(ValueError, match="data_dir"):
        FrameSynthesizer(None, None, device=DEV, net=gpu_net)


def test_frames_of_a_batch_outlive_later_batches_and_give_their_block_back(gpu_net, monkeypatch):
    imgs, lms, _ = make_frames(10, 270, 360, seed=4)
    clip = ResidentClip(imgs, lms, None, DEV)
    wd = torch.from_numpy(np.random.default_rng(3).standard_normal((4, 32, 32, 32)).astype(np.float32)).cuda()
    gc.collect()
    assert resident_clip.outstanding_pinned_bytes() == 0
    held = clip.submit(gpu_net, [0, 1, 2, 3], windows=wd).result()
    first = [f.copy() for f in held]
    assert resident_clip.outstanding_pinned_bytes() >= 4 * 270 * 360 * 3
    assert all(f.flags.writeable and f.base is not None for f in held)
    for indices in ([4, 5, 6, 7], [3, 2, 1, 0], [0, 1, 2, 3]):
        later = clip.submit(gpu_net, indices, windows=wd).result()
        assert not any(np.shares_memory(a, b) for a in later for b in held)
        del later
    _same(held, first)                                                          # nothing overwrote them
    monkeypatch.setattr(resident_clip, "_PINNED_VIEW_CAP", 0)                   # copies instead of views: the same pixels
    before = resident_clip.outstanding_pinned_bytes()
    copied = clip.submit(gpu_net, [0, 1, 2, 3], windows=wd).result()
    _same(copied, first)
    assert resident_clip.outstanding_pinned_bytes() == before
    monkeypatch.undo()
    del held, copied
    gc.collect()
    assert resident_clip.outstanding_pinned_bytes() == 0
    clip.close()


def test_from_frames_is_the_device_pipeline_without_the_directory(gpu_net):
    # the explicit (x, y, w, h) boxes of tests/test_face_pipeline_gpu.py
    BOXES = [[(100, 80, 135, 120), (50, 40, 183, 170), (-20, -30, 366, 300), (-800, -900, 2006, 1500), (-260, 100, 120, 90)],
             [(300, 250, 100, 140), (10.6, 20.9, 150.2, 135.7)]]
    # the recipe's PFLD weights; the mean face is a face (tests/frame_data.landmarks in the unit square) and not the constant 0.5 of
    # tests/test_face_pipeline_gpu.py, so that the landmarks span a crop box and the batch below is synthesised, not handed back
    from frame_data import landmarks as face_shape
    mean_face = face_shape(0.5, 0.45, 0.3, np.random.default_rng(0), jitter=0.0).astype(np.float32).reshape(-1)
    lm = landmarks.LandmarkDetector(state_dict=recipe.make_pfld_state_dict(), mean_face=mean_face, device=DEV)
    two = np.repeat(np.repeat(recipe.make_s3fd_inputs(2), 4, 1), 4, 2)             # 308 x 372
    bgr = [two[0], two[1], two[0][::-1].copy(), two[1][:, ::-1].copy()]
    boxes = [BOXES[0], None, BOXES[1], [BOXES[0][1]]]                               # frame 1 has no face
    clip = ResidentClip.from_frames(bgr, lm, boxes=boxes, chunk=3)                  # two chunks: 3 + 1
    assert clip.source_index == [0, 2, 3] and len(clip) == 3
    rgb = [np.ascontiguousarray(f[:, :, ::-1]) for f in bgr]
    want = lm.detect_landmarks_device(rgb, boxes=boxes)
    assert want[1] is None
    for got, src in zip(clip.landmarks, clip.source_index):
        assert got.dtype == np.int32 and got.shape == (110, 2) and np.array_equal(got, want[src][0])
    assert torch.equal(clip.frames.cpu(), torch.from_numpy(np.stack([bgr[i] for i in clip.source_index])))
    wd = torch.from_numpy(np.random.default_rng(3).standard_normal((3, 32, 32, 32)).astype(np.float32)).cuda()
    kept = [bgr[i] for i in clip.source_index]
    try:                                                                            # the host-staged path on those landmarks
        host = frame_loop.process_batch_device(gpu_net, kept, clip.landmarks, [None] * 3, windows=wd)
    except ValueError as exc:                                                       # (the reference's contract on an empty crop box)
        print(f"host-staged path: {exc}")
        host = kept
    print(f"crop boxes {clip.geometry.box.tolist()}, valid {clip.geometry.valid.tolist()}, empty {clip.geometry.empty.tolist()}")
    got = clip.submit(gpu_net, [0, 1, 2], windows=wd).result()
    _same(got, host)
    assert any(not np.array_equal(g, k) for g, k in zip(got, kept)), "no frame of the batch was synthesised"
    clip.close()
