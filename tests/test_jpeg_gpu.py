"""-m gpu: the device JPEG encoder (csrc/jpeg_enc.hip) against the recorded libjpeg-turbo bytes and the numpy twin, its failure
statuses behind fences, and its wiring into the resident clip, FrameSynthesizer and VideoStreamManager.  Byte equality throughout."""
import os

import numpy as np
import pytest
import torch

import jpeg_cases as jc
from calipsync_amd import jpeg, mjpeg_avi
from calipsync_amd.frame_synth import FrameSynthesizer, VideoStreamManager
from calipsync_amd.resident_clip import ResidentClip
from frame_data import make_frames, write_dataset

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(frames):
    return torch.from_numpy(np.array(frames)).to(DEV)          # a copy: the cases are read-only


@pytest.mark.parametrize("name", jc.names())
def test_device_equals_the_recorded_bytes(name):
    frame, q, want = jc.case(name)
    got = jpeg.encode_jpeg_device(_dev(frame[None]), q)
    assert len(got) == 1 and len(got[0]) == len(want) and got[0] == want


def test_device_equals_the_recorded_hash_of_the_full_size_case():
    frame, q, sha, length = jc.full_case()
    got = jpeg.encode_jpeg_device(_dev(frame[None]), q)
    assert [len(g) for g in got] == [length] and jc.sha256(got[0]) == sha


@pytest.mark.parametrize("h,w,q,seed", [(45, 100, 60, 11), (33, 523, 90, 12)])
def test_device_equals_the_host_twin_without_a_fixture(h, w, q, seed):
    gen = jc.generator()
    frame = gen.smooth(seed, h, w)
    frame[h // 3:2 * h // 3, w // 4:3 * w // 4] = gen.noise(seed, h, w)[h // 3:2 * h // 3, w // 4:3 * w // 4]
    got = jpeg.encode_jpeg_device(_dev(frame[None]), q)
    assert got == [jpeg.encode_jpeg_host(frame, q)]
    assert jc.decode(got[0]).shape == (h, w, 3)


def test_frames_of_a_batch_are_encoded_as_when_alone():
    frame, q, want = jc.case("noise_19x37_q95")
    batch = np.stack([frame, frame[::-1], frame[:, ::-1]])
    together = jpeg.encode_jpeg_device(_dev(batch), q)
    alone = [jpeg.encode_jpeg_device(_dev(batch[i:i + 1]), q)[0] for i in range(3)]
    assert together == alone and together[0] == want and len(set(together)) == 3
    assert jpeg.encode_jpeg_device(_dev(batch[:0]), q) == []


def _overflow_batch():
    noise, q, _ = jc.case("noise_16x16_q100")
    return np.stack([noise, np.full((16, 16, 3), 99, dtype=np.uint8), np.ascontiguousarray(noise[::-1])]), q


def test_a_frame_that_outgrows_its_slot_fails_alone_and_writes_nothing_outside():
    batch, q = _overflow_batch()
    raw_row = 8 * 3 * 16
    r = jc.run_op(batch, q, slot_bytes=raw_row)
    assert r.fences_ok and r.tail_ok
    assert list(r.status) == [1, 0, 1]
    want = jpeg.encode_jpeg_host(batch[1], q)
    assert list(r.offsets) == [0, 0, len(want), len(want)]
    assert r.file(1) == want
    # through the Python entry the failed frames come from the host twin: three valid files
    got = jpeg.encode_jpeg_device(_dev(batch), q, slot_bytes=raw_row)
    assert got == [jpeg.encode_jpeg_host(f, q) for f in batch]
    assert got == jpeg.encode_jpeg_device(_dev(batch), q)                # the default slots hold the noise


def test_a_frame_that_would_pass_out_cap_fails_alone():
    frame, q, want = jc.case("noise_19x37_q95")
    batch = np.stack([frame, frame[::-1], frame[:, ::-1]])
    wants = [jpeg.encode_jpeg_host(f, q) for f in batch]
    need = sum(len(w) for w in wants)
    exact = jc.run_op(batch, q, out_cap=need)
    assert exact.fences_ok and list(exact.status) == [0, 0, 0] and [exact.file(i) for i in range(3)] == wants
    short = jc.run_op(batch, q, out_cap=need - 1)
    assert short.fences_ok and short.tail_ok
    assert list(short.status) == [0, 0, 2]
    assert list(short.offsets) == [0, len(wants[0]), len(wants[0]) + len(wants[1]), len(wants[0]) + len(wants[1])]
    assert [short.file(i) for i in range(2)] == wants[:2]
    # a frame in the middle that does not fit leaves room for a smaller one behind it
    small = np.full((19, 37, 3), 7, dtype=np.uint8)
    mixed = np.stack([frame, frame[::-1], small])
    w_small = jpeg.encode_jpeg_host(small, q)
    r = jc.run_op(mixed, q, out_cap=len(wants[0]) + len(w_small))
    assert r.fences_ok and r.tail_ok and list(r.status) == [0, 2, 0] and r.file(0) == wants[0] and r.file(2) == w_small


# ---------------------------------------------------------------------------------------------------------------- the wiring
@pytest.fixture(scope="module")
def gpu_net(recipe_sd):
    from calipsync_amd.unet import Model
    m = Model(6, "hubert").to(DEV)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe_sd.items()})
    return m.eval()


def test_result_jpeg_is_the_host_twins_encoding_of_result(gpu_net):
    imgs, lms, masks = make_frames(5, 270, 360, seed=17)
    wd = torch.from_numpy(np.random.default_rng(3).standard_normal((4, 32, 32, 32)).astype(np.float32)).to(DEV)
    clip = ResidentClip(imgs, lms, masks, DEV)
    indices = [3, 0, 4, 3]
    frames = clip.submit(gpu_net, indices, windows=wd).result()
    assert any(not np.array_equal(f, imgs[i]) for f, i in zip(frames, indices))          # something was synthesised
    pending = clip.submit(gpu_net, indices, windows=wd, download=False)
    files = pending.result_jpeg(95)
    assert pending._host is None                                                         # the raw download was not run
    assert files == [jpeg.encode_jpeg_host(f, 95) for f in frames]
    assert clip.fetch([1, 2], download=False).result_jpeg(60) == [jpeg.encode_jpeg_host(imgs[i], 60) for i in (1, 2)]
    clip.close()


def test_frame_synthesizer_yields_jpeg_in_place_of_frames(gpu_net, tmp_path):
    write_dataset(str(tmp_path), 10, 270, 360, seed=4)
    feats = np.random.default_rng(5).standard_normal((11, 2, 1024)).astype(np.float32)
    make = lambda **kw: FrameSynthesizer(None, str(tmp_path), device=DEV, batch_size=4, seed=9, net=gpu_net, resident=True, **kw)
    for sync in (True, False):
        want = list(make().iterate_synthesized_frames(feats, 0, sync))
        got = list(make(output="jpeg", jpeg_quality=90).iterate_synthesized_frames(feats, 0, sync))
        assert all(set(o) == {"jpeg", "index", "physical_index"} for o in got)
        assert [(o["index"], o["physical_index"]) for o in got] == [(o["index"], o["physical_index"]) for o in want]
        assert len(got) == 11 and [o["jpeg"] for o in got] == [jpeg.encode_jpeg_host(o["frame"], 90) for o in want]
    with pytest.raises(ValueError, match="resident"):
        FrameSynthesizer(None, str(tmp_path), device=DEV, net=gpu_net, output="jpeg")


def test_video_stream_manager_writes_the_avi_from_the_device_bytes(gpu_net, tmp_path, capsys):
    data = tmp_path / "data"
    data.mkdir()
    write_dataset(str(data), 6, 270, 360, seed=4)
    feats = np.random.default_rng(6).standard_normal((7, 2, 1024)).astype(np.float32)
    np.save(str(tmp_path / "audio.npy"), feats)
    kw = dict(device=DEV, batch_size=4, seed=2, net=gpu_net, resident=True)
    vsm = VideoStreamManager(str(data), None, **kw, output="jpeg")
    out = vsm.process_single_file(str(tmp_path / "audio.npy"), str(tmp_path / "result.mp4"))
    assert out == str(tmp_path / "result.avi") and os.path.exists(out) and "NO audio track" in capsys.readouterr().out
    want = [jpeg.encode_jpeg_host(o["frame"], 95)
            for o in FrameSynthesizer(None, str(data), **kw).iterate_synthesized_frames(feats, 0, True)]
    raw = open(out, "rb").read()
    at = 0
    for w in want:                                                                       # the chunks are those bytes, in order
        at = raw.index(b"00dc" + len(w).to_bytes(4, "little") + w, at) + 8 + len(w)
    fps, frames = mjpeg_avi.read_mjpeg_avi(out)
    assert fps == 25 and len(frames) == 7 and frames[0].shape == (270, 360, 3)
