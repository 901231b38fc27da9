"""-m gpu: the device 4:2:0 JPEG encoder (csrc/jpeg_enc420.hip) against the recorded libjpeg-turbo bytes and the numpy twin, its
failure statuses behind fences, and the `subsampling` keyword through the resident clip, FrameSynthesizer and VideoStreamManager.
Byte equality throughout."""
import os

import numpy as np
import pytest
import torch

import jpeg420_cases as j4
import jpeg_cases as jc
from calipsync_amd import jpeg, mjpeg_avi
from calipsync_amd.frame_synth import FrameSynthesizer, VideoStreamManager
from calipsync_amd.resident_clip import ResidentClip
from frame_data import make_frames, write_dataset

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SUB = j4.SUB


def _dev(frames):
    return torch.from_numpy(np.array(frames)).to(DEV)          # a copy: the cases are read-only


@pytest.mark.parametrize("name", j4.names())
def test_device_equals_the_recorded_bytes(name):
    frame, q, want = j4.case(name)
    r = j4.run_op(frame[None], q)
    assert r.fences_ok and r.tail_ok and list(r.status) == [0] and list(r.offsets) == [0, len(want)]
    assert r.file(0) == want
    got = jpeg.encode_jpeg_device(_dev(frame[None]), q, subsampling=SUB)
    assert len(got) == 1 and len(got[0]) == len(want) and got[0] == want


def test_device_equals_the_recorded_hash_of_two_full_size_frames_in_one_batch():
    frame, q, sha, length = j4.full_case()
    got = jpeg.encode_jpeg_device(_dev(np.stack([frame, frame])), q, subsampling=SUB)
    assert [len(g) for g in got] == [length, length] and [jc.sha256(g) for g in got] == [sha, sha]


# no fixture: 1 x 1; one short of and one past whole MCUs both ways; right, bottom and both kinds of dummies; rows of more than
# the 32 MCUs a wave takes at a time: exactly two passes (8 x 1024), a third that ends in dummies (24 x 1048: 66 MCUs; 17 x 1025)
# and five (40 x 2064: 129 MCUs)
SHAPES = [(1, 1, 95, 21), (15, 17, 10, 22), (31, 18, 50, 23), (24, 1048, 95, 24), (40, 2064, 100, 25), (16, 16, 100, 26), (33, 47, 50, 27),
          (8, 1024, 10, 28), (130, 9, 95, 29), (17, 1025, 50, 30)]


@pytest.mark.parametrize("h,w,q,seed", SHAPES)
def test_device_equals_the_host_twin_without_a_fixture(h, w, q, seed):
    frame, want = j4.seeded(h, w, seed), j4.twin(h, w, seed, q)
    r = j4.run_op(frame[None], q)
    assert r.fences_ok and r.tail_ok and list(r.status) == [0]
    assert r.file(0) == want
    assert jc.decode(r.file(0)).shape == (h, w, 3)


def test_frames_of_a_batch_are_encoded_as_when_alone():
    frame, q, want = j4.case("noise_19x37_q95")
    batch = np.stack([frame, frame[::-1], frame[:, ::-1]])
    together = jpeg.encode_jpeg_device(_dev(batch), q, subsampling=SUB)
    alone = [jpeg.encode_jpeg_device(_dev(batch[i:i + 1]), q, subsampling=2)[0] for i in range(3)]
    assert together == alone and together[0] == want and len(set(together)) == 3
    assert jpeg.encode_jpeg_device(_dev(batch[:0]), q, subsampling=SUB) == []


def test_a_frame_that_outgrows_its_slot_fails_alone_and_writes_nothing_outside():
    noise, q, _ = j4.case("noise_32x32_q100")
    batch = np.stack([noise, np.full((32, 32, 3), 99, dtype=np.uint8), np.ascontiguousarray(noise[::-1])])
    raw_row = 384 * 2                                                    # the raw bytes an MCU row of 32 pixels codes
    r = j4.run_op(batch, q, slot_bytes=raw_row)
    assert r.fences_ok and r.tail_ok
    assert list(r.status) == [1, 0, 1]
    want = jpeg.encode_jpeg_host(batch[1], q, SUB)
    assert list(r.offsets) == [0, 0, len(want), len(want)]
    assert r.file(1) == want
    # through the Python entry the failed frames come from the host twin: three valid files
    got = jpeg.encode_jpeg_device(_dev(batch), q, subsampling=SUB, slot_bytes=raw_row)
    assert got == [jpeg.encode_jpeg_host(f, q, SUB) for f in batch]
    assert got == jpeg.encode_jpeg_device(_dev(batch), q, subsampling=SUB)          # the default slots hold the noise


def test_a_frame_that_would_pass_out_cap_fails_alone():
    frame, q, want = j4.case("noise_19x37_q95")
    batch = np.stack([frame, frame[::-1], frame[:, ::-1]])
    wants = [jpeg.encode_jpeg_host(f, q, SUB) for f in batch]
    need = sum(len(w) for w in wants)
    exact = j4.run_op(batch, q, out_cap=need)
    assert exact.fences_ok and list(exact.status) == [0, 0, 0] and [exact.file(i) for i in range(3)] == wants
    short = j4.run_op(batch, q, out_cap=need - 1)
    assert short.fences_ok and short.tail_ok
    assert list(short.status) == [0, 0, 2]
    assert list(short.offsets) == [0, len(wants[0]), len(wants[0]) + len(wants[1]), len(wants[0]) + len(wants[1])]
    assert [short.file(i) for i in range(2)] == wants[:2]


# ---------------------------------------------------------------------------------------------------------------- the wiring
@pytest.fixture(scope="module")
def gpu_net(recipe_sd):
    from calipsync_amd.unet import Model
    m = Model(6, "hubert").to(DEV)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe_sd.items()})
    return m.eval()


def test_result_jpeg_is_the_host_twins_encoding_of_result(gpu_net):
    imgs, lms, masks = make_frames(5, 270, 360, seed=17)                 # 270 = 16 * 16 + 14, 360 = 22 * 16 + 8: right dummies
    wd = torch.from_numpy(np.random.default_rng(3).standard_normal((4, 32, 32, 32)).astype(np.float32)).to(DEV)
    clip = ResidentClip(imgs, lms, masks, DEV)
    indices = [3, 0, 4, 3]
    frames = clip.submit(gpu_net, indices, windows=wd).result()
    pending = clip.submit(gpu_net, indices, windows=wd, download=False)
    files = pending.result_jpeg(95, subsampling=SUB)
    assert pending._host is None                                                         # the raw download was not run
    assert files == [jpeg.encode_jpeg_host(f, 95, SUB) for f in frames]
    assert pending.result_jpeg(95) == [jpeg.encode_jpeg_host(f, 95) for f in frames]     # no keyword: 4:4:4, as before
    assert pending.result_jpeg(95) == pending.result_jpeg(95, "4:4:4") and files == pending.result_jpeg(95, 2)
    assert clip.fetch([1, 2], download=False).result_jpeg(60, SUB) == [jpeg.encode_jpeg_host(imgs[i], 60, SUB) for i in (1, 2)]
    clip.close()


def test_frame_synthesizer_yields_420_files(gpu_net, tmp_path):
    write_dataset(str(tmp_path), 6, 270, 360, seed=4)
    feats = np.random.default_rng(5).standard_normal((7, 2, 1024)).astype(np.float32)
    make = lambda **kw: FrameSynthesizer(None, str(tmp_path), device=DEV, batch_size=4, seed=9, net=gpu_net, resident=True, **kw)
    want = list(make().iterate_synthesized_frames(feats, 0, True))
    got = list(make(output="jpeg", jpeg_quality=90, jpeg_subsampling=SUB).iterate_synthesized_frames(feats, 0, True))
    assert all(set(o) == {"jpeg", "index", "physical_index"} for o in got)
    assert [(o["index"], o["physical_index"]) for o in got] == [(o["index"], o["physical_index"]) for o in want]
    assert len(got) == 7 and [o["jpeg"] for o in got] == [jpeg.encode_jpeg_host(o["frame"], 90, SUB) for o in want]


def test_video_stream_manager_writes_an_avi_of_420_frames(gpu_net, tmp_path, capsys):
    data = tmp_path / "data"
    data.mkdir()
    write_dataset(str(data), 6, 270, 360, seed=4)
    feats = np.random.default_rng(6).standard_normal((7, 2, 1024)).astype(np.float32)
    np.save(str(tmp_path / "audio.npy"), feats)
    kw = dict(device=DEV, batch_size=4, seed=2, net=gpu_net, resident=True)
    vsm = VideoStreamManager(str(data), None, **kw, output="jpeg", jpeg_subsampling=SUB)
    out = vsm.process_single_file(str(tmp_path / "audio.npy"), str(tmp_path / "result.mp4"))
    assert out == str(tmp_path / "result.avi") and os.path.exists(out)
    want = [jpeg.encode_jpeg_host(o["frame"], 95, SUB)
            for o in FrameSynthesizer(None, str(data), **kw).iterate_synthesized_frames(feats, 0, True)]
    raw = open(out, "rb").read()
    at = 0
    for w in want:                                                                       # the chunks are those bytes, in order
        at = raw.index(b"00dc" + len(w).to_bytes(4, "little") + w, at) + 8 + len(w)
    fps, frames = mjpeg_avi.read_mjpeg_avi(out)                                          # Pillow decodes every chunk
    assert fps == 25 and len(frames) == 7 and all(f.shape == (270, 360, 3) for f in frames)
