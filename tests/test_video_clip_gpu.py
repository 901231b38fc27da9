"""-m gpu: ResidentClip.from_video (calipsync_amd/resident_clip.py) on a Motion-JPEG AVI of the kind capture software writes:
4:2:2 frames without their Huffman tables, with a PCM sound track.  The frames decoded on the device, by Pillow on the host and
handed to from_frames as pixels are the same bytes; the sound comes back as it was written."""
import numpy as np
import pytest

import mjpeg_decode_cases as mj
from calipsync_amd import jpeg, landmarks, mjpeg_avi, recipe
from calipsync_amd.resident_clip import ResidentClip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, H, W = 6, 48, 64
BOX = (8, 4, 44, 40)                                            # (x, y, w, h) inside the frame


@pytest.fixture(scope="module")
def detector():
    from frame_data import landmarks as face_shape
    mean_face = face_shape(0.5, 0.45, 0.3, np.random.default_rng(0), jitter=0.0).astype(np.float32).reshape(-1)
    return landmarks.LandmarkDetector(state_dict=recipe.make_pfld_state_dict(), mean_face=mean_face, device=DEV)


def _files():
    gen = mj.generator()
    out = []
    for i in range(N):
        frame = gen.frame("smooth", H, W).copy()
        frame[4 + 3 * i:20 + 3 * i, 8:40] = gen.frame("noise", H, W)[4 + 3 * i:20 + 3 * i, 8:40]
        out.append(gen.strip_dht(gen.pillow_write(frame, "422", quality=95)))
    return out


def test_from_video_holds_the_host_decoders_bytes_and_the_sound(tmp_path, detector):
    files = _files()
    for f in files:
        info = jpeg.parse_jpeg(f, subset="mjpeg")
        assert info.subsampling == 1 and b"\xff\xc4" not in f[:info.scan_offset]
        with pytest.raises(jpeg.JpegUnsupported):
            jpeg.parse_jpeg(f)
    pcm = np.random.default_rng(3).integers(-32768, 32768, (N * 640 + 100, 2)).astype(np.int16)
    path = str(tmp_path / "capture.avi")
    mjpeg_avi.write_mjpeg_avi(path, files, fps=25, audio=(pcm, 16000, 2))
    boxes = [[BOX], [BOX], [BOX], [BOX], None, [BOX]]           # frame 4 has no face
    dev = ResidentClip.from_video(path, detector, chunk=4, boxes=boxes)                      # decode="device" is the default; 4 + 2
    host = ResidentClip.from_video(path, detector, chunk=4, decode="host", boxes=boxes)
    pixels = [jpeg._decode_pillow(f) for f in files]
    ref = ResidentClip.from_frames(pixels, detector, boxes=boxes, chunk=4)
    assert dev.source_index == host.source_index == ref.source_index == [0, 1, 2, 3, 5]
    assert tuple(dev.frames.shape) == (5, H, W, 3) and dev.frames.is_cuda
    assert int((dev.frames != host.frames).sum()) == 0 and int((dev.frames != ref.frames).sum()) == 0
    assert np.array_equal(dev.frames.cpu().numpy(), np.stack([pixels[i] for i in dev.source_index]))
    for a, b, c in zip(dev.landmarks, host.landmarks, ref.landmarks):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    for clip in (dev, host):
        got, rate, width = clip.audio
        assert (rate, width) == (16000, 2) and got.dtype == np.int16 and np.array_equal(got, pcm) and clip.fps == 25.0
    assert ref.audio is None and ref.fps is None
    with pytest.raises(ValueError, match="decode"):
        ResidentClip.from_video(path, detector, decode="gpu")
    silent = str(tmp_path / "silent.avi")
    mjpeg_avi.write_mjpeg_avi(silent, files[:2], fps=30)
    clip = ResidentClip.from_video(silent, detector, boxes=[[BOX], [BOX]])
    assert clip.audio is None and clip.fps == 30.0 and len(clip) == 2
