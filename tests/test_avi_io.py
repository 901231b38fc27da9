"""The AVI container on the host (no GPU): mjpeg_avi.write_mjpeg_avi with and without a PCM sound track, mjpeg_avi.read_avi on
its files and on hand-built files of the kinds other writers produce, and VideoStreamManager(audio_track="pcm") on its no-cv2
branch.  The layouts are assembled here with struct from the AVI documentation, not taken from the code under test."""
import os
import struct
import sys
import wave

import numpy as np
import pytest

from calipsync_amd import audio, mjpeg_avi

H, W = 16, 24


def _jpeg(seed, h=H, w=W, **kw):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(buf, format="JPEG", **kw)
    return buf.getvalue()


FRAMES = [_jpeg(i) for i in range(7)]          # odd and even lengths among them
assert {len(f) & 1 for f in FRAMES} == {0, 1}


def chunk(cc, body):
    return cc + struct.pack("<I", len(body)) + bytes(body) + (b"\0" if len(body) & 1 else b"")


def lst(kind, body):
    return b"LIST" + struct.pack("<I", len(body) + 4) + kind + body


def video_strl(n, biggest, rate=25000, scale=1000, fourcc=b"MJPG", w=W, h=H, extra=b""):
    strh = b"vids" + fourcc + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, scale, rate, 0, n, biggest, 0xFFFFFFFF, 0, 0, 0, w, h)
    strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, fourcc, w * h * 3, 0, 0, 0, 0)
    return lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf) + extra)


def audio_strl(n, channels=1, rate=16000, width=2, tag=1):
    align = channels * width
    strh = b"auds" + bytes(4) + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, 1, rate, 0, n, 0, 0xFFFFFFFF, align, 0, 0, 0, 0)
    return lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, 8 * width)))


def avi(strls, movi, n, biggest, fps=25.0, streams=1, flags=0x10, index=None, form=b"AVI ", tail=b""):
    """a whole file: hdrl (avih + the stream lists), the movi list, idx1 (None: left out)"""
    avih = struct.pack("<14I", int(round(1e6 / fps)), int(biggest * fps), 0, flags, n, 0, streams, biggest, W, H, 0, 0, 0, 0)
    body = form + lst(b"hdrl", chunk(b"avih", avih) + strls) + lst(b"movi", movi) + (b"" if index is None else chunk(b"idx1", index))
    return b"RIFF" + struct.pack("<I", len(body)) + body + tail


def silent_file(frames, fps=25.0):
    """the layout write_mjpeg_avi has written since before it knew of sound: one MJPG stream, 00dc chunks, idx1 from 'movi'"""
    movi, index, off = b"", b"", 4
    for f in frames:
        index += b"00dc" + struct.pack("<III", 0x10, off, len(f))
        c = chunk(b"00dc", f)
        movi += c
        off += len(c)
    biggest = max(len(f) for f in frames)
    return avi(video_strl(len(frames), biggest, int(round(fps * 1000))), movi, len(frames), biggest, fps, index=index)


def write(tmp_path, data, name="clip.avi"):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def pcm_of(seed, n, channels, width):
    lo, hi = {1: (0, 256), 2: (-32768, 32768), 3: (-(1 << 23), 1 << 23), 4: (-(1 << 31), 1 << 31)}[width]
    return np.random.default_rng(seed).integers(lo, hi, (n, channels)).astype({1: np.uint8, 2: np.int16}.get(width, np.int32))


def chunks_of(data):
    """[(fourcc, body)] of the movi list of a file, in order"""
    at = data.index(b"movi") - 8
    size = struct.unpack_from("<I", data, at + 4)[0]
    out, pos = [], at + 12
    while pos < at + 8 + size:
        n = struct.unpack_from("<I", data, pos + 4)[0]
        out.append((data[pos:pos + 4], data[pos + 8:pos + 8 + n]))
        assert pos % 2 == 0                                      # every chunk on an even offset
        pos += 8 + n + (n & 1)
    assert pos == at + 8 + size
    return out


# ---------------------------------------------------------------------------------------------------------------- the writer
@pytest.mark.parametrize("fps", [25.0, 29.97])
def test_without_audio_the_file_is_byte_for_byte_the_old_one(tmp_path, fps):
    p = str(tmp_path / "a.avi")
    assert mjpeg_avi.write_mjpeg_avi(p, FRAMES, fps=fps, audio=None) == len(FRAMES)
    assert open(p, "rb").read() == silent_file(FRAMES, fps)
    q = str(tmp_path / "b.avi")
    mjpeg_avi.write_mjpeg_avi(q, FRAMES, fps=fps)
    assert open(q, "rb").read() == silent_file(FRAMES, fps)


def test_the_header_fields_of_a_file_with_audio(tmp_path):
    rate, channels, width = 44100, 2, 3
    pcm = pcm_of(1, 12345, channels, width)
    p = str(tmp_path / "a.avi")
    mjpeg_avi.write_mjpeg_avi(p, FRAMES, fps=29.97, audio=(pcm, rate, width))
    data = open(p, "rb").read()
    assert data[:4] == b"RIFF" and struct.unpack_from("<I", data, 4)[0] == len(data) - 8 and data[8:12] == b"AVI "
    assert data[24:28] == b"avih"
    avih = struct.unpack_from("<14I", data, 32)
    assert avih[3] == 0x10 | 0x100 and avih[4] == len(FRAMES) and avih[6] == 2 and avih[8:10] == (W, H)      # HASINDEX | ISINTERLEAVED; dwStreams
    assert data[100:104] == b"strh" and data[108:116] == b"vidsMJPG"                                    # the video strl is still first
    v = struct.unpack_from("<IHHIIIIIIII4H", data, 116)
    assert (v[4], v[5], v[7]) == (1000, 29970, len(FRAMES))
    at = 88 + 12 + 64 + 48                                       # behind the video strl: LIST strl of the audio stream
    assert at == 212 and data[at:at + 4] == b"LIST" and data[at + 8:at + 16] == b"strlstrh" and data[at + 20:at + 28] == b"auds" + bytes(4)
    a = struct.unpack_from("<IHHIIIIIIII4H", data, at + 28)
    align = channels * width
    assert (a[4], a[5], a[6], a[7], a[9], a[10]) == (1, rate, 0, 12345, 0xFFFFFFFF, align)      # dwScale, dwRate, dwStart, dwLength, quality, dwSampleSize
    sf = at + 20 + 56
    assert data[sf:sf + 4] == b"strf" and struct.unpack_from("<I", data, sf + 4)[0] == 16
    assert struct.unpack_from("<HHIIHH", data, sf + 8) == (1, channels, rate, rate * align, align, 8 * width)
    movi = data.index(b"movi")
    assert data[movi - 8:movi - 4] == b"LIST" and movi - 8 == sf + 8 + 16
    found = chunks_of(data)
    assert a[8] == max(len(b) for cc, b in found if cc == b"01wb")                                  # dwSuggestedBufferSize
    idx = data.index(b"idx1", movi + struct.unpack_from("<I", data, movi - 4)[0] - 4)
    n_idx = struct.unpack_from("<I", data, idx + 4)[0] // 16
    assert n_idx == len(found) and idx + 8 + 16 * n_idx == len(data)
    for i, (cc, body) in enumerate(found):
        e_cc, flags, off, size = struct.unpack_from("<4sIII", data, idx + 8 + 16 * i)
        assert e_cc == cc and cc in (b"00dc", b"01wb") and flags == 0x10 and size == len(body)
        assert data[movi + off:movi + off + 4] == cc and struct.unpack_from("<I", data, movi + off + 4)[0] == size
        assert (movi + off) % 2 == 0


@pytest.mark.parametrize("fps", [25.0, 29.97])
@pytest.mark.parametrize("channels,rate,width", [(1, 16000, 2), (2, 44100, 3)])
@pytest.mark.parametrize("length", ["equal", "longer", "shorter"])
def test_audio_round_trips_and_its_chunks_follow_the_formula(tmp_path, fps, channels, rate, width, length):
    n = len(FRAMES)
    vrate, scale = int(round(fps * 1000)), 1000
    exact = n * rate * scale // vrate
    total = {"equal": exact, "longer": exact + rate // 3 + 1, "shorter": 2 * rate * scale // vrate + 5}[length]
    pcm = pcm_of(7, total, channels, width)
    p = str(tmp_path / "a.avi")
    mjpeg_avi.write_mjpeg_avi(p, FRAMES, fps=fps, audio=(pcm, rate, width))
    data = open(p, "rb").read()
    align = channels * width
    want, k = [], 0                                              # the chunk sequence the formula gives
    for i in range(n):
        want.append((b"00dc", len(FRAMES[i])))
        end = min((i + 1) * rate * scale // vrate, total)
        if end > k:
            want.append((b"01wb", (end - k) * align))
            k = end
    if k < total:
        want.append((b"01wb", (total - k) * align))
    assert [(cc, len(b)) for cc, b in chunks_of(data)] == want
    assert b"".join(b for cc, b in chunks_of(data) if cc == b"01wb") == audio.pcm_bytes(pcm, width).tobytes()
    clip = mjpeg_avi.read_avi(p, audio="require")
    assert (clip.fps, clip.rate, clip.scale, clip.width, clip.height) == (vrate / scale, vrate, scale, W, H) and clip.notes == []
    assert [bytes(f) for f in clip.frames] == FRAMES and len(clip) == n
    got, got_rate, got_width = clip.audio
    assert (got_rate, got_width) == (rate, width) and got.shape == pcm.shape and got.dtype == pcm.dtype and (got == pcm).all()
    assert len(mjpeg_avi.read_mjpeg_avi(p)[1]) == n             # the old helper still finds the frames (its fps is the last strh's)


def test_audio_from_a_wav_path_and_what_the_writer_refuses(tmp_path):
    pcm = pcm_of(3, 4000, 2, 2)
    wav = str(tmp_path / "a.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(2), w.setsampwidth(2), w.setframerate(22050)
        w.writeframes(audio.pcm_bytes(pcm, 2).tobytes())
    p = str(tmp_path / "a.avi")
    mjpeg_avi.write_mjpeg_avi(p, FRAMES, audio=wav)
    got, rate, width = mjpeg_avi.read_avi(p).audio
    assert (rate, width) == (22050, 2) and (got == pcm).all()
    mjpeg_avi.write_mjpeg_avi(p, FRAMES, audio=(pcm_of(4, 999, 1, 1), 8000, 1))            # 8-bit offset binary, 32-bit
    assert (mjpeg_avi.read_avi(p).audio[0] == pcm_of(4, 999, 1, 1)).all()
    mjpeg_avi.write_mjpeg_avi(p, FRAMES, audio=(pcm_of(5, 999, 3, 4), 48000, 4))
    assert (mjpeg_avi.read_avi(p).audio[0] == pcm_of(5, 999, 3, 4)).all()
    q = str(tmp_path / "never.avi")
    for bad in ((pcm.astype(np.float32), 22050, 2), (pcm, 22050, 5), (pcm, 0, 2), (pcm.reshape(10, 20, -1), 22050, 2), 17):
        with pytest.raises(ValueError):
            mjpeg_avi.write_mjpeg_avi(q, FRAMES, audio=bad)
        assert not os.path.exists(q)


def test_the_4_gib_error_counts_the_audio_and_removes_the_partial_file(tmp_path, monkeypatch):
    pcm = pcm_of(9, 16000, 1, 2)
    p = str(tmp_path / "a.avi")
    mjpeg_avi.write_mjpeg_avi(p, FRAMES, audio=(pcm, 16000, 2))
    whole = os.path.getsize(p)
    silent = len(silent_file(FRAMES))
    os.remove(p)
    monkeypatch.setattr(mjpeg_avi, "RIFF_LIMIT", whole)          # it fits exactly
    mjpeg_avi.write_mjpeg_avi(p, FRAMES, audio=(pcm, 16000, 2))
    os.remove(p)
    for limit in (whole - 1, silent + 1000, 600):                # the audio chunks and their index entries count
        monkeypatch.setattr(mjpeg_avi, "RIFF_LIMIT", limit)
        with pytest.raises(ValueError, match="4 GiB"):
            mjpeg_avi.write_mjpeg_avi(p, FRAMES, audio=(pcm, 16000, 2))
        assert not os.path.exists(p)
    monkeypatch.setattr(mjpeg_avi, "RIFF_LIMIT", silent)
    mjpeg_avi.write_mjpeg_avi(p, FRAMES)                         # the silent file's limit is where it was
    os.remove(p)
    monkeypatch.setattr(mjpeg_avi, "RIFF_LIMIT", silent - 1)
    with pytest.raises(ValueError, match="4 GiB"):
        mjpeg_avi.write_mjpeg_avi(p, FRAMES)
    assert not os.path.exists(p)

    def failing():
        yield FRAMES[0]
        raise RuntimeError("the synthesizer broke")

    monkeypatch.setattr(mjpeg_avi, "RIFF_LIMIT", 1 << 30)
    with pytest.raises(RuntimeError):
        mjpeg_avi.write_mjpeg_avi(p, failing(), audio=(pcm, 16000, 2))
    assert not os.path.exists(p)


# ---------------------------------------------------------------------------------------------------------------- the reader
def _movi(items):
    return b"".join(chunk(cc, body) for cc, body in items)


def test_rec_lists_junk_and_odd_chunks(tmp_path):
    pcm = pcm_of(2, 300, 1, 2)
    raw = audio.pcm_bytes(pcm, 2).tobytes()
    rec = lambda i: lst(b"rec ", chunk(b"00dc", FRAMES[i]) + chunk(b"01wb", raw[200 * i:200 * (i + 1)]))
    movi = chunk(b"JUNK", b"x" * 7) + rec(0) + chunk(b"JUNK", b"") + rec(1) + rec(2) + chunk(b"ix00", b"y" * 9)
    strls = video_strl(3, 999, extra=chunk(b"JUNK", b"z" * 5)) + chunk(b"JUNK", b"pad") + audio_strl(300)
    clip = mjpeg_avi.read_avi(write(tmp_path, avi(strls, movi, 3, 999, streams=2, index=b"garbage that is not an index")))
    assert [bytes(f) for f in clip.frames] == FRAMES[:3] and (clip.audio[0] == pcm).all() and clip.audio[1:] == (16000, 2)
    assert clip.fps == 25.0 and (clip.width, clip.height) == (W, H)


def test_the_audio_stream_first(tmp_path):
    pcm = pcm_of(2, 100, 2, 2)
    raw = audio.pcm_bytes(pcm, 2).tobytes()
    movi = _movi([(b"00wb", raw[:200]), (b"01dc", FRAMES[0]), (b"01dc", FRAMES[1]), (b"00wb", raw[200:])])
    clip = mjpeg_avi.read_avi(write(tmp_path, avi(audio_strl(100, 2) + video_strl(2, 999, 30000, 1001), movi, 2, 999, streams=2)))
    assert [bytes(f) for f in clip.frames] == FRAMES[:2] and (clip.audio[0] == pcm).all() and clip.fps == 30000 / 1001


def test_a_zero_length_frame_is_the_frame_before_it(tmp_path):
    movi = _movi([(b"00dc", FRAMES[0]), (b"00dc", b""), (b"00dc", FRAMES[2])])
    clip = mjpeg_avi.read_avi(write(tmp_path, avi(video_strl(3, 999), movi, 3, 999)))
    assert [bytes(f) for f in clip.frames] == [FRAMES[0], FRAMES[0], FRAMES[2]] and "frame 1 was dropped" in clip.notes[0]
    with pytest.raises(ValueError, match="frame 0 is empty"):
        mjpeg_avi.read_avi(write(tmp_path, avi(video_strl(2, 999), _movi([(b"00dc", b""), (b"00dc", FRAMES[0])]), 2, 999)))


def test_a_file_cut_off_mid_recording(tmp_path):
    whole = silent_file(FRAMES)
    at = whole.index(b"idx1")
    assert [bytes(f) for f in mjpeg_avi.read_avi(write(tmp_path, whole[:at])).frames] == FRAMES          # no idx1
    last = whole.rindex(b"00dc", 0, at)                                                                # the last frame's chunk
    for cut in (last + 8 + len(FRAMES[-1]) // 2, last + 8, last + 5):                                  # inside its body, its size
        clip = mjpeg_avi.read_avi(write(tmp_path, whole[:cut]))
        assert [bytes(f) for f in clip.frames] == FRAMES[:-1]
    # the sizes a recorder leaves when it never came back to patch them: RIFF and movi run past the end, or are zero
    for riff, movi_size in ((0xFFFFFFF0, 0x7FFFFFF0), (0, 0)):
        data = bytearray(whole[:last + 8 + 3])
        struct.pack_into("<I", data, 4, riff)
        struct.pack_into("<I", data, whole.index(b"movi") - 4, movi_size)
        clip = mjpeg_avi.read_avi(write(tmp_path, bytes(data)))
        assert [bytes(f) for f in clip.frames] == FRAMES[:-1]
    with pytest.raises(ValueError, match="not a RIFF/AVI"):
        mjpeg_avi.read_avi(write(tmp_path, b"RIFX" + whole[4:]))


def test_another_codec_is_named(tmp_path):
    movi = _movi([(b"00dc", FRAMES[0])])
    with pytest.raises(ValueError, match="'H264'.*not Motion-JPEG"):
        mjpeg_avi.read_avi(write(tmp_path, avi(video_strl(1, 999, fourcc=b"H264"), movi, 1, 999)))
    clip = mjpeg_avi.read_avi(write(tmp_path, avi(video_strl(1, 999, fourcc=b"mjpg"), movi, 1, 999)))          # case-insensitive
    assert bytes(clip.frames[0]) == FRAMES[0]


def test_opendml_files_are_refused(tmp_path):
    movi = _movi([(b"00dc", FRAMES[0])])
    more = b"RIFF" + struct.pack("<I", 4 + 12 + len(movi)) + b"AVIX" + lst(b"movi", movi)
    with pytest.raises(ValueError, match="OpenDML"):
        mjpeg_avi.read_avi(write(tmp_path, avi(video_strl(1, 999), movi, 1, 999, tail=more)))
    with pytest.raises(ValueError, match="OpenDML"):
        mjpeg_avi.read_avi(write(tmp_path, avi(video_strl(1, 999, extra=chunk(b"indx", bytes(24))), movi, 1, 999, tail=more)))
    with pytest.raises(ValueError, match="OpenDML"):
        mjpeg_avi.read_avi(write(tmp_path, more))
    # an indx chunk in a file that ends with its first RIFF is an ordinary AVI with one more index
    clip = mjpeg_avi.read_avi(write(tmp_path, avi(video_strl(1, 999, extra=chunk(b"indx", bytes(24))), movi, 1, 999)))
    assert len(clip) == 1


def test_audio_that_is_not_pcm(tmp_path):
    movi = _movi([(b"00dc", FRAMES[0]), (b"01wb", b"\x01\x02\x03\x04")])
    p = write(tmp_path, avi(video_strl(1, 999) + audio_strl(2, tag=0x55), movi, 1, 999, streams=2))          # MP3
    clip = mjpeg_avi.read_avi(p)
    assert clip.audio is None and len(clip) == 1 and "not PCM" in clip.notes[0] and "0x55" in clip.notes[0]
    with pytest.raises(ValueError, match="not PCM.*0x55"):
        mjpeg_avi.read_avi(p, audio="require")
    with pytest.raises(ValueError, match="no audio stream"):
        mjpeg_avi.read_avi(write(tmp_path, silent_file(FRAMES)), audio="require")
    with pytest.raises(ValueError, match="audio"):
        mjpeg_avi.read_avi(p, audio="maybe")


def test_a_frame_of_another_size_is_named(tmp_path):
    field = _jpeg(50, H // 2, W)                                 # what an interlaced two-field stream holds
    movi = _movi([(b"00dc", FRAMES[0]), (b"00dc", FRAMES[1]), (b"00dc", field)])
    with pytest.raises(ValueError, match=f"frame 2 is a JPEG of {H // 2} x {W}.*{H} x {W}"):
        mjpeg_avi.read_avi(write(tmp_path, avi(video_strl(3, 999), movi, 3, 999)))
    with pytest.raises(ValueError, match="frame 1.*no SOI"):
        mjpeg_avi.read_avi(write(tmp_path, avi(video_strl(2, 999), _movi([(b"00dc", FRAMES[0]), (b"00dc", b"not a jpeg")]), 2, 999)))


# ---------------------------------------------------------------------------------------------------------------- the manager
class _StubSynthesizer:
    """what VideoStreamManager needs of a FrameSynthesizer: output, and frames for features"""
    calls = 0

    def __init__(self, **kw):
        self.output = kw.get("output", "frames")

    def iterate_synthesized_frames(self, features, start, flag):
        type(self).calls += 1
        for i in range(len(features)):
            frame = np.full((H, W, 3), 10 * i, dtype=np.uint8)
            yield {"frame": frame, "jpeg": mjpeg_avi.encode_jpeg(frame)}


@pytest.fixture
def manager(monkeypatch):
    from calipsync_amd import frame_synth
    monkeypatch.setattr(frame_synth, "FrameSynthesizer", _StubSynthesizer)
    monkeypatch.setitem(sys.modules, "cv2", None)                # import cv2 -> ImportError: the no-cv2 branch
    monkeypatch.setattr(_StubSynthesizer, "calls", 0)
    return frame_synth.VideoStreamManager


def _wav(path, pcm, rate, width):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm.shape[1]), w.setsampwidth(width), w.setframerate(rate)
        w.writeframes(audio.pcm_bytes(pcm, width).tobytes())
    return str(path)


@pytest.mark.parametrize("output", ["frames", "jpeg"])
def test_the_manager_writes_the_wav_beside_the_frames(tmp_path, manager, capsys, output):
    feats = np.zeros((5, 2, 1024), dtype=np.float32)
    pcm = pcm_of(11, 5 * 640 + 77, 1, 2)
    wav = _wav(tmp_path / "in.wav", pcm, 16000, 2)
    vsm = manager("data", None, hubert_path=lambda path: feats, audio_track="pcm", output=output)
    out = vsm.process_single_file(wav, str(tmp_path / "out.mp4"))
    assert out == str(tmp_path / "out.avi") and "NO audio track" not in capsys.readouterr().out
    clip = mjpeg_avi.read_avi(out, audio="require")
    assert len(clip) == 5 and clip.fps == 25.0 and clip.audio[1:] == (16000, 2) and (clip.audio[0] == pcm).all()
    # "none", the default, writes the bytes it always wrote
    silent = manager("data", None, hubert_path=lambda path: feats, output=output)
    assert silent.audio_track == "none"
    out2 = silent.process_single_file(wav, str(tmp_path / "silent.mp4"))
    assert "NO audio track" in capsys.readouterr().out
    frames = [np.full((H, W, 3), 10 * i, dtype=np.uint8) for i in range(5)]
    assert open(out2, "rb").read() == silent_file([mjpeg_avi.encode_jpeg(f) for f in frames])


def test_the_manager_refuses_features_and_bad_wavs_before_synthesis(tmp_path, manager):
    feats = np.zeros((3, 2, 1024), dtype=np.float32)
    np.save(tmp_path / "feats.npy", feats)
    vsm = manager("data", None, hubert_path=lambda path: feats, audio_track="pcm")
    with pytest.raises(ValueError, match="audio_track='pcm' needs a PCM WAV"):
        vsm.process_single_file(str(tmp_path / "feats.npy"), str(tmp_path / "out.mp4"))
    (tmp_path / "bad.wav").write_bytes(b"RIFF\x04\0\0\0JUNK")
    with pytest.raises(ValueError, match="not a PCM WAV"):
        vsm.process_single_file(str(tmp_path / "bad.wav"), str(tmp_path / "out.mp4"))
    assert _StubSynthesizer.calls == 0 and not os.path.exists(tmp_path / "out.avi")
    with pytest.raises(ValueError, match="audio_track"):
        manager("data", None, audio_track="aac")
    manager("data", None).process_single_file(str(tmp_path / "feats.npy"), str(tmp_path / "out.mp4"))      # "none" still takes features
    assert _StubSynthesizer.calls == 1
