"""-m gpu: the device JPEG decoder (csrc/jpeg_dec.hip) below and above the ledger's cases: every recorded file at the subsequence
lengths that force late synchronisation (32 bits) and that make one subsequence per restart segment, the public entry
decode_jpeg_device with its host fallback, and the resident clip decoded on the device.  Every comparison is byte equality."""
import os

import numpy as np
import pytest
import torch

import jpeg_decode_cases as jd
from calipsync_amd import jpeg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("chunk_bits", [32, jd.BIG_CHUNK], ids=["chunk32", "one_subsequence"])
@pytest.mark.parametrize("name", jd.names())
def test_every_fixture_case_at_other_subsequence_lengths(name, chunk_bits):
    res = jd.run_op([jd.case(name)[0]], chunk_bits)
    assert res.fences_ok and res.data_ok and list(res.status) == [0]
    diff = jd.differences(res.out[0], name)
    print(f"{name} at chunk_bits {chunk_bits}: {diff:.0f} bytes differ")
    assert diff == 0


def test_the_operator_checks_its_arguments_before_it_launches():
    from calipsync_amd import _lib
    data = jd.case("noise_8x8_default")[0]
    plan = jpeg.plan_decode([data])
    blob = torch.from_numpy(plan.blob.copy()).to(DEV)
    out = torch.full((1, 8, 8, 3), 0x5A, dtype=torch.uint8, device=DEV)
    status = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    scratch = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)

    def call(kw=None):
        p = jpeg.plan_decode([data])
        for k, v in (kw or {}).items():
            if k == "chunk_bits":
                p.chunk_bits = v
            else:
                p.rec[0, k] = v
        jpeg.decode_jpeg_op(p, blob, scratch, out, status, 8, 8)

    for bad in ({0: blob.numel()}, {1: blob.numel() + 1}, {4: 2}, {5: blob.numel() - 4}, {6: blob.numel() - 8}, {7: 1000}, {8: 1}, {2: 1},
                {"chunk_bits": 48}):
        with pytest.raises(RuntimeError, match="jpegdec_decode"):
            call(bad)
    with pytest.raises(RuntimeError, match="scratch"):
        jpeg.decode_jpeg_op(plan, blob, scratch[:64], out, status, 8, 8)
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and int(status[0]) == 0x5A5A5A5A                      # nothing was launched
    call()
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and jd.differences(out[0].cpu().numpy(), "noise_8x8_default") == 0


def _progressive(h, w):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(jd.generator().frame("smooth", h, w)[:, :, ::-1].copy()).save(buf, format="JPEG", progressive=True)
    return buf.getvalue()


def test_decode_jpeg_device_end_to_end():
    names = ["noise_48x64_default", "smooth_48x64_sub0", "noise_48x64_optimize", "smooth_48x64_rstrows"]
    files = [jd.case(n)[0] for n in names]
    out = jpeg.decode_jpeg_device(files, device=DEV)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (4, 48, 64, 3) and out.is_cuda
    got = out.cpu().numpy()
    assert all(jd.differences(got[i], n) == 0 for i, n in enumerate(names))
    # a progressive file and a broken scan inside a good batch: decoded on the host, the neighbours on the device
    prog = _progressive(48, 64)
    _, bad, _ = jd.malformed()["zrl_overrun"]
    mixed = [files[0], prog, files[1]]
    got = jpeg.decode_jpeg_device(mixed, device=DEV).cpu().numpy()
    assert jd.differences(got[0], names[0]) == 0 and jd.differences(got[2], names[1]) == 0
    assert np.array_equal(got[1], jpeg._decode_pillow(prog))
    with pytest.raises(jpeg.JpegUnsupported, match="file 1.*progressive"):
        jpeg.decode_jpeg_device(mixed, device=DEV, fallback="raise")
    with pytest.raises(jpeg.JpegCorrupt, match="file 1") as exc:
        jpeg.decode_jpeg_device([files[0], bad, files[1]], device=DEV, fallback="raise")
    assert exc.value.status == 1
    # the default fallback for a bad scan: Pillow reads this file, the device gives it status 1, and the slot holds Pillow's pixels
    got = jpeg.decode_jpeg_device([files[0], bad, files[1]], device=DEV).cpu().numpy()
    assert np.array_equal(got[1], jpeg._decode_pillow(bad))
    assert jd.differences(got[0], names[0]) == 0 and jd.differences(got[2], names[1]) == 0
    one, many, other = jd.malformed()["too_many_blocks"]          # status 3, 8 x 8
    got = jpeg.decode_jpeg_device([one, many, other], device=DEV).cpu().numpy()
    assert np.array_equal(got[1], jpeg._decode_pillow(many))
    assert np.array_equal(got[0], jd.pixels_of(one)) and np.array_equal(got[2], jd.pixels_of(other))
    cut = jd.malformed()["cut_in_half"][1]                      # neither the device nor Pillow reads a scan cut in half
    with pytest.raises(OSError):
        jpeg._decode_pillow(cut)
    with pytest.raises(jpeg.JpegCorrupt, match="file 1.*Pillow cannot read") as exc:
        jpeg.decode_jpeg_device([files[0], cut, files[1]], device=DEV)
    assert exc.value.status == jpeg.scan_status(cut)
    with pytest.raises(jpeg.JpegUnreadable, match="cannot read file 2") as exc:
        jpeg.decode_jpeg_device([files[0], files[1], b"not a jpeg at all"], device=DEV)
    assert exc.value.index == 2
    with pytest.raises(ValueError, match="one size"):
        jpeg.decode_jpeg_device([files[0], jd.case("noise_33x18_default")[0]], device=DEV)
    with pytest.raises(ValueError, match="fallback"):
        jpeg.decode_jpeg_device(files, device=DEV, fallback="cpu")
    into = torch.zeros((2, 48, 64, 3), dtype=torch.uint8, device=DEV)
    assert jpeg.decode_jpeg_device(files[:2], out=into) is into and jd.differences(into[1].cpu().numpy(), names[1]) == 0
    assert tuple(jpeg.decode_jpeg_device([], device=DEV).shape) == (0, 0, 0, 3)


def _jpeg_dataset(root, n=8, h=64, w=48):
    """an infer_data directory whose frames are .jpg files written with Pillow's defaults"""
    from frame_data import make_frames
    _, lms, _ = make_frames(n, 540, 720, seed=31)
    gen = jd.generator()
    for d in ("frames", "positions", "masks"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for i in range(n):
        frame = gen.frame("smooth", h, w).copy()
        frame[8 + i:24 + i, 4:40] = gen.frame("noise", h, w)[8 + i:24 + i, 4:40]
        with open(os.path.join(root, "frames", f"{i:06d}.jpg"), "wb") as f:
            f.write(gen.pillow_write(frame))
        np.savetxt(os.path.join(root, "positions", f"{i:06d}.txt"), lms[i] * [w / 720.0, h / 540.0])


def test_resident_clip_decoded_on_the_device_holds_the_host_decoders_bytes(tmp_path, recipe_sd):
    from calipsync_amd.frame_synth import FrameSynthesizer
    from calipsync_amd.resident_clip import ResidentClip
    from calipsync_amd.unet import Model
    _jpeg_dataset(str(tmp_path))
    host = ResidentClip.from_data_dir(str(tmp_path), DEV, decode="host")
    dev = ResidentClip.from_data_dir(str(tmp_path), DEV, decode="device")
    assert tuple(dev.frames.shape) == tuple(host.frames.shape) == (8, 64, 48, 3)
    assert int((dev.frames != host.frames).sum()) == 0
    with pytest.raises(ValueError, match="decode"):
        ResidentClip.from_data_dir(str(tmp_path), DEV, decode="gpu")
    os.makedirs(tmp_path / "broken")
    import shutil
    for d in ("frames", "positions", "masks"):
        shutil.copytree(tmp_path / d, tmp_path / "broken" / d)
    (tmp_path / "broken" / "frames" / "000005.jpg").write_bytes(b"not a jpeg at all")
    for how in ("host", "device"):
        with pytest.raises(ValueError, match="cannot read .*000005.jpg"):
            ResidentClip.from_data_dir(str(tmp_path / "broken"), DEV, decode=how)
    net = Model(6, "hubert").to(DEV)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe_sd.items()})
    net.eval()
    feats = np.random.default_rng(5).standard_normal((9, 2, 1024)).astype(np.float32)
    make = lambda how: FrameSynthesizer(None, str(tmp_path), device=DEV, batch_size=4, seed=9, net=net, resident=True, clip_decode=how)
    want = list(make("host").iterate_synthesized_frames(feats, 0, True))
    got = list(make("device").iterate_synthesized_frames(feats, 0, True))
    assert [o["physical_index"] for o in got] == [o["physical_index"] for o in want] and len(got) == 9
    for g, w in zip(got, want):
        assert np.array_equal(g["frame"], w["frame"])
    with pytest.raises(ValueError, match="clip_decode"):
        FrameSynthesizer(None, str(tmp_path), device=DEV, net=net, resident=False, clip_decode="device")
