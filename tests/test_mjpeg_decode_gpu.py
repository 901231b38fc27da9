"""-m gpu: the wider device JPEG decoder (csrc/jpeg_dec_mjpeg.hip) through casync_op_mjpegdec_decode between fences, and the
public entry decode_jpeg_device(subset="mjpeg").  Every recorded 4:2:2, grayscale and table-less file at the subsequence lengths
that force late synchronisation (32 bits) and that make one subsequence per restart segment; the four samplings in one batch; the
baseline decoder's own cases through the new entry, byte for byte what the old entry gives; malformed scans; the argument checks.
Every comparison is byte equality.  The files of one size travel as one batch, so a case costs one call."""
import numpy as np
import pytest
import torch

import jpeg_decode_cases as jd
import mjpeg_decode_cases as mj
from calipsync_amd import jpeg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNK_IDS = ["chunk32", "one_subsequence"]


@pytest.mark.parametrize("chunk_bits", mj.CHUNKS, ids=CHUNK_IDS)
@pytest.mark.parametrize("size", sorted(mj.by_size()), ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_fixture_case(size, chunk_bits):
    group = mj.by_size()[size]
    res = mj.run_op([mj.case(n)[0] for n in group], chunk_bits)
    assert res.fences_ok and res.data_ok
    diffs = {n: mj.differences(res.out[i], n) for i, n in enumerate(group)}
    print(f"{len(group)} files of {size} at chunk_bits {chunk_bits}: status {sorted(set(res.status.tolist()))}, "
          f"{sum(diffs.values()):.0f} bytes differ")
    assert list(res.status) == [0] * len(group)
    assert not {n: d for n, d in diffs.items() if d}


@pytest.mark.parametrize("chunk_bits", mj.CHUNKS, ids=CHUNK_IDS)
def test_one_batch_of_the_four_samplings(chunk_bits):
    batch = mj.mixed_batch()
    plan = jpeg.plan_decode([f for f, _, _ in batch], chunk_bits, subset="mjpeg")
    assert list(plan.rec[:, 2]) == [0, 1, 2, 3]
    res = mj.run_op([f for f, _, _ in batch], chunk_bits)
    assert res.fences_ok and res.data_ok and list(res.status) == [0, 0, 0, 0]
    assert [diff(res.out[i], n) for i, (_, n, diff) in enumerate(batch)] == [0, 0, 0, 0]


@pytest.mark.parametrize("size", sorted({jd.size_of(n) for n in jd.names()}), ids=lambda s: f"{s[0]}x{s[1]}")
def test_baseline_cases_give_the_old_entrys_bytes(size):
    group = [n for n in jd.names() if jd.size_of(n) == size]
    files = [jd.case(n)[0] for n in group]
    new, old = mj.run_op(files), mj.run_op(files, entry="baseline")
    for res in (new, old):
        assert res.fences_ok and res.data_ok and list(res.status) == [0] * len(group)
    assert int((new.out != old.out).sum()) == 0
    assert all(jd.differences(new.out[i], n) == 0 for i, n in enumerate(group))


@pytest.mark.parametrize("name", mj.MALFORMED)
def test_a_malformed_scan_gives_the_twins_status_and_leaves_its_neighbours(name):
    a, bad, b = mj.malformed()[name]
    want = jpeg.scan_status(bad, subset="mjpeg")
    assert want != 0
    res = mj.run_op([a, bad, b])
    print(f"{name}: status {list(res.status)}, the host twin says {want}")
    assert res.fences_ok and res.data_ok and list(res.status) == [0, want, 0]
    assert np.array_equal(res.out[0], mj.pixels_of(a)) and np.array_equal(res.out[2], mj.pixels_of(b))


def test_the_operator_checks_its_arguments_before_it_launches():
    name = "c422noise_8x16_default"
    data = mj.case(name)[0]
    plan = jpeg.plan_decode([data], subset="mjpeg")
    blob = torch.from_numpy(plan.blob.copy()).to(DEV)
    out = torch.full((1, 8, 16, 3), 0x5A, dtype=torch.uint8, device=DEV)
    status = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    scratch = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)

    def call(kw=None):
        p = jpeg.plan_decode([data], subset="mjpeg")
        for k, v in (kw or {}).items():
            if k == "chunk_bits":
                p.chunk_bits = v
            else:
                p.rec[0, k] = v
        jpeg.decode_jpeg_op(p, blob, scratch, out, status, 8, 16)

    # the table of tests/test_jpeg_decode_gpu.py; a sampling word of 0 (4:4:4: two MCUs, so another segment count than the
    # record's), of 4 and of -1 in the place of its {2: 1}, which this entry admits
    for bad in ({0: blob.numel()}, {1: blob.numel() + 1}, {4: 2}, {5: blob.numel() - 4}, {6: blob.numel() - 8}, {7: 1000}, {8: 1}, {2: 4}, {2: -1},
                {9: 4}, {"chunk_bits": 48}):
        with pytest.raises(RuntimeError, match="mjpegdec_decode"):
            call(bad)
    with pytest.raises(RuntimeError, match="sampling 4"):
        call({2: 4})
    with pytest.raises(RuntimeError, match="scratch"):
        jpeg.decode_jpeg_op(plan, blob, scratch[:64], out, status, 8, 16)
    from calipsync_amd import _lib
    lib = _lib.load()
    assert lib.casync_op_mjpegdec_workspace_bytes(1, 0, 16, 1) < 0 and lib.casync_op_mjpegdec_workspace_bytes(1, 8, 16, -1) < 0
    # sized for the largest sampling: 4:4:4 has the most blocks (3 per 8 x 8), 4:2:0 the largest MCU padding
    assert lib.casync_op_mjpegdec_workspace_bytes(2, 8, 16, 0) == 2 * (6 * 128 + 512)
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and int(status[0]) == 0x5A5A5A5A                      # nothing was launched
    call()
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and mj.differences(out[0].cpu().numpy(), name) == 0


def _progressive(h, w):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(jd.generator().frame("smooth", h, w)[:, :, ::-1].copy()).save(buf, format="JPEG", progressive=True)
    return buf.getvalue()


def test_decode_jpeg_device_end_to_end():
    batch = mj.mixed_batch()
    files = [f for f, _, _ in batch] + [mj.case("nodht422_48x64_all")[0]]
    out = jpeg.decode_jpeg_device(files, device=DEV, subset="mjpeg", fallback="raise")      # nothing takes the host path
    assert out.dtype == torch.uint8 and tuple(out.shape) == (5, 48, 64, 3) and out.is_cuda
    got = out.cpu().numpy()
    assert [diff(got[i], n) for i, (_, n, diff) in enumerate(batch)] == [0, 0, 0, 0] and mj.differences(got[4], "nodht422_48x64_all") == 0
    # the default subset sends the same files to the host and gives the same pixels
    assert np.array_equal(jpeg.decode_jpeg_device(files, device=DEV).cpu().numpy(), got)
    with pytest.raises(jpeg.JpegUnsupported, match="file 1.*chroma sampling"):
        jpeg.decode_jpeg_device(files, device=DEV, fallback="raise")
    # a progressive file in the middle of a batch takes the host path; fallback="raise" names it
    prog = _progressive(48, 64)
    mixed = [files[1], prog, files[3]]
    got = jpeg.decode_jpeg_device(mixed, device=DEV, subset="mjpeg").cpu().numpy()
    assert mj.differences(got[0], batch[1][1]) == 0 and mj.differences(got[2], batch[3][1]) == 0
    assert np.array_equal(got[1], jpeg._decode_pillow(prog))
    with pytest.raises(jpeg.JpegUnsupported, match="file 1.*progressive"):
        jpeg.decode_jpeg_device(mixed, device=DEV, subset="mjpeg", fallback="raise")
    # a non-zero device status: status 1 and 3 fall back to Pillow where it reads the file, "raise" carries the code
    a, bad, b = mj.malformed()["422_zrl_overrun"]
    with pytest.raises(jpeg.JpegCorrupt, match="file 1") as exc:
        jpeg.decode_jpeg_device([a, bad, b], device=DEV, subset="mjpeg", fallback="raise")
    assert exc.value.status == 1
    got = jpeg.decode_jpeg_device([a, bad, b], device=DEV, subset="mjpeg").cpu().numpy()
    assert np.array_equal(got[1], jpeg._decode_pillow(bad)) and np.array_equal(got[0], mj.pixels_of(a)) and np.array_equal(got[2], mj.pixels_of(b))
    a, many, b = mj.malformed()["gray_too_many_blocks"]
    with pytest.raises(jpeg.JpegCorrupt) as exc:
        jpeg.decode_jpeg_device([a, many, b], device=DEV, subset="mjpeg", fallback="raise")
    assert exc.value.status == 3
    a, cut, b = mj.malformed()["422_cut_in_half"]                # neither the device nor Pillow reads a scan cut in half
    with pytest.raises(jpeg.JpegCorrupt, match="file 1.*Pillow cannot read") as exc:
        jpeg.decode_jpeg_device([a, cut, b], device=DEV, subset="mjpeg")
    assert exc.value.status == jpeg.scan_status(cut, subset="mjpeg")
    with pytest.raises(ValueError, match="one size"):
        jpeg.decode_jpeg_device([files[1], mj.case("c422noise_9x17_default")[0]], device=DEV, subset="mjpeg")
    into = torch.zeros((2, 48, 64, 3), dtype=torch.uint8, device=DEV)
    assert jpeg.decode_jpeg_device(files[1:3], out=into, subset="mjpeg") is into and mj.differences(into[0].cpu().numpy(), batch[1][1]) == 0
    assert tuple(jpeg.decode_jpeg_device([], device=DEV, subset="mjpeg").shape) == (0, 0, 0, 3)
