"""calipsync_amd/facedet.py without a GPU: the state-dict manifest, the packed layout and the L2Norm fold, and the
post-processing -- Detect.forward + nms, S3FD.detect_faces, S3FDFaceDetector.detect -- bit for bit against what the reference
itself returned on the fixture (tests/golden/s3fd_b2.npz), and against tests/s3fd_ref.py's torch restatement on seeded synthetic
dense inputs."""
import os

import numpy as np
import pytest
import torch

import s3fd_ref
from calipsync_amd import _lib, facedet, recipe
from conftest import GOLDEN

H, W, P = 77, 93, 596


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "s3fd_b2.npz"))


@pytest.fixture(scope="module")
def sd():
    return recipe.make_s3fd_state_dict()


def test_manifest_is_the_references(sd):
    with open(os.path.join(GOLDEN, "state_dict_manifest_s3fd.txt")) as f:
        want = [line.split(" ", 1) for line in f.read().splitlines()]
    got = facedet.manifest()
    assert len(got) == len(want) == 65
    for (key, shape), (wkey, rest) in zip(got, want):
        assert key == wkey and rest == f"{shape} float32".replace(",)", ",)"), (key, rest)
    assert sum(int(np.prod(s)) for _, s in got) == facedet.N_PARAMETERS == 22459110
    assert [k for k, _ in got] == list(sd) and all(v.dtype == np.float32 for v in sd.values())
    facedet.check_state_dict(sd)


def test_check_state_dict_names_what_is_wrong(sd):
    bad = dict(sd)
    del bad["extras.2.bias"]
    with pytest.raises(ValueError, match="lacks extras.2.bias"):
        facedet.check_state_dict(bad)
    bad = dict(sd, **{"conf.0.weight": sd["conf.1.weight"]})
    with pytest.raises(ValueError, match="conf.0.weight has shape"):
        facedet.check_state_dict(bad)
    with pytest.raises(ValueError, match="unexpected key vgg.99.weight"):
        facedet.check_state_dict(dict(sd, **{"vgg.99.weight": sd["vgg.0.weight"]}))


def test_pack_round_trips_through_the_engines_layout(sd):
    items, total = _lib.s3fd_layout()
    assert all(off % 64 == 0 for _, off, _ in items) and total % 64 == 0
    buf = facedet.pack(sd)
    assert buf.dtype == np.float32 and buf.size == total
    named, back = facedet.packed_tensors(sd), facedet.unpack(buf)
    assert set(named) == set(back) == {n for n, _, _ in items}
    for name, a in named.items():
        assert np.array_equal(back[name], a.reshape(-1)), name
    # the layouts the header states
    assert np.array_equal(named["conv1_1.w"].reshape(3, 3, 3, 64), sd["vgg.0.weight"].transpose(2, 3, 1, 0))
    assert np.array_equal(named["conv4_2.w"].reshape(512, 3, 3, 512), sd["vgg.19.weight"].transpose(0, 2, 3, 1))
    assert np.array_equal(named["fc6.w"].reshape(1024, 3, 3, 512), sd["vgg.31.weight"].transpose(0, 2, 3, 1))
    assert np.array_equal(named["fc7.w"], sd["vgg.33.weight"][:, :, 0, 0]) and np.array_equal(named["conv7_1.w"], sd["extras.2.weight"][:, :, 0, 0])
    assert np.array_equal(named["head4.w"].reshape(8, 3, 3, 512)[:4], sd["loc.4.weight"].transpose(0, 2, 3, 1))
    assert np.array_equal(named["head4.w"].reshape(8, 3, 3, 512)[4:6], sd["conf.4.weight"].transpose(0, 2, 3, 1))
    assert not named["head4.w"].reshape(8, -1)[6:].any() and not named["head4.b"][6:].any()
    assert np.array_equal(named["head0.b"], np.concatenate([sd["loc.0.bias"], sd["conf.0.bias"]]))


def test_l2norm_fold_is_exact_in_float64_and_rounded_once(sd):
    named = facedet.packed_tensors(sd)
    for k, (name, c) in enumerate(facedet.L2NORMS):
        g = sd[f"{name}.weight"].astype(np.float64)
        w = np.concatenate([sd[f"loc.{k}.weight"], sd[f"conf.{k}.weight"]]).astype(np.float64) * g.reshape(1, c, 1, 1)
        rows = w.shape[0]
        got = named[f"head{k}.w"].reshape(8, 3, 3, c)[:rows].transpose(0, 3, 1, 2)
        assert np.array_equal(got, w.astype(np.float32)), name            # the float64 product, rounded once
    # ... and the folded conv equals the unfolded form in float64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 256, 4, 5, generator=g, dtype=torch.float64)
    xn = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    gamma, w, b = (torch.from_numpy(sd[k].astype(np.float64)) for k in ("L2Norm3_3.weight", "loc.0.weight", "loc.0.bias"))
    unfolded = torch.nn.functional.conv2d(gamma.view(1, -1, 1, 1) * xn, w, b, padding=1)
    folded = torch.nn.functional.conv2d(xn, w * gamma.view(1, -1, 1, 1), b, padding=1)
    assert float((unfolded - folded).abs().max()) <= 1e-13 * float(unfolded.abs().max())


def test_map_sizes_and_workspace_agree_with_the_library():
    import ctypes as C
    lib = _lib.load()
    assert facedet.map_sizes(H, W) == [(19, 23), (10, 12), (5, 6), (2, 3), (1, 2), (1, 1)] and facedet.n_priors(H, W) == P
    assert facedet.n_priors(270, 480) == 10750               # (what the reference itself builds: PriorBox on a 270 x 480 input)
    for h, w in ((H, W), (64, 64), (16, 16), (15, 64), (270, 480), (31, 33), (1, 1), (8, 8), (0, 5)):
        assert lib.casync_s3fd_priors(h, w) == facedet.n_priors(h, w), (h, w)
        maps = facedet.map_sizes(h, w) if h > 0 else None
        assert (lib.casync_s3fd_workspace_bytes(1, h, w) > 0) == (maps is not None)
        for k in range(6 if maps else 0):
            mh, mw = C.c_int(), C.c_int()
            assert lib.casync_s3fd_map_size(h, w, k, C.byref(mh), C.byref(mw)) == 0 and (mh.value, mw.value) == maps[k]
    assert lib.casync_s3fd_workspace_bytes(0, H, W) == 0 and lib.casync_s3fd_workspace_bytes(1, 9000, 64) == 0


# ---- the restatement in segments ---------------------------------------------------------------------------------------------
def _network_in_one_pass(sd, x, dtype):
    """S3FDNet.forward written out in one piece (nets.py:109-171), as tests/s3fd_ref.py had it before it was cut into segments:
    what segment() and heads() must compose to"""
    F = torch.nn.functional
    p = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items()}
    x = torch.as_tensor(x).to(dtype)
    taps, sources = {}, []
    for idx, name, _cin, _cout, k in facedet.VGG:
        kw = dict(padding=6, dilation=6) if name == "fc6" else dict(padding=k // 2)
        x = F.relu(F.conv2d(x, p[f"vgg.{idx}.weight"], p[f"vgg.{idx}.bias"], **kw))
        if idx in s3fd_ref.STAGE_AFTER:
            taps[s3fd_ref.STAGE_AFTER[idx]] = x
        if idx in (14, 21, 28):
            norm = x.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10
            sources.append(p[f"{facedet.L2NORMS[len(sources)][0]}.weight"].view(1, -1, 1, 1) * torch.div(x, norm))
        if idx in s3fd_ref.POOLS:
            x = F.max_pool2d(x, 2, 2, ceil_mode=s3fd_ref.POOLS[idx])
    sources.append(x)
    for idx, name, _cin, _cout, k in facedet.EXTRAS:
        x = F.relu(F.conv2d(x, p[f"extras.{idx}.weight"], p[f"extras.{idx}.bias"], stride=2 if k == 3 else 1, padding=k // 2))
        if k == 3:
            taps[name] = x
            sources.append(x)
    loc, conf = [], []
    for k, s in enumerate(sources):
        lo = F.conv2d(s, p[f"loc.{k}.weight"], p[f"loc.{k}.bias"], padding=1)
        co = F.conv2d(s, p[f"conf.{k}.weight"], p[f"conf.{k}.bias"], padding=1)
        if k == 0:
            co = torch.cat((co[:, 0:3].max(dim=1, keepdim=True)[0], co[:, 3:]), dim=1)
        loc.append(lo.permute(0, 2, 3, 1).reshape(lo.shape[0], -1))
        conf.append(co.permute(0, 2, 3, 1).reshape(co.shape[0], -1))
    taps["loc"] = torch.cat(loc, 1).view(x.shape[0], -1, 4)
    taps["conf"] = torch.cat(conf, 1).view(x.shape[0], -1, 2)
    taps["maps"] = [tuple(s.shape[2:]) for s in sources]
    return taps


@pytest.mark.parametrize("h,w", [(H, W), (141, 86)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_segments_and_the_heads_compose_to_the_network_bit_for_bit(sd, fx, h, w, dtype):
    u8 = recipe.make_s3fd_inputs(2, h, w) if (h, w) == (H, W) else recipe.make_s3fd_inputs(1, h, w, seed=recipe.S3FD_INPUT_SEED + 1)
    x = torch.from_numpy((u8.astype(np.float32) - facedet.IMG_MEAN).transpose(0, 3, 1, 2).copy())
    want = _network_in_one_pass(sd, x, dtype)
    assert want["maps"] == facedet.map_sizes(h, w)
    chained, start, t = {}, None, x
    for k in range(9):
        name, t = s3fd_ref.segment(sd, t, start, dtype)
        assert name == facedet.STAGES[k] and t.dtype == dtype
        chained[name], start = t, name
    for k, name in enumerate(facedet.STAGES[:9]):
        assert torch.equal(chained[name], want[name]), name
        if k:                                                # ... and each segment alone, started by index from the tap in front
            again, u = s3fd_ref.segment(sd, want[facedet.STAGES[k - 1]], k - 1, dtype)
            assert again == name and torch.equal(u, want[name]), name
    loc, conf, maps = s3fd_ref.heads(sd, [chained[n] for n in s3fd_ref.SOURCES], dtype)
    assert maps == want["maps"] and torch.equal(loc, want["loc"]) and torch.equal(conf, want["conf"])
    whole = s3fd_ref.network(sd, x, dtype)
    assert set(whole) == set(want) and whole["maps"] == want["maps"]
    assert all(torch.equal(whole[n], want[n]) for n in want if n != "maps")
    with pytest.raises(ValueError, match="no tap behind"):
        s3fd_ref.segment(sd, t, "conv7_2", dtype)
    if (h, w) == (H, W) and dtype == torch.float64:          # the pieces are the reference: its own float64 forward of these frames
        assert np.abs(loc.numpy() - fx["loc64"]).max() <= 1e-11 and np.abs(conf.numpy() - fx["conf64"]).max() <= 1e-11
        assert np.abs(s3fd_ref.dense(whole, h, w).numpy() - fx["det64"]).max() <= 1e-12


# ---- post-processing on the fixture: bit for bit ----------------------------------------------------------------------------
class _Dense:
    """stands in for the engine: forward_u8 returns prepared dense outputs in turn"""

    def __init__(self, outs):
        self.outs = list(outs)

    def forward_u8(self, frames):
        return self.outs.pop(0)[:len(frames)]

    def close(self):
        pass


def _singles(fx):
    """the dense tensors of the single-frame forwards the reference's detect made, as one batch"""
    return np.stack([fx["det32.0"], fx["det32.1"]])


def _detector(outs, conf=0.1):
    det = facedet.S3FDDetector.__new__(facedet.S3FDDetector)
    det.conf_threshold, det.scale, det.last_detection, det.det_net = conf, 1, None, _Dense(outs)
    return det


def test_detect_output_equals_the_references_detect_forward(fx):
    got = facedet.detect_output(fx["det32"])
    assert got.dtype == np.float32 and got.shape == (2, 2, 750, 5)
    assert np.array_equal(got, fx["detect32"])
    assert all(int((got[i, 1, :, 0] > 0).sum()) >= 3 for i in range(2))
    for i in range(2):                                       # ... and of each frame forwarded alone (other float32 bits)
        assert np.array_equal(facedet.detect_output(fx[f"det32.{i}"][None])[0], fx[f"detect32.{i}"])


@pytest.mark.parametrize("tag,th", [("01", 0.1), ("08", 0.8)])
def test_detect_faces_rows_equal_the_references(fx, tag, th):
    for i in range(2):
        rows = facedet.detect_faces_rows(fx[f"detect32.{i}"], W, H, th)
        want = fx[f"faces{tag}.{i}"]
        assert rows.dtype == np.float64 and rows.shape == want.shape and len(rows) >= 1
        assert np.array_equal(rows, want), (tag, i)


def test_detect_equals_the_references_detect(fx):
    frames = [np.zeros((H, W, 3), np.uint8)] * 2
    got = _detector([_singles(fx)]).detect(frames)
    for i, (boxes, idx) in enumerate(got):
        assert boxes.dtype == np.float64 and np.array_equal(boxes, fx[f"detect.{i}.boxes"])
        assert idx == list(fx[f"detect.{i}.indices"])
    called = _detector([_singles(fx)])(frames)
    assert [[tuple(r) for r in fx[f"detect.{i}.boxes"]] for i in range(2)] == called


def test_the_empty_case_and_the_last_detection_fallback(fx):
    frame = np.zeros((H, W, 3), np.uint8)
    empty = np.zeros((1, P, 5), np.float32)
    det = _detector([empty, _singles(fx)[:1], empty])
    boxes, idx = det.detect([frame])[0]                     # detect_face.py:50-52: no face and no history
    assert isinstance(boxes, np.ndarray) and boxes.shape == (0,) and idx == []
    assert det([frame]) == [[tuple(r) for r in fx["detect.0.boxes"]]]
    again = det.detect([frame])[0]                          # detect_face.py:53-55: the last detection stands in
    assert again is det.last_detection and np.array_equal(again[0], fx["detect.0.boxes"])


# ---- post-processing on synthetic dense inputs, against the torch restatement -------------------------------------------------
def _synthetic(seed):
    """dense det [1,P,5] of one of four kinds: clustered boxes, nothing above the threshold, more than 750 survivors, one
    candidate"""
    rng = np.random.RandomState(seed)
    kind = ("clustered", "empty", "many", "single")[seed % 4] if seed % 25 else "many"
    if kind == "many" and seed % 25:
        kind = "clustered"                                   # (the 900-survivor walk is the slow one: 8 of the 200)
    p = 900 if kind == "many" else int(rng.randint(40, 400))
    det = np.zeros((1, p, 5), np.float32)
    if kind == "many":                                       # a 30 x 30 grid of disjoint boxes
        gy, gx = np.divmod(np.arange(p), 30)
        x1, y1 = gx / 30.0 + rng.uniform(0, 0.005, p), gy / 30.0 + rng.uniform(0, 0.005, p)
        det[0, :, 1:] = np.stack([x1, y1, x1 + 0.02, y1 + 0.02], 1)
        det[0, :, 0] = rng.uniform(0.06, 1.0, p)
    else:
        centres = rng.uniform(0.1, 0.9, (int(rng.randint(1, 6)), 2))
        c = centres[rng.randint(0, len(centres), p)] + rng.normal(0, 0.03, (p, 2))
        wh = rng.uniform(0.03, 0.3, (p, 2))
        det[0, :, 1:] = np.concatenate([c - wh / 2, c + wh / 2], 1)
        det[0, :, 0] = rng.beta(0.5, 2.0, p)
        if kind == "empty":
            det[0, :, 0] *= 0.05
        if kind == "single":
            det[0, :, 0] *= 0.05
            det[0, int(rng.randint(p)), 0] = rng.uniform(0.2, 1.0)
    return kind, det


def test_post_processing_equals_the_torch_restatement_on_200_synthetic_inputs():
    kinds = {}
    for seed in range(200):
        kind, det = _synthetic(seed)
        mine = facedet.detect_output(det)
        theirs = s3fd_ref.detect_torch(torch.from_numpy(det))
        assert np.array_equal(mine, theirs.numpy()), (seed, kind)
        n = int((mine[0, 1, :, 0] > 0).sum())
        th = 0.5 if kind == "many" else (0.1, 0.5, 0.8)[seed % 3]   # (750 rows above it: see the next test)
        rows = facedet.detect_faces_rows(mine[0], 480, 270, th)
        want = s3fd_ref.detect_faces_torch(theirs[0], 480, 270, th)
        assert rows.shape == want.shape and np.array_equal(rows, want), (seed, kind)
        kinds.setdefault(kind, []).append((n, len(rows)))
    assert set(kinds) == {"clustered", "empty", "many", "single"}
    assert all(n == 0 and m == 0 for n, m in kinds["empty"]) and all(n == 1 for n, _ in kinds["single"])
    assert all(n == 750 for n, _ in kinds["many"]) and any(n > 5 for n, _ in kinds["clustered"])


def test_750_rows_above_the_threshold_run_off_the_end_as_in_the_reference():
    _, det = _synthetic(0)
    with pytest.raises(IndexError):
        facedet.detect_faces_rows(facedet.detect_output(det)[0], 480, 270, 0.01)


def test_scale_one_bypasses_the_resize(monkeypatch, fx):
    def boom(*a, **k):
        raise AssertionError("resize_scale called at scale 1")
    monkeypatch.setattr(facedet, "resize_scale", boom)
    det = _detector([fx["det32"]])
    assert len(det.dense([np.zeros((H, W, 3), np.uint8)] * 2)) == 2
