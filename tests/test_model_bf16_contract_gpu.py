"""-m gpu: the bf16 U-Net engine held to an equal-contract model, PLAN BY PLAN and SEGMENT BY SEGMENT, and to the reference's own
bf16 autocast error end to end.

Segments (tests/unet_bf16_model.py): the forward is cut at the taps casync_tap serves.  For every plan below one forward runs,
every tap is read (and must be a widened bf16 tensor), and every segment is recomputed on the CPU FROM THE ENGINE'S OWN START
TAPS in two forms -- the float64 oracle on the raw state dict, and the equal-contract model (folded weights, bf16 GEMM
operands, fp32 sums, one rounding wherever the engine stores bf16).  The engine's tap `got` must meet

    max|got - ref64| <= MAX_BAR x max|model - ref64|        mean|got - ref64| <= MEAN_BAR x mean|model - ref64|

with the two factors of tests/test_facedet_bf16_gpu.py (2.0, 1.25), and mean|model - ref64| > 0 so that no ratio is vacuous.
No error accumulates over a segment's start, so a dropped halo row, an addend missing on one border, a permuted channel or a
tile rounded twice moves a ratio by far more than the factor; the plain engine-against-model difference is printed, not
barred (two summation orders of one contract differ).  Only the first and last frame of each lane go through the oracle.

Plans, at the smallest batch that selects each; every case asserts from the launch log, by the names of
tools/kernel_resources.table(), that the kernels which define it ran:

    b3          GEMM + dw3x3 launches, materialised upsample, K split by stream-K / the small-M tile (single lane)
    b3_nosk     the same with gemm_streamk = 0
    b12         single lane: pw_dw_bf16_kernel / _strip_kernel, commuted upsample of up1.0 / up2.0, ir_fused_bf16_kernel with ir_dw_mfma
    b32         two lanes of 16 frames (kMinLaneBatch)
    ring        bf16_plan = 48: three lanes, gemm_ring128 (pw_gemm_glds_kernel<__bf16, 128, 128, 2, 2, 2, false>), audio on the
                lane's stream.  The ring instance takes launches of more than 256 tiles only: the batch goes up from 48 in
                steps of 3 x 16 until the launch log shows it (RING_BATCH records where it did: B = 144, three lanes of 48,
                on an MI355X; at 48 and 96 frames no 128 x 128 launch of a lane passes 256 tiles).
    option legs at B = 12, each re-checking the segments the option touches: att_bf16 = 0, att_nz = 2, ir_dw_mfma = 0,
    fuse_dw_bf16 = 1, fuse_dw_bf16 = 0, ups_commute_bf16 = 0.

(cross_attention_bf16_kernel is the attention core of EVERY batch of the default options, B = 3 included: launch_cross_attention
asks att_bf16 and att_nz only.)

WeNet: the audio segments of WenetModel(6, precision="bf16") at B = 2 (GEMM + depthwise launches) and B = 16
(pw_dw_bf16_rect_kernel<16, 32, 64>); the rest of the net is shared with the HuBERT model.

End to end: the engine's taps and output on the golden inputs against float64, within MAX_BAR / MEAN_BAR times the reference's
own |autocast - float64| of tests/golden/unet_bf16_bar.npz (made by tests/golden/make_unet_bf16_bar.py), both audio modes.

Measured on an MI355X (DESIGN section 7 has the table).  Segments, engine / model: 1.000 on max and mean (to three decimals) in
every plan and option leg, except
  kx     mean 1.069 ... 1.071, max 1.000 ... 1.422 -- the engine adds each b_1 GEMM's value to the running sum before rounding it
         for the att_i tap, the model can only start from the rounded tap (tests/unet_bf16_model.py);
  fuse   max 0.905 ... 1.112, mean 0.997 ... 1.005; u1 / u2 max 0.831 ... 1.000 (b12, fuse_dw_bf16=1); out max 1.000 ... 1.102 (fp32 sums
         in another order); mean 0.999 ... 1.002 on all of these.
The engine-against-model difference itself is 0 for x1; its mean is below 7 % of the model's own mean error elsewhere, but for kx (71 %)
and fuse (47 %: four blocks with K up to 2048, where another summation order flips roundings of E that the next block amplifies).
End to end, engine / autocast: HuBERT max 0.326 (x1) ... 0.920 (audio_conv3), mean 0.280 (x1) ... 0.881 (audio_conv2), the output
0.656 / 0.566; WeNet max 0.598 ... 1.033, mean 0.621 ... 1.182 (audio_conv1), output 0.647 / 0.621.
What this test found: WeNet's audio_conv1 first measured max 1.021 x, mean 1.364 x autocast against the 1.25 x bar, and the equal-contract
model reproduced both figures.  AudioConvWenet's conv1 is a RESIDUAL block on the network's fp32 input; under autocast the reference keeps
that sum in fp32 (x + conv(x): only conv(x) is bf16), the engine added the bf16-rounded window.  Fixed in the engine (engine.hip encode()):
the window is stored as two bf16 halves, R(x) and R(x - R(x)), the project GEMM adds both in fp32 and rounds once -- 1.033 / 1.182 now,
audio_conv2 1.069 / 1.096 -> 0.971 / 1.007.
"""
import functools
import os

import numpy as np
import pytest
import torch

import gpu_util
import unet_bf16_model as um
import wenet_ref
from calipsync_amd import recipe
from calipsync_amd.unet import Model, WenetModel
from conftest import GOLDEN
from oracle import unet_oracle
from test_facedet_bf16_gpu import MAX_BAR, MEAN_BAR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LANE = 16                                   # kMinLaneBatch (engine.hip)
RING = "pw_gemm_glds_kernel<__bf16, 128, 128, 2, 2, 2, false>"
ATT16, ATT32 = "cross_attention_bf16_kernel", "cross_attention_kernel<__bf16>"
UPS = "upsample2x_kernel<__bf16>"
STRIP, FRAME20 = "pw_dw_bf16_strip_kernel<40, 8, 1, 64>", "pw_dw_bf16_kernel<20, 1, 64, 1>"
FUSED_MFMA, FUSED_VALU = "ir_fused_bf16_kernel<32, 64, 64, 2, false, true>", "ir_fused_bf16_kernel<64, 128, 32, 1, true, false>"
RECT = "pw_dw_bf16_rect_kernel<16, 32, 64>"
FAMILIES = ("dw3x3", "pw_dw_bf16")          # any instance of these counts
SEG_NAMES = [n for n, _ in um.SEGMENTS]
NO_COMMUTE = dict(um.DEFAULT_FLAGS, commute_up=())

# plan -> batch, options, lanes, model flags, the segments to check (None = all), kernels that must / must not have run
# ("dw3x3" / "pw_dw_bf16" stand for any instance of that family)
PLANS = {
    "b3": dict(batch=3, opts={}, lanes=1, flags=NO_COMMUTE, only=None, ran=("dw3x3", UPS, ATT16, FUSED_MFMA, FUSED_VALU), not_ran=("pw_dw_bf16",)),
    "b3_nosk": dict(batch=3, opts=dict(gemm_streamk=0), lanes=1, flags=NO_COMMUTE, only=None, ran=("dw3x3", UPS, ATT16), not_ran=("pw_dw_bf16",)),
    "b12": dict(batch=12, opts={}, lanes=1, flags=um.DEFAULT_FLAGS, only=None, ran=(STRIP, FRAME20, ATT16, FUSED_MFMA, FUSED_VALU),
                not_ran=("dw3x3", UPS)),
    "b32": dict(batch=32, opts={}, lanes=2, flags=um.DEFAULT_FLAGS, only=None, ran=(STRIP, FRAME20, ATT16, FUSED_MFMA), not_ran=("dw3x3", UPS)),
    "ring": dict(batch=None, opts=dict(bf16_plan=48), lanes=3, flags=um.DEFAULT_FLAGS, only=None, ran=(RING, STRIP, FRAME20, ATT16),
                 not_ran=("dw3x3", UPS)),
    "att_bf16=0": dict(batch=12, opts=dict(att_bf16=0), lanes=1, flags=dict(um.DEFAULT_FLAGS, p_bf16=False),
                       only=um.FLAG_SEGMENTS["p_bf16"], ran=(ATT32,), not_ran=(ATT16,)),
    "att_nz=2": dict(batch=12, opts=dict(att_nz=2), lanes=1, flags=dict(um.DEFAULT_FLAGS, p_bf16=False),
                     only=um.FLAG_SEGMENTS["p_bf16"], ran=(ATT32,), not_ran=(ATT16,)),
    "ir_dw_mfma=0": dict(batch=12, opts=dict(ir_dw_mfma=0), lanes=1, flags=dict(um.DEFAULT_FLAGS, dw_taps_bf16=0),
                         only=um.FLAG_SEGMENTS["dw_taps_bf16"], ran=("ir_fused_bf16_kernel<32, 64, 64, 2, false, false>", FUSED_VALU),
                         not_ran=(FUSED_MFMA,)),
    # fuse_dw_bf16 = 1: the 40 x 40 blocks (down2.1, down3.0, up2.0) leave the strip kernel, up2.0 its commuted upsample with it
    "fuse_dw_bf16=1": dict(batch=12, opts=dict(fuse_dw_bf16=1), lanes=1, flags=dict(um.DEFAULT_FLAGS, commute_up=("up1",)),
                           only=("x3", "x4", "u1", "u2"), ran=(FRAME20, "dw3x3", UPS), not_ran=(STRIP,)),
    "fuse_dw_bf16=0": dict(batch=12, opts=dict(fuse_dw_bf16=0), lanes=1, flags=NO_COMMUTE,
                           only=("x3", "x4", "x5", "audio_conv4", "a", "fuse", "u1", "u2"), ran=("dw3x3", UPS), not_ran=("pw_dw_bf16",)),
    "ups_commute_bf16=0": dict(batch=12, opts=dict(ups_commute_bf16=0), lanes=1, flags=NO_COMMUTE, only=("u1", "u2"),
                               ran=(STRIP, FRAME20, UPS), not_ran=("dw3x3",)),
}
RING_BATCHES = (48, 96, 144, 192)           # 3 x 16 frames and up
RING_BATCH = {}                             # filled by _run("ring"): the batch at which the 128 x 128 ring instance ran
CASES = [(p, s) for p, spec in PLANS.items() for s in (spec["only"] or SEG_NAMES)]


@functools.lru_cache(maxsize=None)
def _sd(mode="hubert"):
    return recipe.make_state_dict(mode=mode)


@functools.lru_cache(maxsize=None)
def _sd64(mode="hubert"):
    return um.to64(_sd(mode))


@functools.lru_cache(maxsize=None)
def _contract(mode="hubert"):
    return um.Contract(_sd(mode), mode)


_NETS = {}


def _net(mode="hubert"):
    if mode not in _NETS:
        m = (WenetModel(6, precision="bf16") if mode == "wenet" else Model(6, "hubert", precision="bf16")).to(DEV)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in _sd(mode).items()})
        _NETS[mode] = m.eval()
    return _NETS[mode]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _NETS.clear()
    for f in (_run, _wenet_run, _golden_run, _oracle64):
        f.cache_clear()
    torch.cuda.empty_cache()


def _lane_frames(batch, lanes):
    """first and last frame of each lane (run_forward's split: batch / lanes frames each, the remainder to the first lanes)"""
    pick, b0 = [], 0
    for l in range(lanes):
        n = batch // lanes + (1 if l < batch % lanes else 0)
        pick += [b0, b0 + n - 1]
        b0 += n
    return sorted(set(pick))


def _forward(net, x, a, names, pick):
    """one forward with the launch log on -> (taps of frames `pick` on the host, launched kernel names)"""
    batch = x.shape[0]
    with gpu_util.launched() as ran:
        out = net(torch.from_numpy(x).to(DEV), torch.from_numpy(a).to(DEV))
        torch.cuda.synchronize()
    taps = {n: net.tap(n, batch)[pick].cpu() for n in names if n != "out"}
    taps["out"] = out[pick].cpu()
    return taps, ran


def _check_kernels(plan, ran, must, must_not):
    table = gpu_util.kernel_table()
    if table:                                # (empty where the library was shipped without its objects)
        assert not [n for n in ran if n not in table], (plan, "launched kernels the built library's table does not name")
    def seen(k):
        return any(n.startswith(k) for n in ran) if k in FAMILIES else k in ran

    for k in must:
        assert seen(k), (plan, "did not run", k, sorted(ran))
    for k in must_not:
        assert not seen(k), (plan, "ran", k, sorted(ran))


@functools.lru_cache(maxsize=None)
def _run(plan):
    spec, net = PLANS[plan], _net()
    batches = RING_BATCHES if spec["batch"] is None else (spec["batch"],)
    with gpu_util.options(net, **spec["opts"]):
        for batch in batches:
            assert batch >= LANE * spec["lanes"] if spec["lanes"] > 1 else batch < 2 * LANE      # run_forward's lane rule
            if plan == "ring":
                assert batch >= net.get_option("bf16_plan") == 48
            else:
                assert batch < net.get_option("bf16_plan") and net.get_option("lanes") == 2
            pick = _lane_frames(batch, spec["lanes"])
            x, a = recipe.make_inputs_range(700, batch)
            taps, ran = _forward(net, x, a, SEG_NAMES, pick)
            if plan != "ring" or RING in ran:
                break
        if plan == "ring":
            RING_BATCH["batch"] = batch
            print(f"ring: {RING} ran at B = {batch}")
        if plan == "b3":          # the K split is in effect: without it the same forward has other bits
            with gpu_util.options(net, gemm_streamk=0):
                plain, _ = _forward(net, x, a, ("out",), pick)
            assert not torch.equal(plain["out"], taps["out"]), "gemm_streamk changed nothing at B = 3: no GEMM split its K"
    _check_kernels(plan, ran, spec["ran"], spec["not_ran"])
    taps["x"], taps["audio"] = torch.from_numpy(x[pick]), torch.from_numpy(a[pick])
    return taps


def _stat(got, ref):
    d = (got.double() - ref).abs()
    return (float(d.max()) if bool(torch.isfinite(d).all()) else float("inf")), float(d.mean())


def _hold(tag, name, got, src, mode, flags):
    """the assertion of this module: one segment of one plan"""
    ref = um.reference(_sd64(mode), name, *src, mode=mode)
    model = _contract(mode).segment(name, *src, **flags)
    assert got.shape == ref.shape == model.shape
    if name != "out":
        assert torch.equal(got, um.bf16(got)), (tag, name, "not a widened bf16 tensor")
    (mx, mean), (mmx, mmean) = _stat(got, ref), _stat(model, ref)
    dmx, dmean = _stat(got, model.double())
    assert mmean > 0 and mmx > 0, (tag, name, "the model has no error here: the ratio would be vacuous")
    print(f"{tag:18s} {name:12s} engine/model max {mx / mmx:.3f} mean {mean / mmean:.3f}   (engine {mx:.3e} {mean:.3e}, model {mmx:.3e} "
          f"{mmean:.3e}; engine - model max {dmx:.3e} mean {dmean:.3e})")
    assert mx <= MAX_BAR * mmx and mean <= MEAN_BAR * mmean, (tag, name, round(mx / mmx, 3), round(mean / mmean, 3))


@pytest.mark.parametrize("plan,name", CASES)
def test_segment_from_the_engines_own_taps_within_the_equal_contract_models_error(plan, name):
    taps = _run(plan)
    _hold(plan, name, taps[name], [taps[k] for k in um.SOURCES[name]], "hubert", PLANS[plan]["flags"])


def test_the_ring_plan_ran_at_its_smallest_batch():
    """RING_BATCH: where the 128 x 128 ring instance first appears (launches of more than 256 tiles)"""
    _run("ring")
    assert RING_BATCH["batch"] in RING_BATCHES
    print("ring plan batch:", RING_BATCH["batch"])


# ---- WeNet: the audio segments ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wenet_run(batch):
    net = _net("wenet")
    x, a = recipe.make_inputs(40 + batch, mode="wenet")
    x, a = x[40:], a[40:]
    pick = _lane_frames(batch, 1)
    taps, ran = _forward(net, x, a, um.AUDIO_SEGMENTS, pick)
    if batch >= 12:
        _check_kernels(f"wenet b{batch}", ran, (RECT,), ())
    else:
        _check_kernels(f"wenet b{batch}", ran, ("dw3x3",), ("pw_dw_bf16",))
    taps["audio"] = torch.from_numpy(a[pick])
    return taps


@pytest.mark.parametrize("name", um.AUDIO_SEGMENTS)
@pytest.mark.parametrize("batch", [2, 16])
def test_wenet_audio_segment_within_the_equal_contract_models_error(batch, name):
    taps = _wenet_run(batch)
    _hold(f"wenet b{batch}", name, taps[name], [taps[k] for k in um.SOURCES[name]], "wenet", um.DEFAULT_FLAGS)


# ---- end to end: the reference's own autocast error ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle64(mode):
    x, a = recipe.make_inputs(2, mode=mode)
    taps = {}
    taps["out"] = (wenet_ref if mode == "wenet" else unet_oracle).forward(_sd64(mode), torch.from_numpy(x).double(),
                                                                          torch.from_numpy(a).double(), taps)
    return taps


@functools.lru_cache(maxsize=None)
def _golden_run(mode):
    x, a = recipe.make_inputs(2, mode=mode)
    taps, _ = _forward(_net(mode), x, a, SEG_NAMES, [0, 1])
    return taps


END_TO_END = [("hubert", n) for n in SEG_NAMES if n != "audio_conv1"] + \
             [("wenet", n) for n in ("audio_conv1", "audio_conv2", "audio_conv3", "audio_conv4", "audio_conv5", "a", "x5", "tx", "kx", "fuse", "u4", "out")]


@pytest.mark.parametrize("mode,name", END_TO_END)
def test_golden_inputs_end_to_end_within_the_references_autocast_error(mode, name):
    """|engine - float64| of a tap of the B = 2 golden forward against [max, mean] of the reference's |autocast - float64| at the same
    tap (every tap the float64 restatement records: unet_oracle.forward has none behind HuBERT's conv1, wenet_ref.forward those
    of tests/test_wenet_gpu.py)."""
    bar = np.load(os.path.join(GOLDEN, "unet_bf16_bar.npz"))
    assert float(bar[f"{mode}.fp32_vs_fixture"]) <= 1e-5 and float(bar[f"{mode}.f64_vs_oracle"]) <= 1e-12
    got, ref = _golden_run(mode)[name], _oracle64(mode)[name]
    (mx, mean), (amx, amean) = _stat(got, ref), bar[f"{mode}.{name}"]
    print(f"{mode:6s} {name:12s} max {mx:.3e} = {mx / amx:.3f} x autocast, mean {mean:.3e} = {mean / amean:.3f} x autocast")
    assert mx <= MAX_BAR * amx and mean <= MEAN_BAR * amean, (mode, name, round(mx / amx, 3), round(mean / amean, 3))
