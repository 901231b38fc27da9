"""Deterministic golden recipe "G1.2" for weights and inputs.

The reference ships no checkpoint and PyTorch's default init makes parity
vacuous (``gamma = 0`` switches all four cross-attention outputs off,
reference module/unet.py:205).  This recipe gives a trained-like, numerically
well-conditioned network whose output depends measurably on the audio branch
and on the attention blocks.

The random stream is the repo's own counter-based generator (splitmix64 hash
of ``(seed, crc32(key), index)`` -> Box-Muller), *not* ``torch.randn`` or a
NumPy ``Generator`` distribution, so the very same bits are produced in the
build container (where the golden fixtures are made from the reference) and on
the GPU box (where only this repo exists).
"""
from __future__ import annotations

import zlib
from typing import Dict, Tuple

import numpy as np

from . import arch

WEIGHT_SEED = 1234
INPUT_SEED = 7
GAIN = 1.2
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x: np.ndarray) -> np.ndarray:
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
    z = x
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
    return z ^ (z >> np.uint64(31))


def _bits(seed: int, stream: int, n: int, lane: int) -> np.ndarray:
    """n 64-bit words of stream (seed, stream, lane); pure function of its args."""
    with np.errstate(over="ignore"):
        base = _splitmix64(np.array([(seed << 32) ^ (stream & 0xFFFFFFFF)], dtype=np.uint64))
        base = _splitmix64(base + np.uint64(lane))
        idx = np.arange(n, dtype=np.uint64)
        return _splitmix64(base + idx * np.uint64(0xD1342543DE82EF95))


def uniform01(seed: int, stream: int, n: int, lane: int = 0) -> np.ndarray:
    """float64 uniforms in [0, 1) with 53 random bits."""
    return (_bits(seed, stream, n, lane) >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


def normal01(seed: int, stream: int, n: int) -> np.ndarray:
    """float64 standard normals (Box-Muller on two independent lanes)."""
    u1 = uniform01(seed, stream, n, lane=1)
    u2 = uniform01(seed, stream, n, lane=2)
    r = np.sqrt(-2.0 * np.log1p(-u1))          # 1-u1 in (0, 1]
    return r * np.cos(2.0 * np.pi * u2)


def _stream(key: str) -> int:
    return zlib.crc32(key.encode("utf-8"))


def make_state_dict(seed: int = WEIGHT_SEED, mode: str = "hubert") -> Dict[str, np.ndarray]:
    """All 582 entries of the reference ``state_dict`` (wenet: 577) as NumPy arrays (G1.2).  A key present in both
    modes with the same shape gets the same values in both."""
    sd: Dict[str, np.ndarray] = {}
    for key, shape, dtype, role in arch.manifest(mode):
        n = int(np.prod(shape)) if shape else 1
        s = _stream(key)
        if role in ("conv_weight", "linear_weight"):
            fan_in = int(np.prod(shape[1:]))
            v = normal01(seed, s, n) * (GAIN / np.sqrt(fan_in))
        elif role == "conv_bias":
            v = normal01(seed, s, n) * 0.05
        elif role == "bn_weight":
            v = 0.8 + 0.4 * uniform01(seed, s, n)
        elif role == "bn_bias":
            v = normal01(seed, s, n) * 0.1
        elif role == "bn_mean":
            v = normal01(seed, s, n) * 0.1
        elif role == "bn_var":
            v = 0.8 + 0.4 * uniform01(seed, s, n)
        elif role == "gamma":
            v = np.full(n, 0.5)
        elif role == "bn_count":
            sd[key] = np.zeros(shape, dtype=np.int64)
            continue
        else:  # pragma: no cover - manifest roles are closed
            raise ValueError(role)
        sd[key] = v.astype(np.float32).reshape(shape)
    return sd


# Second fixture, "G1.2-B" (tests/golden/unet_g12b_b3.npz): other seeds, and the corners the first recipe leaves
# out -- attention gammas of both signs and very different sizes, BatchNorm channels whose running variance
# (1e-3) is small enough for eps = 1e-5 to matter in the fold, audio features four times larger, an odd batch.
WEIGHT_SEED_B = 0x5EED0B
INPUT_SEED_B = 0x1B0B
GAMMAS_B = (0.5, -0.75, 1.25, 0.1)
SMALL_VAR_B = 1e-3
AUDIO_SCALE_B = 4.0
BATCH_B = 3


def make_state_dict_b() -> Dict[str, np.ndarray]:
    """The G1.2-B weights: ``make_state_dict(WEIGHT_SEED_B)`` with GAMMAS_B on the four cross-attention blocks
    and every 7th BatchNorm channel (offset by the layer) at running_var = 1e-3; the BatchNorm weight of those
    channels is scaled by sqrt(1e-3) so that activations keep their size through the 60-odd layers."""
    sd = make_state_dict(WEIGHT_SEED_B)
    g = 0
    for key, shape, _dtype, role in arch.manifest():
        if role == "gamma":
            sd[key] = np.full(shape, GAMMAS_B[g], dtype=np.float32)
            g += 1
        elif role == "bn_var":
            sel = np.arange(shape[0]) % 7 == _stream(key) % 7
            sd[key] = np.where(sel, np.float32(SMALL_VAR_B), sd[key]).astype(np.float32)
            wkey = key[: -len("running_var")] + "weight"
            sd[wkey] = np.where(sel, sd[wkey] * np.float32(np.sqrt(SMALL_VAR_B)), sd[wkey]).astype(np.float32)
    assert g == len(GAMMAS_B)
    return sd


def make_inputs_b(batch: int = BATCH_B) -> Tuple[np.ndarray, np.ndarray]:
    x, a = make_inputs(batch, INPUT_SEED_B)
    return x, (a * np.float32(AUDIO_SCALE_B)).astype(np.float32)


def make_inputs(batch: int, seed: int = INPUT_SEED, mode: str = "hubert") -> Tuple[np.ndarray, np.ndarray]:
    """Synthetic frames: x ~ U(0,1) [B,6,160,160], audio ~ N(0,1) [B,32,32,32] (wenet: [B,256,16,32]).

    Mirrors the reference self-benchmark's shapes
    (image_infer_v1/models/unet.py:342-347).  Frame ``b`` depends only on
    ``(seed, b)``, so any shard of a larger batch reproduces the same frames."""
    x = np.empty((batch, 6, arch.FACE_HW, arch.FACE_HW), dtype=np.float32)
    a = np.empty((batch,) + arch.AUDIO_SHAPE[mode], dtype=np.float32)
    for b in range(batch):
        x[b] = uniform01(seed, 0x1000000 + b, x[b].size).astype(np.float32).reshape(x[b].shape)
        a[b] = normal01(seed, 0x2000000 + b, a[b].size).astype(np.float32).reshape(a[b].shape)
    return x, a


def make_inputs_range(start: int, count: int, seed: int = INPUT_SEED):
    """Frames [start, start+count) of the infinite synthetic stream."""
    x = np.empty((count, 6, arch.FACE_HW, arch.FACE_HW), dtype=np.float32)
    a = np.empty((count, 32, arch.AUDIO_HW, arch.AUDIO_HW), dtype=np.float32)
    for i in range(count):
        b = start + i
        x[i] = uniform01(seed, 0x1000000 + b, x[i].size).astype(np.float32).reshape(x[i].shape)
        a[i] = normal01(seed, 0x2000000 + b, a[i].size).astype(np.float32).reshape(a[i].shape)
    return x, a


# ---- PFLD_GhostOne landmark network (calipsync_amd/landmarks.py) ----------------------------------------------------
PFLD_WEIGHT_SEED = 0x9F1D
PFLD_INPUT_SEED = 0x9F1E


def make_pfld_state_dict(seed: int = PFLD_WEIGHT_SEED) -> Dict[str, np.ndarray]:
    """The 2090 entries of a train-form ``PFLD_GhostOne(0.5, 192, 110)`` state dict.  Each MobileOneBlock sums six conv
    branches (+ scale + skip), so BatchNorm gammas near 1 take the activations to 5e4 within the network; this recipe keeps
    every stage at order 1: conv weights U(+-1/sqrt(fan_in)) with fan_in = (cin/groups) k^2, plain conv biases
    U(+-1/sqrt(256)), BN running_var U(0.75, 1.25), running_mean and bias N(0, 0.1^2), BN weight 0.4 U(0.75, 1.25) with a
    negative sign with probability 1/4."""
    from . import landmarks
    sd: Dict[str, np.ndarray] = {}
    for key, shape in landmarks.manifest("train"):
        n = int(np.prod(shape)) if shape else 1
        s = _stream("pfld." + key)
        leaf = key.rsplit(".", 1)[1]
        is_bn = ".bn." in key or ".rbr_skip." in key
        if leaf == "num_batches_tracked":
            sd[key] = np.zeros(shape, dtype=np.int64)
            continue
        if is_bn and leaf == "running_var":
            v = 0.75 + 0.5 * uniform01(seed, s, n)
        elif is_bn and leaf in ("running_mean", "bias"):
            v = normal01(seed, s, n) * 0.1
        elif is_bn and leaf == "weight":
            sign = np.where(uniform01(seed, s, n, lane=3) < 0.25, -1.0, 1.0)
            v = 0.4 * (0.75 + 0.5 * uniform01(seed, s, n)) * sign
        elif leaf == "weight":
            v = (2.0 * uniform01(seed, s, n) - 1.0) / np.sqrt(int(np.prod(shape[1:])))
        else:                                   # conv_out.bias, localization.*.bias
            v = (2.0 * uniform01(seed, s, n) - 1.0) / np.sqrt(256.0)
        sd[key] = v.astype(np.float32).reshape(shape)
    return sd


def make_pfld_inputs(batch: int, seed: int = PFLD_INPUT_SEED) -> np.ndarray:
    """Synthetic face crops as cv2.resize hands them over: uint8 BGR [B,192,192,3]; crop b depends only on (seed, b)."""
    x = np.empty((batch, 192, 192, 3), dtype=np.uint8)
    for b in range(batch):
        x[b] = np.floor(uniform01(seed, 0x3000000 + b, x[b].size) * 256.0).astype(np.uint8).reshape(x[b].shape)
    return x


# ---- S3FD face detector (calipsync_amd/facedet.py) -------------------------------------------------------------------
S3FD_WEIGHT_SEED = 0x53FD
S3FD_INPUT_SEED = 0x53FE
# Per source: the factor on conf[k]'s weights and the shift of its face-logit bias.  He-initialised heads with neither
# saturate (scores of exactly 1.0, nearly every prior above 0.05), and a detection fixture would then hang on ties; with these
# constants, found once, a few percent of the priors pass 0.05 and no two scores come close (tests/golden/make_s3fd_golden.py
# asserts the margins).
S3FD_CONF_SCALE = (6.0, 3.75, 3.0, 3.5, 4.5, 4.0)
S3FD_CONF_SHIFT = (-11.9, -10.7, -13.1, -4.2, 0.2, -0.8)


def make_s3fd_state_dict(seed: int = S3FD_WEIGHT_SEED) -> Dict[str, np.ndarray]:
    """The 65 entries of an ``S3FDNet`` state dict: conv weights N(0, 2 / fan_in) (the trunk is conv + ReLU throughout, so this
    keeps the scale from stage to stage), conv1_1 a further 1 / 25 (its input is pixels minus the mean, of order 50), biases
    N(0, 0.05^2), L2Norm weights their constants 10 / 8 / 5 times U(0.75, 1.25) so the fold into the heads is visible, head
    weights N(0, 1 / fan_in) -- on the normalised sources, whose elements are of order weight / sqrt(C), times sqrt(C) /
    weight -- and the conf heads calibrated by S3FD_CONF_*."""
    from . import facedet
    sd: Dict[str, np.ndarray] = {}
    gammas = (10.0, 8.0, 5.0)
    for key, shape in facedet.manifest():
        n = int(np.prod(shape))
        s = _stream("s3fd." + key)
        module, index, leaf = key.split(".") if key.count(".") == 2 else (key.split(".")[0], "", key.split(".")[1])
        if module.startswith("L2Norm"):
            v = gammas[[m for m, _ in facedet.L2NORMS].index(module)] * (0.75 + 0.5 * uniform01(seed, s, n))
        elif leaf == "bias":
            v = normal01(seed, s, n) * 0.05
            if module == "conf":
                v[-1] += S3FD_CONF_SHIFT[int(index)]             # the face logit is the last channel of every conf head
        elif module in ("loc", "conf"):
            k, cin = int(index), shape[1]
            v = normal01(seed, s, n) / np.sqrt(9.0 * cin)
            if k < 3:
                v *= np.sqrt(cin) / gammas[k]
            if module == "conf":
                v *= S3FD_CONF_SCALE[k]
        else:
            v = normal01(seed, s, n) * np.sqrt(2.0 / int(np.prod(shape[1:])))
            if key == "vgg.0.weight":
                v /= 25.0
        sd[key] = v.astype(np.float32).reshape(shape)
    return sd


def make_s3fd_inputs(batch: int, h: int = 77, w: int = 93, seed: int = S3FD_INPUT_SEED) -> np.ndarray:
    """Synthetic frames as the detector receives them: uint8 [B,h,w,3]; frame b depends only on (seed, b, h, w).  Smooth
    blobs over noise rather than white noise, so neighbouring priors differ."""
    x = np.empty((batch, h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    for b in range(batch):
        u = uniform01(seed, 0x5000000 + b, 64)
        img = 96.0 + 64.0 * uniform01(seed, 0x6000000 + b, h * w * 3).reshape(h, w, 3)
        for i in range(6):
            cy, cx, r = u[4 * i] * h, u[4 * i + 1] * w, 4.0 + 12.0 * u[4 * i + 2]
            g = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * r * r))
            img += (160.0 * u[4 * i + 3] - 60.0) * g[:, :, None] * (0.5 + u[32 + 3 * i:35 + 3 * i])
        x[b] = np.clip(np.floor(img), 0, 255).astype(np.uint8)
    return x


# ---- SyncNet_color, the lip-sync judge (calipsync_amd/syncnet.py) ----------------------------------------------------
SYNCNET_WEIGHT_SEED = 0x5C1E
SYNCNET_INPUT_SEED = 0x5C1F


def make_syncnet_state_dict(mode: str = "hubert", seed: int = SYNCNET_WEIGHT_SEED) -> Dict[str, np.ndarray]:
    """The 217 entries of a ``SyncNet_color(mode)`` state dict: conv weights N(0, 1 / fan_in) (gain 1.0: at G1.2's 1.2 the
    residual trunk grows to 35), conv biases N(0, 0.05^2), BatchNorm weight and running_var U(0.8, 1.2), bias and running_mean
    N(0, 0.1^2).  Every stage's max |x| then stays between 1.5 and 12 (tests/golden/make_syncnet_golden.py asserts [0.1, 16]).  A
    key of both modes with one shape has one value."""
    from . import syncnet
    sd: Dict[str, np.ndarray] = {}
    for key, shape in syncnet.manifest(mode):
        n = int(np.prod(shape)) if shape else 1
        s = _stream("syncnet." + key)
        block, leaf = key.rsplit(".", 2)[1:]
        if leaf == "num_batches_tracked":
            sd[key] = np.zeros(shape, dtype=np.int64)
            continue
        if block == "0":
            v = normal01(seed, s, n) / np.sqrt(int(np.prod(shape[1:]))) if leaf == "weight" else normal01(seed, s, n) * 0.05
        elif leaf in ("weight", "running_var"):
            v = 0.8 + 0.4 * uniform01(seed, s, n)
        else:
            v = normal01(seed, s, n) * 0.1
        sd[key] = v.astype(np.float32).reshape(shape)
    return sd


def make_syncnet_inputs(batch: int, mode: str = "hubert", seed: int = SYNCNET_INPUT_SEED) -> Tuple[np.ndarray, np.ndarray]:
    """Synthetic pairs: face ~ U(0,1) [B,3,160,160], audio ~ N(0,1) [B,32,32,32] (wenet: [B,256,16,32]); pair b depends only on
    (seed, b) and, the audio window, on the mode's shape."""
    from . import syncnet
    x = np.empty((batch, 3, syncnet.FACE_HW, syncnet.FACE_HW), dtype=np.float32)
    a = np.empty((batch,) + syncnet.AUDIO_SHAPE[mode], dtype=np.float32)
    for b in range(batch):
        x[b] = uniform01(seed, 0x7000000 + b, x[b].size).astype(np.float32).reshape(x[b].shape)
        a[b] = normal01(seed, 0x8000000 + b, a[b].size).astype(np.float32).reshape(a[b].shape)
    return x, a


# ---- the trainer's loss network (calipsync_amd/losses.py) ------------------------------------------------------------
VGG19_WEIGHT_SEED = 0x1619
VGG19_INPUT_SEED = 0x161A


def make_vgg19_state_dict(seed: int = VGG19_WEIGHT_SEED) -> Dict[str, np.ndarray]:
    """The fourteen entries of ``vgg19().features[:15]`` under the state dict's own names (features.{0,2,5,7,10,12,14}.{weight,
    bias}): conv weights N(0, 2 / fan_in) -- the trunk is conv + ReLU throughout, so activations stay O(1) through the seven
    convs on images in [0, 1] -- and biases N(0, 0.05^2)."""
    from . import losses
    sd: Dict[str, np.ndarray] = {}
    for key, shape in losses.manifest():
        n = int(np.prod(shape))
        s = _stream("vgg19." + key)
        v = normal01(seed, s, n) * (0.05 if key.endswith(".bias") else np.sqrt(2.0 / int(np.prod(shape[1:]))))
        sd[key] = v.astype(np.float32).reshape(shape)
    return sd


def make_loss_inputs(batch: int, h: int = 160, w: int = 160, seed: int = VGG19_INPUT_SEED) -> Tuple[np.ndarray, np.ndarray]:
    """(preds, labels) fp32 [B,3,h,w] in [0, 1] as the trainer hands them to its loss: a label of smooth blobs over noise and a
    prediction that is the label plus a perturbation of a tenth of the range; image b depends only on (seed, b, h, w)."""
    frames = make_s3fd_inputs(batch, h, w, seed).astype(np.float64) / 255.0
    labels = np.ascontiguousarray(frames.transpose(0, 3, 1, 2))
    preds = np.empty_like(labels)
    for b in range(batch):
        preds[b] = labels[b] + 0.1 * (uniform01(seed, 0x7000000 + b, 3 * h * w).reshape(3, h, w) - 0.5)
    return np.clip(preds, 0.0, 1.0).astype(np.float32), labels.astype(np.float32)
