"""The CASync U-Net in SEGMENTS, in two arithmetics -- a plain helper module for the tests, not a conftest.

The forward is cut at the taps ``casync_tap`` serves.  A segment takes the tensors the engine had at its start and returns
the tensor at its end (``SEGMENTS``: name of the end tap -> names of the start tensors):

    x -> x1 -> x2 -> x3 -> x4 -> x5          audio -> audio_conv1 -> ... -> audio_conv5 -> a          (x5, a) -> tx
    (ox_prev, a, tx) -> att_i  (ox_prev = tx for i = 0)          (tx, att0..3) -> kx          kx -> fuse
    (fuse, x4) -> u1    (u1, x3) -> u2    (u2, x2) -> u3    (u3, x1) -> u4          u4 -> out

Two forms of every segment:

* ``reference(sd64, name, *src)`` -- FLOAT64: the functions of ``oracle/unet_oracle.py`` on the raw, unfolded state dict cast to
  float64 (mode='wenet': AudioConvWenet's blocks, composed to ``tests/wenet_ref.py``'s forward bit for bit in
  tests/test_unet_bf16_model.py).  Nothing of ``calipsync_amd.pack`` enters it.
* ``Contract(sd).segment(name, *src, **flags)`` -- the EQUAL-CONTRACT MODEL of the bf16 engine, torch on the CPU: the
  BatchNorm-folded weights of ``calipsync_amd.pack.fold``, rounded to fp32 as ``pack.pack`` writes them; every matrix the
  handle reads through ``WG(...)`` (engine.hip) rounded once more to bf16, what ``f32_to_bf16_kernel`` writes; biases, scale
  vectors, depthwise taps, the stem's and the head's weights fp32; every sum fp32; every tensor the engine stores as bf16
  -- in HBM, in LDS or as a matrix operand -- rounded to bf16 (round to nearest even) at that point.
  ``Contract(sd, rounding=False)`` is the same arithmetic with no rounding at all (fp32 folded weights): the composition
  then equals ``unet_oracle.forward`` up to the fold and fp32 reassociation (tests/test_unet_bf16_model.py: <= 1e-5).

The rounding points, read off the kernels (R = one rounding to bf16; everything else fp32):

inverted residual, every form -- E = R(lrelu(W1.x + b1)), D = R(lrelu(dw3x3(E) + bd)), y = R(lrelu(W2.D + b2) [+ x]):
  * un-fused chain (``Plan::ir``'s last branch: pw_gemm -> dw3x3_kernel / dw3x3_lds_kernel -> pw_gemm): E and D are bf16
    tensors in HBM, the residual x is read back as bf16 and added in fp32 behind the activation (epilogue_rows_cols:
    bias, [pre-residual], LReLU, post-residual, [second affine + LReLU], store);
  * ``pw_dw_bf16_kernel`` / ``_strip_kernel`` / ``_rect_kernel``: E is a bf16 image in LDS (e_store), D bf16 in HBM;
  * ``ir_fused_bf16_kernel``: E bf16 in LDS, D converted to bf16 as the B operand of the project MFMA, y from the
    accumulators.  With ``ir_dw_mfma`` the nine depthwise taps enter the product ROUNDED TO BF16 (flag ``dw_taps_bf16``: 1 = every
    fused instance but the 64 -> 128 -> 32 one, i.e. up4.0; 2 = all; 0 = fp32 taps).  ``FUSED`` lists the blocks that
    kernel takes (fuse_ir, hw >= 32, the channel counts of ir_fused_supported): the choice does not depend on the batch.
  * the Up blocks the fused kernel takes (up3.0 / up4.0) compute the bilinear x2 of ``lo`` while loading their A fragments
    and convert it to bf16: the same contract as the materialised route below.
Up block, first inverted residual (``commute_up``: the stages whose expand conv is commuted; the engine: up1 and up2 from
``fuse_dw_bf16_min`` frames per launch, up2 only with fuse_dw_bf16 >= 2):
  * materialised (``upsample2x_kernel<__bf16>``): cat = [R(up(lo)), skip], E = R(lrelu(W1.cat + b1));
  * commuted (``UpMode::CommuteUnfused``): G = R(W1a.lo) at the low resolution (no bias), E = R(lrelu(W1b.skip + b1 + up(G))),
    up() in fp32 (ups_at_lds_b).
audio encoder: the NCHW fp32 window is stored as bf16 NHWC first (``nchw_to_nhwc_kernel<__bf16>``: R(audio)); conv3 / conv5
  are implicit GEMMs: R(act(W.x + b)), LeakyReLU (wenet: ReLU); HuBERT's conv7 carries bn7 + LReLU as the second affine of
  its project GEMM: R(lrelu(s7 (lrelu(W2.D + b2) + x) + t7)), nothing rounded in between.  AudioConvWenet's conv1 is a RESIDUAL
  block on the fp32 input (the reference keeps that sum in fp32 under autocast): the engine also stores lo = R(audio - R(audio))
  (``nchw_to_nhwc_kernel<__bf16>`` with lo = 1) and its project GEMM rounds once, R((lrelu(W2.D + b2) + R(audio)) + lo): post-residual,
  then the running-sum output.
fusion MLP: H = R(lrelu(fc1.cat + b)), tx = R(fc2.H + b + rs * cat) (pre-residual, scaled per column; no activation).
attention block i: [ox | q] = R(p1q.prev + b) (query_conv composed into p_1 on the host: 576 columns), [K | V] = R(kv.a + b),
  S = q^T k, P = softmax(S) with fp32 statistics; ``cross_attention_bf16_kernel`` rounds P to bf16 before V.P^T (flag
  ``p_bf16``), ``cross_attention_kernel<__bf16>`` (att_bf16 = 0 or att_nz != 0) does not; AO = R(gamma * O + ox);
  att_i = R(lrelu(b1.AO + b + rs * tx)).
kx: the running sum lives in bf16: KX = R(tx + att0), R(KX + att1), R(KX + att2), kx = R(lrelu(s (KX + att3) + t)).  (The engine
  adds the b_1 GEMM's value BEFORE it is rounded for the att_i tap; a model that starts from the taps cannot: its att_i is
  already rounded.  The difference is below one rounding of the larger running sum.)
stem: ``inc_kernel<__bf16>`` (``inc_mfma`` = 0, the default) computes the whole block in fp32 from the fp32 NCHW input and fp32
  weights; only x1 = R(.) is rounded.
head: ``outc_kernel<__bf16>``: fp32 weights and sums on the bf16 u4, 1 / (1 + exp(-s)) in fp32, fp32 NCHW out: no rounding.
model boundary: taps come back as bf16 (widened by ``Model.tap``); x, audio and out are fp32 NCHW.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from calipsync_amd import pack
from oracle import unet_oracle as uo
from oracle.unet_oracle import _act, _bn

SLOPE = 0.01
_AUDIO = (("audio_conv1", ("audio",)), ("audio_conv2", ("audio_conv1",)), ("audio_conv3", ("audio_conv2",)),
          ("audio_conv4", ("audio_conv3",)), ("audio_conv5", ("audio_conv4",)), ("a", ("audio_conv5",)))
SEGMENTS: Tuple[Tuple[str, Tuple[str, ...]], ...] = (
    ("x1", ("x",)), ("x2", ("x1",)), ("x3", ("x2",)), ("x4", ("x3",)), ("x5", ("x4",))) + _AUDIO + (
    ("tx", ("x5", "a")), ("att0", ("tx", "a", "tx")), ("att1", ("att0", "a", "tx")), ("att2", ("att1", "a", "tx")),
    ("att3", ("att2", "a", "tx")), ("kx", ("tx", "att0", "att1", "att2", "att3")), ("fuse", ("kx",)),
    ("u1", ("fuse", "x4")), ("u2", ("u1", "x3")), ("u3", ("u2", "x2")), ("u4", ("u3", "x1")), ("out", ("u4",)))
SOURCES = dict(SEGMENTS)
AUDIO_SEGMENTS = tuple(n for n, _ in _AUDIO)
_DOWN = {"x2": "down1", "x3": "down2", "x4": "down3", "x5": "down4"}
_UP = {"u1": "up1", "u2": "up2", "u3": "up3", "u4": "up4"}
# the blocks ir_fused_bf16_kernel takes (mode='hubert'; wenet's 16x32 conv1 / conv2 are not square: pw_dw_bf16_rect or the chain)
FUSED = ("down1.maxpool_conv.0.double_conv.0", "down1.maxpool_conv.0.double_conv.1", "down2.maxpool_conv.0.double_conv.0",
         "audio_model.conv1", "audio_model.conv2", "up2.conv.double_conv.1", "up3.conv.double_conv.0", "up3.conv.double_conv.1",
         "up4.conv.double_conv.0", "up4.conv.double_conv.1")
VALU_AT_1 = "up4.conv.double_conv.0"      # ir_dw_mfma = 1 leaves the 64 -> 128 -> 32 instance on the vector pipe (fp32 taps)
# which segments a flag can move (tests/test_unet_bf16_model.py holds the model to it; the GPU option legs re-check these)
FLAG_SEGMENTS = {"commute_up": ("u1", "u2"), "p_bf16": ("att0", "att1", "att2", "att3"),
                 "dw_taps_bf16": ("x2", "x3", "audio_conv1", "audio_conv2", "u2", "u3", "u4")}
DEFAULT_FLAGS = dict(commute_up=("up1", "up2"), dw_taps_bf16=1, p_bf16=True)


def bf16(t: torch.Tensor) -> torch.Tensor:
    """one rounding to bf16 (nearest even), widened again"""
    return t.bfloat16().float()


def _same(t: torch.Tensor) -> torch.Tensor:
    return t


# ====================================================================== float64 reference
def to64(sd_np: dict) -> Dict[str, torch.Tensor]:
    return uo.to_torch(sd_np, torch.float64)


def _dense(sd, p: str, bn: str, x, stride, pad, relu: bool):
    y = _bn(sd, f"{p}.{bn}", F.conv2d(x, sd[f"{p}.conv{bn[2:]}.weight"], sd[f"{p}.conv{bn[2:]}.bias"], stride, pad))
    return F.relu(y) if relu else _act(y)


@torch.no_grad()
def reference(sd, name: str, *src: torch.Tensor, mode: str = "hubert") -> torch.Tensor:
    """segment ``name`` from its start tensors by the oracle's functions, in the dtype of ``sd`` (float64 for the tests)"""
    dt = sd["outc.conv.weight"].dtype
    s = [t.to(dt) for t in src]
    wenet = mode == "wenet"
    if name == "x1":
        return uo.inverted_residual(sd, "inc.inconv.0", s[0], 1, False)
    if name in _DOWN:
        return uo.double_conv(sd, f"{_DOWN[name]}.maxpool_conv.0", s[0], 2)
    if name == "audio_conv1":
        return uo.inverted_residual(sd, "audio_model.conv1", s[0], 1, wenet)
    if name == "audio_conv2":
        return uo.inverted_residual(sd, "audio_model.conv2", s[0], 1, wenet)
    if name == "audio_conv3":
        return _dense(sd, "audio_model", "bn3", s[0], (1, 2) if wenet else 2, 1, wenet)
    if name == "audio_conv4":
        return uo.inverted_residual(sd, "audio_model.conv4", s[0], 1, True)
    if name == "audio_conv5":
        return _dense(sd, "audio_model", "bn5", s[0], 2, 3, wenet)
    if name == "a":
        a = uo.inverted_residual(sd, "audio_model.conv6", s[0], 1, True)
        a = uo.inverted_residual(sd, "audio_model.conv7", a, 1, True)
        return a if wenet else _act(_bn(sd, "audio_model.bn7", a))
    if name == "tx":
        return _bn(sd, "bn_tx", torch.cat([s[0], s[1]], 1) + uo.mlp_fusion(sd, s[0], s[1]))
    if name.startswith("att"):
        return uo.attention_block(sd, f"attention_blocks.{name[3:]}", s[0], s[1], s[2])
    if name == "kx":
        kx = s[0]
        for ox in s[1:]:
            kx = ox + kx
        return _act(_bn(sd, "bn_kx", kx))
    if name == "fuse":
        return uo.double_conv(sd, "fuse_conv.1", uo.double_conv(sd, "fuse_conv.0", s[0], 1), 1)
    if name in _UP:
        return uo.up_block(sd, _UP[name], s[0], s[1])
    if name == "out":
        return torch.sigmoid(_bn(sd, "outc_bn", F.conv2d(s[0], sd["outc.conv.weight"], sd["outc.conv.bias"])))
    raise KeyError(name)


# ====================================================================== the equal-contract model
def _lrelu(t):
    return F.leaky_relu(t, SLOPE)


def _up(t):
    return F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)


class Contract:
    """The bf16 engine's arithmetic on the CPU (module docstring).  ``rounding=False``: fp32 folded weights, nothing rounded."""

    def __init__(self, sd_np: dict, mode: str = "hubert", rounding: bool = True):
        self.mode, self.wenet = mode, mode == "wenet"
        self.r = bf16 if rounding else _same
        self.f = {k: torch.from_numpy(np.ascontiguousarray(v).astype(np.float32)) for k, v in pack.fold(sd_np, mode).items()}
        self._wg: Dict[str, torch.Tensor] = {}

    # ---- weights
    def W(self, name: str) -> torch.Tensor:
        """an fp32 tensor of the handle: bias, scale, depthwise taps"""
        return self.f[name]

    def WG(self, name: str) -> torch.Tensor:
        """a GEMM matrix as the bf16 handle stores it"""
        if name not in self._wg:
            self._wg[name] = self.r(self.f[name])
        return self._wg[name]

    # ---- operators (NCHW fp32 in and out)
    @staticmethod
    def _pw(x, w, b=None):
        return F.conv2d(x, w.reshape(w.shape[0], w.shape[1], 1, 1), b)

    def _dw(self, e, p: str, stride, taps_bf16: bool):
        wd = self.W(f"{p}.dw.w")                                  # tap-major [9][C]
        if taps_bf16:
            wd = self.r(wd)
        c = wd.shape[1]
        return F.conv2d(e, wd.t().reshape(c, 1, 3, 3), self.W(f"{p}.dw.b"), stride, 1, 1, c)

    def _taps_bf16(self, p: str, dw_taps_bf16: int) -> bool:
        return p in FUSED and not self.wenet_rect(p) and (dw_taps_bf16 >= 2 or (dw_taps_bf16 == 1 and p != VALU_AT_1))

    def wenet_rect(self, p: str) -> bool:
        return self.wenet and p in ("audio_model.conv1", "audio_model.conv2")

    def _ir(self, p: str, x, stride: int, res: bool, dw_taps_bf16: int, e=None, affine=None, res_lo=None):
        """one inverted residual; ``e``: the expand conv's pre-activation when the caller built it (an Up block); ``res_lo``: a second
        residual addend, added in fp32 behind the first (wenet's conv1: the low half of the fp32 window)"""
        r = self.r
        if e is None:
            e = self._pw(x, self.WG(f"{p}.pw1.w"), self.W(f"{p}.pw1.b"))
        e = r(_lrelu(e))
        d = r(_lrelu(self._dw(e, p, stride, self._taps_bf16(p, dw_taps_bf16))))
        y = _lrelu(self._pw(d, self.WG(f"{p}.pw2.w"), self.W(f"{p}.pw2.b")))
        if res:
            y = y + x
        if res_lo is not None:
            y = res_lo + y
        if affine is not None:
            y = _lrelu(y * affine[0].reshape(1, -1, 1, 1) + affine[1].reshape(1, -1, 1, 1))
        return r(y)

    def _double(self, p: str, x, stride: int, dw_taps_bf16: int):
        x = self._ir(f"{p}.double_conv.0", x, stride, False, dw_taps_bf16)
        return self._ir(f"{p}.double_conv.1", x, 1, True, dw_taps_bf16)

    def _inc(self, x):
        """inc_kernel<__bf16>: fp32 weights, fp32 E and D, one rounding at the end"""
        v = self.f["inc.inconv.0.fused"]
        w1, b1, wd, bd = v[:72].reshape(6, 12).t(), v[72:84], v[84:192].reshape(9, 12), v[192:204]
        w2, b2 = v[204:588].reshape(12, 32).t(), v[588:620]
        e = _lrelu(self._pw(x, w1.contiguous(), b1))
        d = _lrelu(F.conv2d(e, wd.t().reshape(12, 1, 3, 3), bd, 1, 1, 1, 12))
        return self.r(_lrelu(self._pw(d, w2.contiguous(), b2)))

    def _dense(self, name: str, x, stride, pad):
        w = self.WG(f"{name}.w")                                  # [N][(ky, kx, cin)]
        n, cin = w.shape[0], x.shape[1]
        y = F.conv2d(x, w.reshape(n, 3, 3, cin).permute(0, 3, 1, 2).contiguous(), self.W(f"{name}.b"), stride, pad)
        return self.r(F.relu(y) if self.wenet else _lrelu(y))

    def _up_block(self, stage: str, lo, skip, commute: bool, dw_taps_bf16: int):
        r, p = self.r, f"{stage}.conv.double_conv.0"
        if commute:
            g = r(self._pw(lo, self.WG(f"{p}.pw1a.w")))
            e = self._pw(skip, self.WG(f"{p}.pw1b.w"), self.W(f"{p}.pw1.b")) + _up(g)
        else:
            e = self._pw(torch.cat([r(_up(lo)), skip], 1), self.WG(f"{p}.pw1.w"), self.W(f"{p}.pw1.b"))
        t = self._ir(p, None, 1, False, dw_taps_bf16, e=e)
        return self._ir(f"{stage}.conv.double_conv.1", t, 1, True, dw_taps_bf16)

    def _attention(self, i: int, prev, a, tx, p_bf16: bool):
        r, p = self.r, f"attention_blocks.{i}"
        b, _, h, w = prev.shape
        n = h * w
        p1q = r(self._pw(prev, self.WG(f"{p}.p1q.w"), self.W(f"{p}.p1q.b")))
        ox, q = p1q[:, :512], p1q[:, 512:].reshape(b, 64, n)
        kv = r(self._pw(a, self.WG("att.kv.w")[576 * i:576 * (i + 1)], self.W("att.kv.b")[576 * i:576 * (i + 1)]))
        k, v = kv[:, :64].reshape(b, 64, n), kv[:, 64:].reshape(b, 512, n)
        att = torch.softmax(torch.bmm(q.transpose(1, 2), k), dim=-1)          # [B, n_face, n_audio], fp32 statistics
        if p_bf16:
            att = r(att)
        o = torch.bmm(v, att.transpose(1, 2)).reshape(b, 512, h, w)
        ao = r(self.W(f"{p}.gamma") * o + ox)
        y = self._pw(ao, self.WG(f"{p}.b1.w"), self.W(f"{p}.b1.b")) + self.W(f"{p}.b1.rs").reshape(1, -1, 1, 1) * tx
        return r(_lrelu(y))

    # ---- segments
    @torch.no_grad()
    def segment(self, name: str, *src: torch.Tensor, commute_up=DEFAULT_FLAGS["commute_up"],
                dw_taps_bf16: int = DEFAULT_FLAGS["dw_taps_bf16"], p_bf16: bool = DEFAULT_FLAGS["p_bf16"]) -> torch.Tensor:
        r = self.r
        s = [t.float() for t in src]
        if commute_up is True:
            commute_up = ("up1", "up2")
        commute_up = tuple(commute_up or ())
        assert set(commute_up) <= {"up1", "up2"}, "the engine commutes the expand conv of up1.0 / up2.0 only"
        if name == "x1":
            return self._inc(s[0])
        if name in _DOWN:
            return self._double(f"{_DOWN[name]}.maxpool_conv.0", s[0], 2, dw_taps_bf16)
        if name == "audio_conv1":                                   # the boundary: the fp32 window is stored as bf16 first
            hi = r(s[0])
            lo = r(s[0] - hi) if self.wenet else None               # wenet: conv1's residual add takes the window as hi + lo
            return self._ir("audio_model.conv1", hi, 1, self.wenet, dw_taps_bf16, res_lo=lo)
        if name == "audio_conv2":
            return self._ir("audio_model.conv2", s[0], 1, self.wenet, dw_taps_bf16)
        if name == "audio_conv3":
            return self._dense("audio_model.conv3", s[0], (1, 2) if self.wenet else 2, 1)
        if name == "audio_conv4":
            return self._ir("audio_model.conv4", s[0], 1, True, dw_taps_bf16)
        if name == "audio_conv5":
            return self._dense("audio_model.conv5", s[0], 2, 3)
        if name == "a":
            a = self._ir("audio_model.conv6", s[0], 1, True, dw_taps_bf16)
            bn7 = None if self.wenet else (self.W("audio_model.bn7.s"), self.W("audio_model.bn7.t"))
            return self._ir("audio_model.conv7", a, 1, True, dw_taps_bf16, affine=bn7)
        if name == "tx":
            cat = torch.cat([s[0], s[1]], 1)
            h = r(_lrelu(self._pw(cat, self.WG("mlp_fusion.fc1.w"), self.W("mlp_fusion.fc1.b"))))
            return r(self._pw(h, self.WG("mlp_fusion.fc2.w"), self.W("mlp_fusion.fc2.b")) +
                     self.W("mlp_fusion.fc2.rs").reshape(1, -1, 1, 1) * cat)
        if name.startswith("att"):
            return self._attention(int(name[3:]), s[0], s[1], s[2], p_bf16)
        if name == "kx":
            kx = s[0]
            for ox in s[1:4]:
                kx = r(kx + ox)
            return r(_lrelu((kx + s[4]) * self.W("bn_kx.s").reshape(1, -1, 1, 1) + self.W("bn_kx.t").reshape(1, -1, 1, 1)))
        if name == "fuse":
            return self._double("fuse_conv.1", self._double("fuse_conv.0", s[0], 1, dw_taps_bf16), 1, dw_taps_bf16)
        if name in _UP:
            return self._up_block(_UP[name], s[0], s[1], _UP[name] in commute_up, dw_taps_bf16)
        if name == "out":
            y = self._pw(s[0], self.W("outc.w").reshape(3, 32), self.W("outc.b"))
            return 1.0 / (1.0 + torch.exp(-y))
        raise KeyError(name)


def compose(step, x: torch.Tensor, audio: torch.Tensor) -> Dict[str, torch.Tensor]:
    """every tap of a forward built from the segments, each fed with the previous ones' outputs: ``step(name, *src)``"""
    t = {"x": x, "audio": audio}
    for name, srcs in SEGMENTS:
        t[name] = step(name, *[t[k] for k in srcs])
    return t
