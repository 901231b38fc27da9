// HuBERT-large feature extractor (transformers HubertModel with do_stable_layer_norm, fp32) on gfx950.
//
// Replaces the stock-torch model behind HubertExtractor.extract_features (image_infer_v1/utils/hubert_extractor.py).
// Activations are channels-last ([rows][channels], rows = (sequence, time)), so every layer is one of:
//   conv0 + LayerNorm + GELU      hb_conv0_kernel       (1 input channel, k=10, s=5: a dot of 10 per output)
//   conv1..6                      launch_rows_gemm      (k=3/2, s=2 over 512 channels: overlapping A rows, lda = 2*512)
//   LayerNorm (+ GELU)            hb_layernorm_kernel   (512 or 1024 columns, one row per wave, two-pass in registers)
//   linear layers                 launch_rows_gemm      (bias, exact GELU, post-residual in the epilogue)
//   positional conv               hb_posconv_kernel     (k=128, 16 groups of 64: implicit GEMM on v_mfma_f32_32x32x2_f32)
//   self-attention                hb_attention_kernel   (16 heads of 64, online softmax, scores stay in registers)
// The feature-encoder GEMMs run one launch per sequence: with an odd input length the rows of the next sequence do not
// continue the overlapping-row pattern.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "handle.h"

namespace {

constexpr int kHid = 1024, kConvC = 512, kHeads = 16, kHeadD = 64, kFF = 4096;
constexpr int kPosK = 128, kPosG = 16, kPosC = 64;   // positional conv: kernel, groups, channels per group
constexpr float kEps = 1e-5f;
constexpr int kConvK[7] = {10, 3, 3, 3, 3, 2, 2};
constexpr int kConvS[7] = {5, 2, 2, 2, 2, 2, 2};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- conv0 (1 -> 512, k=10, s=5) + LayerNorm(512) + GELU --------------------------------------------------------------
// One wave per output row; lane owns channels 4*lane..+3 and 256+4*lane..+3 and keeps their taps in registers.
__global__ __launch_bounds__(256) void hb_conv0_kernel(const float* __restrict__ wave, int S, int T0, int rows,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       const float* __restrict__ g, const float* __restrict__ be,
                                                       float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  float wr[8][10], br[8], gr[8], er[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = (j >> 2) * 256 + 4 * lane + (j & 3);
#pragma unroll
    for (int k = 0; k < 10; ++k) wr[j][k] = w[c * 10 + k];
    br[j] = bias[c], gr[j] = g[c], er[j] = be[c];
  }
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {
    const int b = r / T0, t = r - b * T0;
    const float* xs = wave + (size_t)b * S + (size_t)5 * t;
    float xv[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) xv[k] = xs[k];
    float v[8], s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float a = br[j];
#pragma unroll
      for (int k = 0; k < 10; ++k) a = fmaf(wr[j][k], xv[k], a);
      v[j] = a, s += a;
    }
    const float mean = wave_sum(s) * (1.f / kConvC);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] -= mean, q += v[j] * v[j];
    const float inv = 1.f / sqrtf(wave_sum(q) * (1.f / kConvC) + kEps);
    f32x4 o[2];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j >> 2][j & 3] = gelu_erf(fmaf(v[j] * inv, gr[j], er[j]));
    float* dst = out + (size_t)r * kConvC + 4 * lane;
    *reinterpret_cast<f32x4*>(dst) = o[0];
    *reinterpret_cast<f32x4*>(dst + 256) = o[1];
  }
}

// ---- LayerNorm over C columns (+ exact GELU), one row per wave ------------------------------------------------------
// in == out is allowed (every lane reads its own elements before it writes them).
template <int C, bool GELU>
__global__ __launch_bounds__(256) void hb_layernorm_kernel(const float* in, int ldi, float* out, int ldo, int rows,
                                                           const float* __restrict__ g, const float* __restrict__ be, float eps) {
  constexpr int NV = C / 256;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* p = in + (size_t)row * ldi + 4 * lane;
  f32x4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    v[j] = *reinterpret_cast<const f32x4*>(p + 256 * j);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s += v[j][e];
      asm("" : "+v"(s));   // a scalar chain: the compiler pairs these adds into v_pk_add_f32 with op_sel otherwise
    }
  }
  const float mean = wave_sum(s) * (1.f / C);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = v[j][e] - mean;
      v[j][e] = d, q += d * d;
    }
  const float inv = 1.f / sqrtf(wave_sum(q) * (1.f / C) + eps);
  float* d = out + (size_t)row * ldo + 4 * lane;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const f32x4 gg = *reinterpret_cast<const f32x4*>(g + 256 * j + 4 * lane);
    const f32x4 bb = *reinterpret_cast<const f32x4*>(be + 256 * j + 4 * lane);
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = v[j][e] * inv;
      asm("" : "+v"(t));   // element by element: no packed multiply taking a scalar from a register pair's high half
      t = fmaf(t, gg[e], bb[e]);
      y[e] = GELU ? gelu_erf(t) : t;
    }
    *reinterpret_cast<f32x4*>(d + 256 * j) = y;
  }
}

// ---- grouped positional conv: out = x + GELU(conv(x) + bias), k=128, pad 64, last step dropped ------------------------
// Output row t of group g: sum over taps k and channels c of x[t + k - 64, 64g + c] * w[g][k][n][c].  A workgroup owns 64
// rows x the 64 channels of one group; the 191 input rows it touches sit in LDS once, so each tap's k-tile is that block
// shifted by one row.  The tap's 64x64 weight tile is prefetched into registers while the previous tap computes.
constexpr int kPcRows = 192, kPcLd = 68;   // LDS row stride 68 floats: conflict-free b128 reads per lane group
constexpr int kPcLds = (kPcRows + 64) * kPcLd * 4;
__global__ __launch_bounds__(256) void hb_posconv_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                         const float* __restrict__ bias, float* __restrict__ out, int T) {
  extern __shared__ __attribute__((aligned(16))) float pc_smem[];
  float* xs = pc_smem;                      // [192][68]: rows t0-64 .. t0+127
  float* ws = pc_smem + kPcRows * kPcLd;    // [64][68]:  w[g][tap][n][c]
  const int t0 = blockIdx.x * 64, g = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1, c32 = lane & 31, kh = lane >> 5;
  const float* xb = x + (size_t)b * T * kHid + g * kPosC;
  for (int idx = tid; idx < kPcRows * 16; idx += 256) {
    const int r = idx >> 4, c4 = (idx & 15) * 4, t = t0 - 64 + r;
    const f32x4 v = t >= 0 && t < T ? *reinterpret_cast<const f32x4*>(xb + (size_t)t * kHid + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(xs + r * kPcLd + c4) = v;
  }
  const float* wg = wp + (size_t)g * kPosK * 4096;
  f32x4 wr[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) wr[q] = *reinterpret_cast<const f32x4*>(wg + (tid + 256 * q) * 4);
  f32x16 acc = {};
  for (int tap = 0; tap < kPosK; ++tap) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = tid + 256 * q;
      *reinterpret_cast<f32x4*>(ws + (idx >> 4) * kPcLd + (idx & 15) * 4) = wr[q];
    }
    __syncthreads();
    if (tap + 1 < kPosK) {
#pragma unroll
      for (int q = 0; q < 4; ++q) wr[q] = *reinterpret_cast<const f32x4*>(wg + (size_t)(tap + 1) * 4096 + (tid + 256 * q) * 4);
    }
    // A[i][c] = xs[i + tap][c], B[c][n] = ws[n][c]; lane half kh takes c = 8q + 4kh .. +3 of every 8 (same order for both)
    const float* arow = xs + (wm * 32 + c32 + tap) * kPcLd + 4 * kh;
    const float* brow = ws + (wn * 32 + c32) * kPcLd + 4 * kh;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(arow + 8 * q), bb = *reinterpret_cast<const f32x4*>(brow + 8 * q);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bb[s], acc, 0, 0, 0);
    }
  }
  const int n = g * kPosC + wn * 32 + c32;
  const float bn = bias[n];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int t = t0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
    if (t < T) {
      const size_t o = ((size_t)b * T + t) * kHid + n;
      out[o] = x[o] + gelu_erf(acc[r] + bn);
    }
  }
}

// ---- self-attention, 16 heads of 64, any T >= 1 ---------------------------------------------------------------------
// qkv: [B*T][3072] = (q pre-scaled by 1/8 | k | v), out: [B*T][1024].  A wave owns 32 queries of one head and walks the
// keys in tiles of 32 staged in LDS (shared by the workgroup's waves).  S^T = K Q^T puts one query per lane column, so the
// softmax statistics of a query live in one lane pair (l, l^32); P^T is consumed straight from the accumulator registers
// as the B operand of O^T = V^T P^T (k order = the accumulator's row order, the same for A and B).  No score touches HBM.
constexpr int kAttWaves = 2, kAttLd = 68;
__global__ __launch_bounds__(64 * kAttWaves) void hb_attention_kernel(const float* __restrict__ qkv, float* __restrict__ out, int T) {
  __shared__ __attribute__((aligned(16))) float Ks[32 * kAttLd];
  __shared__ __attribute__((aligned(16))) float Vs[32 * kAttLd];
  const int head = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, c32 = lane & 31, h = lane >> 5;
  const int i0 = (blockIdx.x * kAttWaves + (tid >> 6)) * 32, qi = i0 + c32;
  const float* base = qkv + (size_t)b * T * (3 * kHid) + head * kHeadD;
  f32x4 q[8];   // Q[qi][8g + 4h .. +3]
#pragma unroll
  for (int g = 0; g < 8; ++g)
    q[g] = qi < T ? *reinterpret_cast<const f32x4*>(base + (size_t)qi * (3 * kHid) + 8 * g + 4 * h) : f32x4{0.f, 0.f, 0.f, 0.f};
  f32x16 o0 = {}, o1 = {};
  float m = -INFINITY, l = 0.f;
  for (int j0 = 0; j0 < T; j0 += 32) {
    __syncthreads();
    for (int idx = tid; idx < 1024; idx += 64 * kAttWaves) {
      const int which = idx >> 9, r = (idx >> 4) & 31, c4 = (idx & 15) * 4, j = j0 + r;
      const f32x4 v = j < T ? *reinterpret_cast<const f32x4*>(base + (size_t)j * (3 * kHid) + kHid * (1 + which) + c4)
                            : f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>((which ? Vs : Ks) + r * kAttLd + c4) = v;
    }
    __syncthreads();
    f32x16 s = {};
    const float* krow = Ks + c32 * kAttLd + 4 * h;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const f32x4 kv = *reinterpret_cast<const f32x4*>(krow + 8 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[e], q[g][e], s, 0, 0, 0);
    }
    // s[r] = S^T[key j0 + (r&3) + 8(r>>2) + 4h][query qi]
    if (j0 + 32 > T) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (j0 + (r & 3) + 8 * (r >> 2) + 4 * h >= T) s[r] = -INFINITY;
    }
    float mx = s[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx), alpha = expf(m - mn);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = expf(s[r] - mn);
      ps += s[r];
    }
    l = l * alpha + ps;
    m = mn;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float a0 = o0[r], a1 = o1[r];
      asm("" : "+v"(a0), "+v"(a1));
      o0[r] = a0 * alpha, o1[r] = a1 * alpha;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* vrow = Vs + ((r & 3) + 8 * (r >> 2) + 4 * h) * kAttLd + c32;
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[0], s[r], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32], s[r], o1, 0, 0, 0);
    }
  }
  const float inv = 1.f / (l + __shfl_xor(l, 32));
  if (qi < T) {
    float* dst = out + ((size_t)b * T + qi) * kHid + head * kHeadD;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int e = (r & 3) + 8 * (r >> 2) + 4 * h;
      dst[e] = o0[r] * inv;
      dst[e + 32] = o1[r] * inv;
    }
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------
int launch_conv0(const float* wave, int batch, int S, const float* w, const float* b, const float* g, const float* be,
                 float* out, hipStream_t s) {
  CASYNC_REQUIRE(wave && w && b && g && be && out && batch > 0 && S >= 10, "hubert conv0: bad args (S=%d)", S);
  const int T0 = (S - 10) / 5 + 1;
  const long long rows = (long long)batch * T0;
  CASYNC_REQUIRE(rows < (1ll << 31), "hubert conv0: too many rows");
  const long long want = (rows + 3) / 4;
  const unsigned grid = (unsigned)(want < 4096 ? want : 4096);
  return casync_launch(hb_conv0_kernel, dim3(grid), dim3(256), 0, s, wave, S, T0, (int)rows, w, b, g, be, out);
}

int launch_layernorm(const float* in, int ldi, float* out, int ldo, int rows, int cols, const float* g, const float* b,
                     float eps, bool gelu, hipStream_t s) {
  CASYNC_REQUIRE(in && out && g && b && rows > 0, "hubert layernorm: bad args");
  CASYNC_REQUIRE(cols == 512 || cols == 1024, "hubert layernorm: %d columns (512 or 1024)", cols);
  CASYNC_REQUIRE(ldi >= cols && ldo >= cols && ldi % 4 == 0 && ldo % 4 == 0 && (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0,
                 "hubert layernorm: leading dimensions / alignment");
  const dim3 grid((rows + 3) / 4);
  if (cols == 512)
    return gelu ? casync_launch(hb_layernorm_kernel<512, true>, grid, dim3(256), 0, s, in, ldi, out, ldo, rows, g, b, eps)
                : casync_launch(hb_layernorm_kernel<512, false>, grid, dim3(256), 0, s, in, ldi, out, ldo, rows, g, b, eps);
  return gelu ? casync_launch(hb_layernorm_kernel<1024, true>, grid, dim3(256), 0, s, in, ldi, out, ldo, rows, g, b, eps)
              : casync_launch(hb_layernorm_kernel<1024, false>, grid, dim3(256), 0, s, in, ldi, out, ldo, rows, g, b, eps);
}

int launch_posconv(const float* x, const float* wp, const float* bias, float* out, int batch, int T, hipStream_t s) {
  CASYNC_REQUIRE(x && wp && bias && out && batch > 0 && T > 0 && batch <= 65535, "hubert posconv: bad args");
  CASYNC_REQUIRE(x != out, "hubert posconv: in place is not supported");
  static unsigned long long attr_once = 0;
  if (int st = casync_ensure_dyn_lds(&attr_once, reinterpret_cast<const void*>(hb_posconv_kernel), kPcLds)) return st;
  return casync_launch(hb_posconv_kernel, dim3((T + 63) / 64, kPosG, batch), dim3(256), kPcLds, s, x, wp, bias, out, T);
}

int launch_attention(const float* qkv, float* out, int batch, int T, hipStream_t s) {
  CASYNC_REQUIRE(qkv && out && batch > 0 && T > 0 && batch <= 65535, "hubert attention: bad args");
  return casync_launch(hb_attention_kernel, dim3((T + 32 * kAttWaves - 1) / (32 * kAttWaves), kHeads, batch),
                       dim3(64 * kAttWaves), 0, s, qkv, out, T);
}

// ---- packed layout ---------------------------------------------------------------------------------------------------
constexpr int kMaxLayers = 48;

// the packed layout of a model of `layers` layers with every tensor's offset resolved once (as DetLayout of facedet.hip): a
// forward builds no name and searches nothing
struct HbLayout {
  struct Conv {
    int64_t w, b, g, be;   // conv weight and bias, LayerNorm gain and bias
  };
  struct Layer {
    int64_t ln1_g, ln1_b, qkv_w, qkv_b, o_w, o_b, ln2_g, ln2_b, ff1_w, ff1_b, ff2_w, ff2_b;
  };
  PackedLayout packed;
  Conv fe[7];
  int64_t fp_ln_g, fp_ln_b, fp_w, fp_b, pos_w, pos_b, enc_ln_g, enc_ln_b;
  std::vector<Layer> layer;
  explicit HbLayout(int layers) : layer(layers) {
    auto add = [this](const std::string& n, int64_t size) { return packed.add(n, size); };
    for (int i = 0; i < 7; ++i) {
      const std::string p = "fe.conv" + std::to_string(i), ln = "fe.ln" + std::to_string(i);
      fe[i].w = add(p + ".w", (int64_t)kConvC * (i ? kConvC : 1) * kConvK[i]);   // [cout][tap][cin]
      fe[i].b = add(p + ".b", kConvC);
      fe[i].g = add(ln + ".g", kConvC), fe[i].be = add(ln + ".b", kConvC);
    }
    fp_ln_g = add("fp.ln.g", kConvC), fp_ln_b = add("fp.ln.b", kConvC);
    fp_w = add("fp.w", (int64_t)kHid * kConvC), fp_b = add("fp.b", kHid);
    pos_w = add("pos.w", (int64_t)kPosG * kPosK * kPosC * kPosC);   // [group][tap][n][c], weight norm folded
    pos_b = add("pos.b", kHid);
    for (int l = 0; l < layers; ++l) {
      const std::string p = "layer" + std::to_string(l);
      Layer& y = layer[l];
      y.ln1_g = add(p + ".ln1.g", kHid), y.ln1_b = add(p + ".ln1.b", kHid);
      y.qkv_w = add(p + ".qkv.w", (int64_t)3 * kHid * kHid);   // [q | k | v][1024], q rows scaled by 1/8
      y.qkv_b = add(p + ".qkv.b", 3 * kHid);
      y.o_w = add(p + ".o.w", (int64_t)kHid * kHid), y.o_b = add(p + ".o.b", kHid);
      y.ln2_g = add(p + ".ln2.g", kHid), y.ln2_b = add(p + ".ln2.b", kHid);
      y.ff1_w = add(p + ".ff1.w", (int64_t)kFF * kHid), y.ff1_b = add(p + ".ff1.b", kFF);
      y.ff2_w = add(p + ".ff2.w", (int64_t)kHid * kFF), y.ff2_b = add(p + ".ff2.b", kHid);
    }
    enc_ln_g = add("enc.ln.g", kHid), enc_ln_b = add("enc.ln.b", kHid);
  }
};

const HbLayout* hb_layout(int layers) {   // null outside 1..kMaxLayers; built on first use, kept for the process
  static const HbLayout* cache[kMaxLayers + 1];
  static std::once_flag once[kMaxLayers + 1];
  if (layers < 1 || layers > kMaxLayers) return nullptr;
  std::call_once(once[layers], [layers] { cache[layers] = new HbLayout(layers); });
  return cache[layers];
}

// time steps after each feature-encoder conv; T[7] = tokens (0 when the waveform is shorter than one receptive field)
struct HbGeom {
  int64_t t[8];
  explicit HbGeom(int64_t S) {
    t[0] = S;
    for (int i = 0; i < 7; ++i) t[i + 1] = t[i] >= kConvK[i] ? (t[i] - kConvK[i]) / kConvS[i] + 1 : 0;
  }
  int64_t tokens() const { return t[7]; }
};

struct HbWs {
  float *a, *b, *h, *x, *big;
  int64_t floats;
  HbWs(float* base, int batch, const HbGeom& G) {
    const int64_t M = batch * G.tokens();
    const int64_t na = round64(batch * G.t[1] * kConvC), nb = round64(batch * G.t[2] * kConvC), nh = round64(M * kHid);
    a = base, b = base ? a + na : nullptr, h = base ? b + nb : nullptr, x = base ? h + nh : nullptr, big = base ? x + nh : nullptr;
    floats = na + nb + 2 * nh + round64(M * kFF);
  }
};

// The bf16 handle's arena: the conv ping-pong and the wide buffer hold bf16, the residual stream h and the feature
// projection's output x stay fp32; once the positional conv has read x, its bytes hold the bf16 LayerNorm / attention output
// (x16) and the bf16 delta of the out-proj / FF2 GEMM (d16).  The fp32 output of the feature projection's LayerNorm sits in
// the wide buffer, which nothing else uses before layer 0.
struct HbWs16 {
  bf16_t *a, *b, *big, *x16, *d16;
  float *h, *x;
  int64_t bytes;
  HbWs16(void* base_v, int batch, const HbGeom& G) {
    char* base = static_cast<char*>(base_v);
    const int64_t M = batch * G.tokens();
    const int64_t na = round64(batch * G.t[1] * kConvC), nb = round64(batch * G.t[2] * kConvC), nh = round64(M * kHid);
    const int64_t nbig = round64(M * kFF);
    int64_t off = 0;
    auto take = [&](int64_t n) {
      char* p = base ? base + off : nullptr;
      off += n;
      return p;
    };
    a = reinterpret_cast<bf16_t*>(take(na * 2)), b = reinterpret_cast<bf16_t*>(take(nb * 2));
    h = reinterpret_cast<float*>(take(nh * 4)), x = reinterpret_cast<float*>(take(nh * 4));
    big = reinterpret_cast<bf16_t*>(take(nbig * 2));
    x16 = reinterpret_cast<bf16_t*>(x), d16 = x ? x16 + nh : nullptr;
    bytes = off;
  }
};

}  // namespace

struct casync_hubert {
  int device = 0;
  int layers = 0;
  int dtype = DT_F32;              // DT_BF16: the bf16 precision (hb_walk16)
  const HbLayout* lay = nullptr;   // hb_layout(layers), set at create
  PackedWeights pw;                // DT_BF16: the GEMM weight matrices are read from the bf16 image
  hipEvent_t ev_fwd = nullptr;     // FwdGate slot
  const float* w(int64_t off) const { return pw.w + off; }   // off: a member of *lay
  const bf16_t* w16(int64_t off) const { return pw.w16 + off; }
};

namespace {
int gemm(const float* a, int lda, const float* w, const float* bias, float* c, int ldc, int m, int n, int k, int act,
         const float* post, hipStream_t s) {
  GemmEpilogue e;
  e.bias = bias;
  e.act = act;
  e.post_res = post;
  e.ld_post = post ? ldc : 0;
  return launch_rows_gemm(a, lda, w, c, ldc, m, n, k, e, s);
}

int copy_out(float* out, const float* src, size_t floats, hipStream_t s) {
  CASYNC_CHECK_HIP(hipMemcpyAsync(out, src, floats * 4, hipMemcpyDeviceToDevice, s));
  return CASYNC_OK;
}

#define HB(call)                        \
  do {                                  \
    if (int st__ = (call)) return st__; \
  } while (0)

// The fp32 walk of a forward hb_run has checked; stage and n_layers as there.
int hb_walk32(const casync_hubert* H, const float* wave, int batch, const HbGeom& G, float* out, const HbWs& ws, hipStream_t s, int stage,
              int n_layers) {
  const HbLayout& L = *H->lay;
  const int T = (int)G.tokens(), M = batch * T;
  // feature encoder: conv0 -> a, then ping-pong a <-> b
  HB(launch_conv0(wave, batch, (int)G.t[0], H->w(L.fe[0].w), H->w(L.fe[0].b), H->w(L.fe[0].g), H->w(L.fe[0].be), ws.a, s));
  float *cur = ws.a, *nxt = ws.b;
  for (int i = 1; i < 7; ++i) {
    const int tin = (int)G.t[i], tout = (int)G.t[i + 1];
    const HbLayout::Conv& c = L.fe[i];
    for (int b = 0; b < batch; ++b)
      HB(gemm(cur + (size_t)b * tin * kConvC, kConvS[i] * kConvC, H->w(c.w), H->w(c.b), nxt + (size_t)b * tout * kConvC, kConvC, tout,
              kConvC, kConvK[i] * kConvC, 0, nullptr, s));
    HB(launch_layernorm(nxt, kConvC, nxt, kConvC, batch * tout, kConvC, H->w(c.g), H->w(c.be), kEps, true, s));
    float* t = cur;
    cur = nxt, nxt = t;
  }
  if (stage == 1) return copy_out(out, cur, (size_t)M * kConvC, s);
  // feature projection, positional conv
  HB(launch_layernorm(cur, kConvC, nxt, kConvC, M, kConvC, H->w(L.fp_ln_g), H->w(L.fp_ln_b), kEps, false, s));
  HB(gemm(nxt, kConvC, H->w(L.fp_w), H->w(L.fp_b), ws.x, kHid, M, kHid, kConvC, 0, nullptr, s));
  HB(launch_posconv(ws.x, H->w(L.pos_w), H->w(L.pos_b), ws.h, batch, T, s));
  if (stage == 2) return copy_out(out, ws.h, (size_t)M * kHid, s);
  const int nl = stage == 3 ? n_layers : H->layers;
  for (int l = 0; l < nl; ++l) {
    const HbLayout::Layer& y = L.layer[l];
    HB(launch_layernorm(ws.h, kHid, ws.x, kHid, M, kHid, H->w(y.ln1_g), H->w(y.ln1_b), kEps, false, s));
    HB(gemm(ws.x, kHid, H->w(y.qkv_w), H->w(y.qkv_b), ws.big, 3 * kHid, M, 3 * kHid, kHid, 0, nullptr, s));
    HB(launch_attention(ws.big, ws.x, batch, T, s));
    HB(gemm(ws.x, kHid, H->w(y.o_w), H->w(y.o_b), ws.h, kHid, M, kHid, kHid, 0, ws.h, s));
    HB(launch_layernorm(ws.h, kHid, ws.x, kHid, M, kHid, H->w(y.ln2_g), H->w(y.ln2_b), kEps, false, s));
    HB(gemm(ws.x, kHid, H->w(y.ff1_w), H->w(y.ff1_b), ws.big, kFF, M, kFF, kHid, 3, nullptr, s));
    HB(gemm(ws.big, kFF, H->w(y.ff2_w), H->w(y.ff2_b), ws.h, kHid, M, kHid, kFF, 0, ws.h, s));
  }
  if (stage == 3) return copy_out(out, ws.h, (size_t)M * kHid, s);
  return launch_layernorm(ws.h, kHid, out, kHid, M, kHid, H->w(L.enc_ln_g), H->w(L.enc_ln_b), kEps, false, s);
}

// The bf16 precision: bf16 GEMM operands and activations, fp32 sums, fp32 residual stream.  The out-proj
// and FF2 GEMMs write a bf16 delta; h += delta happens inside the LayerNorm that follows (LN2, the next layer's LN1, the
// final one), so `pending` says whether d16 still has to be added to h.
int hb_walk16(const casync_hubert* H, const float* wave, int batch, const HbGeom& G, float* out, const HbWs16& ws, hipStream_t s, int stage,
              int n_layers) {
  const HbLayout& L = *H->lay;
  const int T = (int)G.tokens(), M = batch * T;
  // feature encoder: conv0 -> a, then ping-pong a <-> b (bf16)
  HB(launch_hb16_conv0(wave, batch, (int)G.t[0], H->w(L.fe[0].w), H->w(L.fe[0].b), H->w(L.fe[0].g), H->w(L.fe[0].be), ws.a, s));
  bf16_t *cur = ws.a, *nxt = ws.b;
  for (int i = 1; i < 7; ++i) {
    const int tin = (int)G.t[i], tout = (int)G.t[i + 1];
    const HbLayout::Conv& c = L.fe[i];
    for (int b = 0; b < batch; ++b)
      HB(launch_rows_gemm_bf16(cur + (size_t)b * tin * kConvC, kConvS[i] * kConvC, H->w16(c.w), H->w(c.b), nxt + (size_t)b * tout * kConvC,
                               kConvC, tout, kConvC, kConvK[i] * kConvC, s));
    HB(launch_hb16_layernorm512(nxt, kConvC, nxt, kConvC, batch * tout, H->w(c.g), H->w(c.be), kEps, false, true, s));
    bf16_t* t = cur;
    cur = nxt, nxt = t;
  }
  if (stage == 1) return launch_hb16_widen(cur, out, (long long)M * kConvC, s);
  // feature projection and positional conv on the fp32 kernels
  float* ln32 = reinterpret_cast<float*>(ws.big);
  HB(launch_hb16_layernorm512(cur, kConvC, ln32, kConvC, M, H->w(L.fp_ln_g), H->w(L.fp_ln_b), kEps, true, false, s));
  HB(gemm(ln32, kConvC, H->w(L.fp_w), H->w(L.fp_b), ws.x, kHid, M, kHid, kConvC, 0, nullptr, s));
  HB(launch_posconv(ws.x, H->w(L.pos_w), H->w(L.pos_b), ws.h, batch, T, s));
  if (stage == 2) return copy_out(out, ws.h, (size_t)M * kHid, s);
  const int nl = stage == 3 ? n_layers : H->layers;
  bool pending = false;
  for (int l = 0; l < nl; ++l) {
    const HbLayout::Layer& y = L.layer[l];
    HB(launch_hb16_layernorm1024(ws.h, kHid, pending ? ws.d16 : nullptr, kHid, true, ws.x16, kHid, M, H->w(y.ln1_g), H->w(y.ln1_b), kEps,
                                 false, s));
    HB(launch_rows_gemm_bf16(ws.x16, kHid, H->w16(y.qkv_w), H->w(y.qkv_b), ws.big, 3 * kHid, M, 3 * kHid, kHid, s));
    HB(launch_hb16_attention(ws.big, ws.x16, batch, T, s));
    HB(launch_rows_gemm_bf16(ws.x16, kHid, H->w16(y.o_w), H->w(y.o_b), ws.d16, kHid, M, kHid, kHid, s));
    HB(launch_hb16_layernorm1024(ws.h, kHid, ws.d16, kHid, true, ws.x16, kHid, M, H->w(y.ln2_g), H->w(y.ln2_b), kEps, false, s));
    HB(launch_rows_gemm_bf16(ws.x16, kHid, H->w16(y.ff1_w), H->w(y.ff1_b), ws.big, kFF, M, kFF, kHid, s));
    HB(launch_hb16_gelu(ws.big, (long long)M * kFF, s));
    HB(launch_rows_gemm_bf16(ws.big, kFF, H->w16(y.ff2_w), H->w(y.ff2_b), ws.d16, kHid, M, kHid, kFF, s));
    pending = true;
  }
  if (stage == 3) {
    // the tap includes the pending delta: one more pass of the LayerNorm kernel folds it into h (its bf16 output is unused)
    if (pending)
      HB(launch_hb16_layernorm1024(ws.h, kHid, ws.d16, kHid, true, ws.x16, kHid, M, H->w(L.enc_ln_g), H->w(L.enc_ln_b), kEps, false, s));
    return copy_out(out, ws.h, (size_t)M * kHid, s);
  }
  return launch_hb16_layernorm1024(ws.h, kHid, pending ? ws.d16 : nullptr, kHid, false, out, kHid, M, H->w(L.enc_ln_g), H->w(L.enc_ln_b),
                                   kEps, true, s);
}
#undef HB

int64_t hb_workspace_bytes(int dtype, int batch, const HbGeom& G) {
  return dtype == DT_BF16 ? HbWs16(nullptr, batch, G).bytes : HbWs(nullptr, batch, G).floats * 4;
}

// One forward of either precision: the checks, the geometry, the workspace, the device and the forward gate, then the walk.
// stage 0: final hidden states [B,T,1024]; 1: conv-stack output [B,T,512]; 2: input to layer 0 [B,T,1024];
// 3: hidden states after `n_layers` layers, before the final LayerNorm [B,T,1024]
int hb_run(casync_hubert* H, const float* wave, int batch, int64_t S, float* out, void* ws_dev, int64_t ws_bytes, hipStream_t s,
           int stage, int n_layers) {
  CASYNC_REQUIRE(H && wave && out && ws_dev, "hubert forward: null pointer");
  const bool h16 = H->dtype == DT_BF16;
  CASYNC_REQUIRE(H->pw.w && (!h16 || H->pw.w16), "hubert forward: weights not loaded");
  CASYNC_REQUIRE(batch > 0 && batch <= 65535, "hubert forward: batch %d", batch);
  CASYNC_REQUIRE(S < (1ll << 31), "hubert forward: %lld samples", (long long)S);
  const HbGeom G(S);
  CASYNC_REQUIRE(G.tokens() >= 1, "hubert forward: %lld samples give no token (at least 400 are needed)", (long long)S);
  CASYNC_REQUIRE(stage >= 0 && stage <= 3, "hubert forward: stage %d", stage);
  CASYNC_REQUIRE(n_layers >= 0 && n_layers <= H->layers, "hubert forward: %d layers of %d", n_layers, H->layers);
  CASYNC_REQUIRE((uintptr_t)wave % 4 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)ws_dev % 16 == 0, "hubert forward: alignment");
  const int64_t need = hb_workspace_bytes(H->dtype, batch, G);
  if (ws_bytes < need) {
    casync_set_error("hubert forward: workspace %lld bytes, needs %lld", (long long)ws_bytes, (long long)need);
    return CASYNC_ERR_STATE;
  }
  DeviceGuard guard(H->device);
  CASYNC_CHECK_HIP(guard.err);
  std::unique_lock<std::mutex> gate_lock;   // held until this forward is enqueued
  if (int st = casync_gate_enter(H->device, H, &H->ev_fwd, s, &gate_lock)) return st;
  if (h16) return hb_walk16(H, wave, batch, G, out, HbWs16(ws_dev, batch, G), s, stage, n_layers);
  return hb_walk32(H, wave, batch, G, out, HbWs(static_cast<float*>(ws_dev), batch, G), s, stage, n_layers);
}
}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

int casync_hubert_packed_count(int layers) { return hb_layout(layers) ? hb_layout(layers)->packed.count() : 0; }
const char* casync_hubert_packed_name(int layers, int i) { return hb_layout(layers) ? hb_layout(layers)->packed.name(i) : nullptr; }
int64_t casync_hubert_packed_offset(int layers, int i) { return hb_layout(layers) ? hb_layout(layers)->packed.offset(i) : -1; }
int64_t casync_hubert_packed_size(int layers, int i) { return hb_layout(layers) ? hb_layout(layers)->packed.size(i) : -1; }
int64_t casync_hubert_packed_total(int layers) { return hb_layout(layers) ? hb_layout(layers)->packed.total : 0; }
int64_t casync_hubert_tokens(int64_t samples) { return samples > 0 ? HbGeom(samples).tokens() : 0; }
int64_t casync_hubert_workspace_bytes(int batch, int64_t samples) {
  if (batch <= 0 || samples <= 0) return 0;
  const HbGeom G(samples);
  return G.tokens() > 0 ? hb_workspace_bytes(DT_F32, batch, G) : 0;
}

int64_t casync_hubert_workspace_bytes_h(casync_hubert_handle h, int batch, int64_t samples) {
  if (!h || batch <= 0 || samples <= 0) return 0;
  const HbGeom G(samples);
  return G.tokens() > 0 ? hb_workspace_bytes(h->dtype, batch, G) : 0;
}

int casync_hubert_create(int device_id, int layers, casync_hubert_handle* out) {
  return casync_hubert_create_ex(device_id, layers, DT_F32, out);
}

int casync_hubert_create_ex(int device_id, int layers, int dtype, casync_hubert_handle* out) {
  CASYNC_REQUIRE(out, "hubert_create: null out");
  *out = nullptr;
  CASYNC_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "hubert_create: dtype %d (0 fp32, 1 bf16)", dtype);
  CASYNC_REQUIRE(layers >= 1 && layers <= kMaxLayers, "hubert_create: %d layers (1..%d)", layers, kMaxLayers);
  if (int st = casync_require_gfx950("hubert_create", device_id)) return st;
  casync_hubert* h = new casync_hubert();
  h->device = device_id;
  h->layers = layers;
  h->dtype = dtype;
  h->lay = hb_layout(layers);
  *out = h;
  return CASYNC_OK;
}

void casync_hubert_destroy(casync_hubert_handle h) {
  if (!h) return;
  DeviceGuard guard(h->device);
  casync_gate_forget(h->device, h, &h->ev_fwd);
  h->pw.release();
  delete h;
}

int casync_hubert_load_weights_host(casync_hubert_handle h, const float* packed, int64_t n_floats) {
  CASYNC_REQUIRE(h, "hubert_load_weights: null");
  return h->pw.load_host("hubert_load_weights", h->device, packed, n_floats, h->lay->packed.total, h->dtype == DT_BF16);
}

int casync_hubert_load_weights_device(casync_hubert_handle h, const float* packed_dev, int64_t n_floats) {
  CASYNC_REQUIRE(h, "hubert_load_weights_device: null");
  return h->pw.adopt_device("hubert_load_weights_device", h->device, packed_dev, n_floats, h->lay->packed.total, h->dtype == DT_BF16);
}

int casync_hubert_forward(casync_hubert_handle h, const float* wave_dev, int batch, int64_t samples, float* out_dev,
                          void* workspace_dev, int64_t workspace_bytes, casync_stream stream) {
  return hb_run(h, wave_dev, batch, samples, out_dev, workspace_dev, workspace_bytes, (hipStream_t)stream, 0, 0);
}

int casync_hubert_forward_tap(casync_hubert_handle h, const float* wave_dev, int batch, int64_t samples, int stage, int n_layers,
                              float* out_dev, void* workspace_dev, int64_t workspace_bytes, casync_stream stream) {
  CASYNC_REQUIRE(stage >= 1 && stage <= 3, "hubert_forward_tap: stage %d (1 conv stack, 2 layer-0 input, 3 after n layers)", stage);
  return hb_run(h, wave_dev, batch, samples, out_dev, workspace_dev, workspace_bytes, (hipStream_t)stream, stage, n_layers);
}

int casync_op_hubert_conv0(const float* wave, int batch, int samples, const float* w, const float* b, const float* g,
                           const float* be, float* out, casync_stream stream) {
  return launch_conv0(wave, batch, samples, w, b, g, be, out, (hipStream_t)stream);
}
int casync_op_hubert_layernorm(const float* in, int ldi, float* out, int ldo, int rows, int cols, const float* g, const float* b,
                               float eps, int gelu, casync_stream stream) {
  return launch_layernorm(in, ldi, out, ldo, rows, cols, g, b, eps, gelu != 0, (hipStream_t)stream);
}
int casync_op_hubert_posconv(const float* x, const float* w_packed, const float* bias, float* out, int batch, int T,
                             casync_stream stream) {
  return launch_posconv(x, w_packed, bias, out, batch, T, (hipStream_t)stream);
}
int casync_op_hubert_attention(const float* qkv, float* out, int batch, int T, casync_stream stream) {
  return launch_attention(qkv, out, batch, T, (hipStream_t)stream);
}
int casync_op_rows_gemm(const float* a, int lda, const float* w, const float* bias, float* c, int ldc, int m, int n, int k, int act,
                        const float* post_res, int ld_post, casync_stream stream) {
  GemmEpilogue e;
  e.bias = bias;
  e.act = act;
  e.post_res = post_res;
  e.ld_post = ld_post;
  return launch_rows_gemm(a, lda, w, c, ldc, m, n, k, e, (hipStream_t)stream);
}

}  // extern "C"
