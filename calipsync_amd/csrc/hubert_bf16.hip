// The bf16 precision of the HuBERT feature extractor (hubert.hip, casync_hubert_create_ex with dtype 1): the kernels that
// differ from the fp32 engine's.  GEMM operands and the activations between them are bf16, every sum is fp32, and the
// residual stream h stays fp32 for all layers:
//   conv0 + LayerNorm + GELU        hb16_conv0_kernel            fp32 arithmetic as hb_conv0_kernel, bf16 store
//   LayerNorm over 512 columns      hb16_layernorm512_kernel     bf16 in; bf16 out with GELU (conv stack) or fp32 out (feature projection)
//   LayerNorm over 1024 columns     hb16_layernorm1024_kernel    fp32 h (+ the bf16 delta of the GEMM in front of it, h updated in
//                                                                place) -> bf16 (LN1 / LN2) or fp32 (final): the residual add lives here,
//                                                                so no GEMM writes fp32
//   GELU of the FF1 output          hb16_gelu_kernel             in place, exact (erf) GELU in fp32 on bf16 storage
//   bf16 -> fp32                    hb16_widen_kernel            the conv-stack debug tap
//   self-attention                  hb16_attention_kernel        flash-style on v_mfma_f32_32x32x16_bf16
// The GEMMs are the U-Net's bf16 ring kernels (gemm.hip, launch_rows_gemm_bf16); feature projection and positional conv
// stay on the fp32 kernels of hubert.hip.
#include <math.h>

#include "common.h"

namespace {

constexpr int kHid = 1024, kConvC = 512, kHeads = 16, kHeadD = 64;

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- conv0 (1 -> 512, k=10, s=5) + LayerNorm(512) + GELU, bf16 out ------------------------------------------------------
// hb_conv0_kernel with a bf16 store: one wave per output row, lane owns channels 4*lane..+3 and 256+4*lane..+3.
__global__ __launch_bounds__(256) void hb16_conv0_kernel(const float* __restrict__ wave, int S, int T0, int rows,
                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ g, const float* __restrict__ be,
                                                         bf16_t* __restrict__ out, float eps) {
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
    const float inv = 1.f / sqrtf(wave_sum(q) * (1.f / kConvC) + eps);
    f32x4 o[2];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j >> 2][j & 3] = gelu_erf(fmaf(v[j] * inv, gr[j], er[j]));
    bf16_t* dst = out + (size_t)r * kConvC + 4 * lane;
    st4(dst, o[0]);
    st4(dst + 256, o[1]);
  }
}

// ---- LayerNorm over 512 bf16 columns, one row per wave, lane owns columns 8*lane..+7 (one 16-B load) -----------------------
// OUT_F32: fp32 rows out (feature projection), else bf16 (in == out allowed: a lane reads its elements before it writes them).
template <bool OUT_F32, bool GELU>
__global__ __launch_bounds__(256) void hb16_layernorm512_kernel(const bf16_t* in, int ldi, void* out, int ldo, int rows,
                                                                const float* __restrict__ g, const float* __restrict__ be, float eps) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  V16<bf16_t> x = ld16(in + (size_t)row * ldi + 8 * lane);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    s += x.v[e];
    asm("" : "+v"(s));   // a scalar chain, as in hb_layernorm_kernel: no packed add taking a register pair's high half
  }
  const float mean = wave_sum(s) * (1.f / kConvC);
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float d = x.v[e] - mean;
    x.v[e] = d, q += d * d;
  }
  const float inv = 1.f / sqrtf(wave_sum(q) * (1.f / kConvC) + eps);
  float y[8];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const f32x4 gg = *reinterpret_cast<const f32x4*>(g + 8 * lane + 4 * j);
    const f32x4 bb = *reinterpret_cast<const f32x4*>(be + 8 * lane + 4 * j);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = x.v[4 * j + e] * inv;
      asm("" : "+v"(t));   // element by element (see hb_layernorm_kernel)
      t = fmaf(t, gg[e], bb[e]);
      y[4 * j + e] = GELU ? gelu_erf(t) : t;
    }
  }
  if constexpr (OUT_F32) {
    float* d = static_cast<float*>(out) + (size_t)row * ldo + 8 * lane;
    *reinterpret_cast<f32x4*>(d) = f32x4{y[0], y[1], y[2], y[3]};
    *reinterpret_cast<f32x4*>(d + 4) = f32x4{y[4], y[5], y[6], y[7]};
  } else {
    V16<bf16_t> o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.v[e] = y[e];
    st16(static_cast<bf16_t*>(out) + (size_t)row * ldo + 8 * lane, o);
  }
}

// ---- LayerNorm over the 1024 fp32 columns of the residual stream, with the pending residual add ---------------------------
// v = h[row] (+ delta[row], the bf16 result of the out-proj / FF2 GEMM in front; h[row] = v when store_h), then
// out[row] = LayerNorm(v) as bf16 (LN1 / LN2) or fp32 (the final LayerNorm).  One row per wave, lane owns columns
// 4*lane + 256*j .. +3, two passes in registers.
template <bool OUT_F32>
__global__ __launch_bounds__(256) void hb16_layernorm1024_kernel(float* h, int ldh, const bf16_t* __restrict__ delta, int ldd,
                                                                 int store_h, void* out, int ldo, int rows,
                                                                 const float* __restrict__ g, const float* __restrict__ be, float eps) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float* p = h + (size_t)row * ldh + 4 * lane;
  f32x4 v[4];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = *reinterpret_cast<const f32x4*>(p + 256 * j);
    if (delta) {
      const f32x4 d = ld4(delta + (size_t)row * ldd + 4 * lane + 256 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = v[j][e] + d[e];
        asm("" : "+v"(t));
        v[j][e] = t;
      }
      if (store_h) *reinterpret_cast<f32x4*>(p + 256 * j) = v[j];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s += v[j][e];
      asm("" : "+v"(s));
    }
  }
  const float mean = wave_sum(s) * (1.f / kHid);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = v[j][e] - mean;
      v[j][e] = d, q += d * d;
    }
  const float inv = 1.f / sqrtf(wave_sum(q) * (1.f / kHid) + eps);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x4 gg = *reinterpret_cast<const f32x4*>(g + 256 * j + 4 * lane);
    const f32x4 bb = *reinterpret_cast<const f32x4*>(be + 256 * j + 4 * lane);
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = v[j][e] * inv;
      asm("" : "+v"(t));
      y[e] = fmaf(t, gg[e], bb[e]);
    }
    if constexpr (OUT_F32) *reinterpret_cast<f32x4*>(static_cast<float*>(out) + (size_t)row * ldo + 4 * lane + 256 * j) = y;
    else st4(static_cast<bf16_t*>(out) + (size_t)row * ldo + 4 * lane + 256 * j, y);
  }
}

// ---- exact GELU in place over n8 chunks of 8 bf16 (16-B accesses) ------------------------------------------------------
__global__ __launch_bounds__(256) void hb16_gelu_kernel(bf16_t* x, long long n8) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
    V16<bf16_t> v = ld16(x + 8 * i);
#pragma unroll
    for (int e = 0; e < 8; ++e) v.v[e] = gelu_erf(v.v[e]);
    st16(x + 8 * i, v);
  }
}

// ---- bf16 -> fp32 over n8 chunks of 8 elements ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hb16_widen_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, long long n8) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
    const V16<bf16_t> v = ld16(in + 8 * i);
    *reinterpret_cast<f32x4*>(out + 8 * i) = f32x4{v.v[0], v.v[1], v.v[2], v.v[3]};
    *reinterpret_cast<f32x4*>(out + 8 * i + 4) = f32x4{v.v[4], v.v[5], v.v[6], v.v[7]};
  }
}

// ---- self-attention, 16 heads of 64, any T >= 1, bf16 ---------------------------------------------------------------------
// qkv: [B*T][3072] bf16 = (q pre-scaled by 1/8 | k | v), out: [B*T][1024] bf16.  A workgroup is four waves of 32 queries of
// one head; the keys come in tiles of 64, K and V staged in LDS once for the four waves (global -> registers while the
// previous tile computes, registers -> LDS behind the barrier).  Per tile and wave:
//   S^T = K Q^T   (hb_attention_kernel's orientation: keys on the accumulator rows, one query per lane column), two 32-key
//                 tiles x four k-steps of v_mfma_f32_32x32x16_bf16 with Q held in registers.  The softmax statistics of a
//                 query live in the lane pair (l, l ^ 32): fp32 max and sum, online rescale of O.
//   O^T += V^T P^T: the accumulator tile, rounded to bf16, is the B operand (it sums over the tile's row index = the key;
//                 element j of lane half h is key 16 s + 8 (j >> 2) + 4 h + (j & 3) of a k-step); V^T in that same key
//                 order comes from the row-major V image by ds_read_b64_tr_b16, two reads of four consecutive keys each
//                 (attention_bf16.hip).
// LDS images, 128-B rows of eight 16-B chunks:
//   K: chunk c of row r at 128 r + 16 (c ^ ((r >> 1) & 7)) -- the ring GEMM's swizzle, conflict free for the 32-row reads;
//   V: chunk c of row r at 128 r + 16 (c ^ (((r >> 1) & 1) << 2)) -- the four rows x 64 B that a 32-lane half takes in one
//      transposed read then fall into the four different quarters of the 256-B bank row.
constexpr int kAtWaves = 4, kAtKeys = 64;

__device__ __forceinline__ f32x16 mfma32b(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

__global__ __launch_bounds__(64 * kAtWaves) void hb16_attention_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int T) {
  __shared__ __attribute__((aligned(16))) char Ks[kAtKeys * 128];
  __shared__ __attribute__((aligned(16))) char Vs[kAtKeys * 128];
  const int head = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
  const int qi = (blockIdx.x * kAtWaves + wave) * 32 + r32;
  const bf16_t* base = qkv + (size_t)b * T * (3 * kHid) + head * kHeadD;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  bf16x8 fq[4];   // Q[qi][16 s + 8 h .. +7]
#pragma unroll
  for (int s = 0; s < 4; ++s)
    fq[s] = __builtin_bit_cast(bf16x8, qi < T ? *reinterpret_cast<const f32x4*>(base + (size_t)qi * (3 * kHid) + 16 * s + 8 * h) : zero4);

  // staging: 512 chunks of 16 B per tile and operand, two of each per thread; keys past T are zeros (V must stay finite)
  f32x4 kreg[2], vreg[2];
  auto fetch = [&](int j0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = tid + 256 * u, j = j0 + (idx >> 3);
      const bf16_t* p = base + (size_t)j * (3 * kHid) + 8 * (idx & 7);
      kreg[u] = j < T ? *reinterpret_cast<const f32x4*>(p + kHid) : zero4;
      vreg[u] = j < T ? *reinterpret_cast<const f32x4*>(p + 2 * kHid) : zero4;
    }
  };
  auto stash = [&] {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = tid + 256 * u, r = idx >> 3, c = idx & 7;
      *reinterpret_cast<f32x4*>(Ks + 128 * r + 16 * (c ^ ((r >> 1) & 7))) = kreg[u];
      *reinterpret_cast<f32x4*>(Vs + 128 * r + 16 * (c ^ (((r >> 1) & 1) << 2))) = vreg[u];
    }
  };
  // transposed-read addresses: 16-lane group g = lane >> 4 is lane half h = g >> 1 and channels 16 (g & 1) .. +15 of a
  // 32-channel tile ct; lane 4 qq + p of the group supplies row r0 + qq, chunk 4 ct + 2 (g & 1) + (p >> 1), byte 8 (p & 1),
  // where r0 = 32 t + 16 s + 8 jj + 4 h is a multiple of four: the row's swizzle bit is qq >> 1
  int tr_base[2][2];
  {
    const int g = lane >> 4, i = lane & 15, qq = i >> 2, p = i & 3;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
        tr_base[jj][ct] = 128 * (8 * jj + 4 * h + qq) + 16 * ((4 * ct + 2 * (g & 1) + (p >> 1)) ^ ((qq >> 1) << 2)) + 8 * (p & 1);
  }

  f32x16 o[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[ct][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  fetch(0);
  for (int j0 = 0; j0 < T; j0 += kAtKeys) {
    __syncthreads();   // every wave is done with the previous tile
    stash();
    __syncthreads();
    if (j0 + kAtKeys < T) fetch(j0 + kAtKeys);
    f32x16 st[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st[t][r] = 0.f;
      const int krow = 32 * t + r32;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bf16x8 fk = *reinterpret_cast<const bf16x8*>(Ks + 128 * krow + 16 * ((2 * s + h) ^ ((krow >> 1) & 7)));
        st[t] = mfma32b(fk, fq[s], st[t]);
      }
    }
    // st[t][r] = S^T[key j0 + 32 t + (r & 3) + 8 (r >> 2) + 4 h][query qi]
    if (j0 + kAtKeys > T) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (j0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h >= T) st[t][r] = -INFINITY;
    }
    float mx = st[0][0];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[t][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));   // finite: key j0 exists
    const float mn = fmaxf(m, mx), alpha = __expf(m - mn);
    float ps = 0.f;
    bf16x8 pf[2][2];   // P^T as the B operand: k-step s of tile t = registers 8 s .. 8 s + 7
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __expf(st[t][r] - mn);   // exp(-inf) = 0 for the keys past T
        ps += e;
        pf[t][r >> 3][r & 7] = (bf16_t)e;
      }
    l = l * alpha + ps;
    m = mn;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[ct][r] *= alpha;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (s16x4 __attribute__((address_space(3)))*)(Vs + tr_base[0][ct] + 128 * (32 * t + 16 * s)));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (s16x4 __attribute__((address_space(3)))*)(Vs + tr_base[1][ct] + 128 * (32 * t + 16 * s)));
          const s16x8 av = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          o[ct] = mfma32b(__builtin_bit_cast(bf16x8, av), pf[t][s], o[ct]);
        }
  }
  const float inv = 1.f / (l + __shfl_xor(l, 32));
  if (qi < T) {
    // o[ct][4 g4 + e] = O[qi][32 ct + 8 g4 + 4 h + e]: runs of four channels, 8-byte stores
    bf16_t* dst = out + ((size_t)b * T + qi) * kHid + head * kHeadD + 4 * h;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        st4(dst + 32 * ct + 8 * g4, f32x4{o[ct][4 * g4] * inv, o[ct][4 * g4 + 1] * inv, o[ct][4 * g4 + 2] * inv, o[ct][4 * g4 + 3] * inv});
  }
}

unsigned grid_for(long long items, long long per_block, unsigned cap) {
  const long long want = (items + per_block - 1) / per_block;
  return (unsigned)(want < 1 ? 1 : want < cap ? want : cap);
}

}  // namespace

// ---- launchers -------------------------------------------------------------------------------------------------------
int launch_hb16_conv0(const float* wave, int batch, int S, const float* w, const float* b, const float* g, const float* be,
                      void* out, hipStream_t s) {
  CASYNC_REQUIRE(wave && w && b && g && be && out && batch > 0 && S >= 10, "hubert16 conv0: bad args (S=%d)", S);
  CASYNC_REQUIRE((uintptr_t)out % 8 == 0, "hubert16 conv0: alignment");
  const int T0 = (S - 10) / 5 + 1;
  const long long rows = (long long)batch * T0;
  CASYNC_REQUIRE(rows < (1ll << 31), "hubert16 conv0: too many rows");
  return casync_launch(hb16_conv0_kernel, dim3(grid_for(rows, 4, 4096)), dim3(256), 0, s, wave, S, T0, (int)rows, w, b, g, be,
                       static_cast<bf16_t*>(out), 1e-5f);
}

int launch_hb16_layernorm512(const void* in, int ldi, void* out, int ldo, int rows, const float* g, const float* b, float eps,
                             bool out_f32, bool gelu, hipStream_t s) {
  CASYNC_REQUIRE(in && out && g && b && rows > 0, "hubert16 layernorm512: bad args");
  CASYNC_REQUIRE(out_f32 != gelu, "hubert16 layernorm512: bf16 out with GELU or fp32 out without (out_f32=%d gelu=%d)", (int)out_f32, (int)gelu);
  CASYNC_REQUIRE(ldi >= kConvC && ldo >= kConvC && ldi % 8 == 0 && ldo % (out_f32 ? 4 : 8) == 0 && (uintptr_t)in % 16 == 0 &&
                     (uintptr_t)out % 16 == 0 && (uintptr_t)g % 16 == 0 && (uintptr_t)b % 16 == 0,
                 "hubert16 layernorm512: leading dimensions / alignment");
  const dim3 grid((rows + 3) / 4);
  const bf16_t* i16 = static_cast<const bf16_t*>(in);
  return out_f32 ? casync_launch(hb16_layernorm512_kernel<true, false>, grid, dim3(256), 0, s, i16, ldi, out, ldo, rows, g, b, eps)
                 : casync_launch(hb16_layernorm512_kernel<false, true>, grid, dim3(256), 0, s, i16, ldi, out, ldo, rows, g, b, eps);
}

int launch_hb16_layernorm1024(float* h, int ldh, const void* delta, int ldd, bool store_h, void* out, int ldo, int rows,
                              const float* g, const float* b, float eps, bool out_f32, hipStream_t s) {
  CASYNC_REQUIRE(h && out && g && b && rows > 0, "hubert16 layernorm1024: bad args");
  CASYNC_REQUIRE(ldh >= kHid && ldo >= kHid && ldh % 4 == 0 && ldo % 4 == 0 && (uintptr_t)h % 16 == 0 &&
                     (uintptr_t)out % (out_f32 ? 16 : 8) == 0 && (uintptr_t)g % 16 == 0 && (uintptr_t)b % 16 == 0,
                 "hubert16 layernorm1024: leading dimensions / alignment");
  CASYNC_REQUIRE(!delta || (ldd >= kHid && ldd % 4 == 0 && (uintptr_t)delta % 8 == 0), "hubert16 layernorm1024: bad delta");
  CASYNC_REQUIRE(!out_f32 || static_cast<void*>(h) != out, "hubert16 layernorm1024: fp32 out in place is not supported");
  const dim3 grid((rows + 3) / 4);
  const bf16_t* d16 = static_cast<const bf16_t*>(delta);
  const int st = store_h ? 1 : 0;
  return out_f32 ? casync_launch(hb16_layernorm1024_kernel<true>, grid, dim3(256), 0, s, h, ldh, d16, ldd, st, out, ldo, rows, g, b, eps)
                 : casync_launch(hb16_layernorm1024_kernel<false>, grid, dim3(256), 0, s, h, ldh, d16, ldd, st, out, ldo, rows, g, b, eps);
}

int launch_hb16_gelu(void* x, long long n, hipStream_t s) {
  CASYNC_REQUIRE(x && n > 0 && n % 8 == 0 && (uintptr_t)x % 16 == 0, "hubert16 gelu: %lld elements (a positive multiple of 8, 16-B aligned)", n);
  return casync_launch(hb16_gelu_kernel, dim3(grid_for(n / 8, 256, 8192)), dim3(256), 0, s, static_cast<bf16_t*>(x), n / 8);
}

int launch_hb16_widen(const void* in, float* out, long long n, hipStream_t s) {
  CASYNC_REQUIRE(in && out && n > 0 && n % 8 == 0 && (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0,
                 "hubert16 widen: %lld elements (a positive multiple of 8, 16-B aligned)", n);
  return casync_launch(hb16_widen_kernel, dim3(grid_for(n / 8, 256, 8192)), dim3(256), 0, s, static_cast<const bf16_t*>(in), out, n / 8);
}

int launch_hb16_attention(const void* qkv, void* out, int batch, int T, hipStream_t s) {
  CASYNC_REQUIRE(qkv && out && batch > 0 && T > 0 && batch <= 65535, "hubert16 attention: bad args");
  CASYNC_REQUIRE((uintptr_t)qkv % 16 == 0 && (uintptr_t)out % 8 == 0, "hubert16 attention: alignment");
  const int per_wg = 32 * kAtWaves;
  return casync_launch(hb16_attention_kernel, dim3((T + per_wg - 1) / per_wg, kHeads, batch), dim3(64 * kAtWaves), 0, s,
                       static_cast<const bf16_t*>(qkv), static_cast<bf16_t*>(out), T);
}

// ---- C ABI: one op entry per kernel (tests/kernel_ledger_hb16.py) ----------------------------------------------------------
extern "C" {

int casync_op_hubert16_conv0(const float* wave, int batch, int samples, const float* w, const float* b, const float* g,
                             const float* be, void* out, casync_stream stream) {
  return launch_hb16_conv0(wave, batch, samples, w, b, g, be, out, (hipStream_t)stream);
}
int casync_op_hubert16_layernorm512(const void* in, int ldi, void* out, int ldo, int rows, const float* g, const float* b,
                                    float eps, int out_f32, int gelu, casync_stream stream) {
  return launch_hb16_layernorm512(in, ldi, out, ldo, rows, g, b, eps, out_f32 != 0, gelu != 0, (hipStream_t)stream);
}
int casync_op_hubert16_layernorm1024(float* h, int ldh, const void* delta, int ldd, int store_h, void* out, int ldo, int rows,
                                     const float* g, const float* b, float eps, int out_f32, casync_stream stream) {
  return launch_hb16_layernorm1024(h, ldh, delta, ldd, store_h != 0, out, ldo, rows, g, b, eps, out_f32 != 0, (hipStream_t)stream);
}
int casync_op_hubert16_gelu(void* x, int64_t n, casync_stream stream) { return launch_hb16_gelu(x, n, (hipStream_t)stream); }
int casync_op_hubert16_widen(const void* in, float* out, int64_t n, casync_stream stream) {
  return launch_hb16_widen(in, out, n, (hipStream_t)stream);
}
int casync_op_hubert16_attention(const void* qkv, void* out, int batch, int T, casync_stream stream) {
  return launch_hb16_attention(qkv, out, batch, T, (hipStream_t)stream);
}
int casync_op_rows_gemm_bf16(const void* a, int lda, const void* w, const float* bias, void* c, int ldc, int m, int n, int k,
                             casync_stream stream) {
  return launch_rows_gemm_bf16(a, lda, w, bias, c, ldc, m, n, k, (hipStream_t)stream);
}

}  // extern "C"
