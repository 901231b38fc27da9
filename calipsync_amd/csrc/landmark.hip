// PFLD_GhostOne(width_factor=0.5, input_size=192, landmark_number=110) of the reference's LipDetector
// (utils/lip_detector/tools/pfld_mobileone.py:12-133, base_module.py:87-151,193-420) with every MobileOneBlock folded to
// one conv + bias on the host (calipsync_amd/landmarks.py fold): fp32, NHWC, gfx950.
//
//   lmk_stem_kernel<U8>    conv1 (dense 3x3 s2 + ReLU) recomputed on a one-pixel halo into LDS, conv2 (depthwise 3x3 + ReLU)
//                          from LDS; NHWC out + per-tile channel sums (x1's mean).  Input: float NCHW or uint8 BGR HWC.
//   lmk_ghost_kernel<RELU> GhostOneModule: the pointwise conv of a 6x6 tile and its halo (8x8 = 64 pixels = four 16-row
//                          blocks of v_mfma_f32_16x16x4_f32) into LDS, the depthwise 3x3 from LDS, both halves written as
//                          [.., 2h]; optional per-tile channel sums.
//   lmk_dw_s2_kernel       the linear stride-2 depthwise 3x3 of the three s = 2 bottlenecks.
//   lmk_head_kernel        one workgroup per frame: the four means from the per-tile sums (fixed order), conv7, conv8,
//                          conv_out.
// Every kernel works on one frame per workgroup (or per element) with a plan that does not depend on the batch: frame i of
// a batch has the bits of the same frame forwarded alone, and there is no atomic anywhere.
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "handle.h"

namespace {

__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : 0.f; }

// ------------------------------------------------------------------------------------------------ stem
constexpr int ST = 8;                  // output tile side (conv2 pixels)
constexpr int SH = ST + 2;             // conv1 halo side
constexpr int SI = 2 * SH + 1;         // input patch side (21)
constexpr int SC = 32;                 // channels of conv1 / conv2

template <bool U8>
__global__ __launch_bounds__(256) void lmk_stem_kernel(const void* __restrict__ xin, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, const float* __restrict__ w2,
                                                       const float* __restrict__ b2, float* __restrict__ out,
                                                       float* __restrict__ sums, float* __restrict__ tap1, int Hin, int Win,
                                                       int Ho, int Wo, int tiles_x) {
  __shared__ float s_in[SI * SI * 3];
  __shared__ float s_c1[SH * SH][SC];
  __shared__ float s_red[8][SC];
  const int tid = threadIdx.x, b = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * ST, tx0 = (tile % tiles_x) * ST;
  const int iy0 = 2 * ty0 - 3, ix0 = 2 * tx0 - 3;
  for (int idx = tid; idx < SI * SI * 3; idx += 256) {
    int ci, iy, ix;
    if (U8) {
      ci = idx % 3, ix = (idx / 3) % SI, iy = idx / (3 * SI);
    } else {
      ix = idx % SI, iy = (idx / SI) % SI, ci = idx / (SI * SI);
    }
    const int gy = iy0 + iy, gx = ix0 + ix;
    float v = 0.f;
    if (gy >= 0 && gy < Hin && gx >= 0 && gx < Win) {
      if (U8)
        v = (float)static_cast<const unsigned char*>(xin)[(((size_t)b * Hin + gy) * Win + gx) * 3 + ci] / 255.0f;
      else
        v = static_cast<const float*>(xin)[(((size_t)b * 3 + ci) * Hin + gy) * Win + gx];
    }
    s_in[(iy * SI + ix) * 3 + ci] = v;
  }
  const int c = tid % SC, pg = tid / SC;
  float w[27];
#pragma unroll
  for (int t = 0; t < 27; ++t) w[t] = w1[t * SC + c];
  const float bias1 = b1[c];
  __syncthreads();
  for (int p = pg; p < SH * SH; p += 8) {
    const int hy = p / SH, hx = p % SH;
    const int y1 = ty0 - 1 + hy, x1 = tx0 - 1 + hx;
    float v = 0.f;
    if (y1 >= 0 && y1 < Ho && x1 >= 0 && x1 < Wo) {
      v = bias1;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int ci = 0; ci < 3; ++ci) v = fmaf(w[(ky * 3 + kx) * 3 + ci], s_in[((2 * hy + ky) * SI + 2 * hx + kx) * 3 + ci], v);
      v = relu(v);
      if (tap1 && hy >= 1 && hy <= ST && hx >= 1 && hx <= ST) tap1[(((size_t)b * Ho + y1) * Wo + x1) * SC + c] = v;
    }
    s_c1[p][c] = v;
  }
  float wd[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) wd[t] = w2[t * SC + c];
  const float bias2 = b2[c];
  __syncthreads();
  float part[ST];   // summed as a tree (here and across the pixel groups): the depth of a pairwise sum over the tile's 64 pixels
#pragma unroll
  for (int i = 0; i < ST; ++i) {
    const int p = pg + 8 * i, oy = p / ST, ox = p % ST;
    float v = bias2;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) v = fmaf(wd[ky * 3 + kx], s_c1[(oy + ky) * SH + ox + kx][c], v);
    v = relu(v);
    const int gy = ty0 + oy, gx = tx0 + ox;
    const bool inside = gy < Ho && gx < Wo;
    if (inside) out[(((size_t)b * Ho + gy) * Wo + gx) * SC + c] = v;
    part[i] = inside ? v : 0.f;
  }
  s_red[pg][c] = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
  __syncthreads();
  if (tid < SC) {
    const float s = ((s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid])) +
                    ((s_red[4][tid] + s_red[5][tid]) + (s_red[6][tid] + s_red[7][tid]));
    sums[((size_t)b * gridDim.x + tile) * SC + tid] = s;
  }
}

// ------------------------------------------------------------------------------------------------ ghost module
constexpr int GT = 6;              // output tile side
constexpr int GH = GT + 2;         // halo side: 64 pixels
constexpr int G_MAXN = 128;        // widest padded half (126 -> 128)
constexpr int G_LD = G_MAXN + 4;   // LDS row stride (floats)

// in [B,H,W,ld_in] (cin % 4 == 0, ld_in % 4 == 0), wp [ceil16(cin)][npad] zero-padded, bp [npad], wd [9][npad], bd [npad],
// out [B,H,W,ld_out]: channels [0,half) = act(pw), [half,2 half) = act(dw(act(pw))).  sums (optional, half <= 64):
// [B][tiles][2 half] channel sums over the tile's pixels.
template <bool RELU>
__global__ __launch_bounds__(256) void lmk_ghost_kernel(const float* __restrict__ in, int ld_in, const float* __restrict__ wp,
                                                        const float* __restrict__ bp, const float* __restrict__ wd,
                                                        const float* __restrict__ bd, float* __restrict__ out, int ld_out,
                                                        float* __restrict__ sums, int H, int W, int cin, int half, int npad,
                                                        int tiles_x) {
  __shared__ float s1[GH * GH][G_LD];
  __shared__ float s2[GT * GT][G_LD];
  const int tid = threadIdx.x, b = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * GT, tx0 = (tile % tiles_x) * GT;
  const int lane = tid & 63, mb = tid >> 6, g = lane >> 4, n = lane & 15;
  const int nblk = npad >> 4;
  {
    const int p = mb * 16 + n, gy = ty0 - 1 + p / GH, gx = tx0 - 1 + p % GH;
    const bool valid = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const float* src = in + (((size_t)b * H + (valid ? gy : 0)) * W + (valid ? gx : 0)) * ld_in;
    f32x4 acc[8];
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < cin; k0 += 16) {
      const int kk = k0 + 4 * g;
      f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
      if (valid && kk < cin) a = *reinterpret_cast<const f32x4*>(src + kk);
      const float* wrow = wp + (size_t)kk * npad + n;
#pragma unroll
      for (int nb = 0; nb < 8; ++nb) {
        if (nb < nblk) {
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], wrow[i * npad + nb * 16], acc[nb], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) {
      if (nb < nblk) {
        const int c = nb * 16 + n;
        const float bias = bp[c];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q = mb * 16 + 4 * g + r, qy = ty0 - 1 + q / GH, qx = tx0 - 1 + q % GH;
          float v = acc[nb][r] + bias;
          if (RELU) v = relu(v);
          s1[q][c] = (qy >= 0 && qy < H && qx >= 0 && qx < W) ? v : 0.f;
        }
      }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < GT * GT * half; idx += 256) {
    const int p = idx / half, c = idx - p * half, oy = p / GT, ox = p - oy * GT;
    const float x1 = s1[(oy + 1) * GH + ox + 1][c];
    float d = bd[c];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) d = fmaf(wd[(ky * 3 + kx) * npad + c], s1[(oy + ky) * GH + ox + kx][c], d);
    if (RELU) d = relu(d);
    const int gy = ty0 + oy, gx = tx0 + ox;
    const bool inside = gy < H && gx < W;
    if (inside) {
      float* o = out + (((size_t)b * H + gy) * W + gx) * ld_out;
      o[c] = x1;
      o[half + c] = d;
    }
    if (sums) {
      s2[p][c] = inside ? x1 : 0.f;
      s2[p][half + c] = inside ? d : 0.f;
    }
  }
  if (sums) {
    __syncthreads();
    if (tid < 2 * half) {
      float v[GT * GT];   // pairwise tree (fully unrolled: registers), fixed order
#pragma unroll
      for (int p = 0; p < GT * GT; ++p) v[p] = s2[p][tid];
#pragma unroll
      for (int w = 1; w < GT * GT; w *= 2)
#pragma unroll
        for (int p = 0; p + w < GT * GT; p += 2 * w) v[p] += v[p + w];
      sums[((size_t)b * gridDim.x + tile) * (2 * half) + tid] = v[0];
    }
  }
}

// ------------------------------------------------------------------------------------------------ stride-2 depthwise
// in [B,H,W,C] -> out [B,Ho,Wo,ld_out], Ho = (H-1)/2+1, pad 1, linear; w [9][C] tap-major
__global__ __launch_bounds__(256) void lmk_dw_s2_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ out, int ld_out,
                                                        int B, int H, int W, int C, int Ho, int Wo) {
  const long long total = (long long)B * Ho * Wo * C;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int c = (int)(idx % C);
    long long r = idx / C;
    const int ox = (int)(r % Wo);
    r /= Wo;
    const int oy = (int)(r % Ho), b = (int)(r / Ho);
    float v = bias[c];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = 2 * oy - 1 + ky;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = 2 * ox - 1 + kx;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = fmaf(w[(ky * 3 + kx) * C + c], in[(((size_t)b * H + iy) * W + ix) * C + c], v);
      }
    }
    out[(((size_t)b * Ho + oy) * Wo + ox) * ld_out + c] = v;
  }
}

// ------------------------------------------------------------------------------------------------ head
constexpr int HD = 12;                    // conv6 / conv7 resolution: conv8's kernel is the whole 12x12 frame
constexpr int HP = HD * HD;               // 144
constexpr int C6 = 8, C7 = 16, C8 = 64, NF = 256, NOUT = 220;
struct HeadSums {
  const float* p[4];   // [B][nt][c] per-tile channel sums of x1..x4
  int nt[4];           // tiles per frame
  int cnt[4];          // pixels per frame (the mean's divisor)
};

// x6 [B,12,12,8]; w7 [72][16] (ky,kx,ci major), w8 [(y,x,c)=2304][64], wo [256][220]; out [B, ld_out]; tap7 [B,144,16], tap8 [B,64]
__global__ __launch_bounds__(256) void lmk_head_kernel(HeadSums S, const float* __restrict__ x6, const float* __restrict__ w7,
                                                       const float* __restrict__ b7, const float* __restrict__ w8,
                                                       const float* __restrict__ wo, const float* __restrict__ bo,
                                                       float* __restrict__ out, int ld_out, float* __restrict__ tap7,
                                                       float* __restrict__ tap8) {
  __shared__ float s_x[(HD + 2) * (HD + 2) * C6];   // zero-padded conv6 frame
  __shared__ float s_a[HP * C7];
  __shared__ float s_part[4][C8];
  __shared__ float s_feat[NF];
  const int tid = threadIdx.x, b = blockIdx.x;
  // the four means: thread = channel, tiles in order
  {
    int base = 0;
    const int width[4] = {32, 40, 48, 72};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int cw = width[j];
      if (tid >= base && tid < base + cw) {
        const int c = tid - base;
        const float* p = S.p[j] + (size_t)b * S.nt[j] * cw + c;
        float s = 0.f;   // chunks of 16 tiles, then the chunks: shorter chains than one serial sum, fixed order
        for (int t0 = 0; t0 < S.nt[j]; t0 += 16) {
          float c16 = 0.f;
          for (int t = t0; t < S.nt[j] && t < t0 + 16; ++t) c16 += p[(size_t)t * cw];
          s += c16;
        }
        s_feat[tid] = s / (float)S.cnt[j];
      }
      base += cw;
    }
  }
  for (int idx = tid; idx < (HD + 2) * (HD + 2) * C6; idx += 256) {
    const int ci = idx % C6, px = (idx / C6) % (HD + 2), py = idx / (C6 * (HD + 2));
    const bool in = py >= 1 && py <= HD && px >= 1 && px <= HD;
    s_x[idx] = in ? x6[(((size_t)b * HD + py - 1) * HD + px - 1) * C6 + ci] : 0.f;
  }
  __syncthreads();
  {
    const int co = tid % C7, pg = tid / C7;   // 16 pixel groups x 9 pixels
    for (int p = pg; p < HP; p += 16) {
      const int oy = p / HD, ox = p % HD;
      float v = b7[co];
      for (int t = 0; t < 9; ++t) {
        const float* xs = &s_x[((oy + t / 3) * (HD + 2) + ox + t % 3) * C6];
#pragma unroll
        for (int ci = 0; ci < C6; ++ci) v = fmaf(w7[(t * C6 + ci) * C7 + co], xs[ci], v);
      }
      v = relu(v);
      s_a[p * C7 + co] = v;
      if (tap7) tap7[((size_t)b * HP + p) * C7 + co] = v;
    }
  }
  __syncthreads();
  {
    const int o = tid % C8, q = tid / C8;
    constexpr int KQ = HP * C7 / 4;   // 576
    const float* wq = w8 + (size_t)q * KQ * C8 + o;
    const float* aq = s_a + q * KQ;
    float acc[8];   // eight interleaved chains of 72 terms, then a tree: shorter chains, smaller rounding error
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = 0.f;
    for (int k = 0; k < KQ; k += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] = fmaf(aq[k + u], wq[(size_t)(k + u) * C8], acc[u]);
    }
    s_part[q][o] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  }
  __syncthreads();
  if (tid < C8) {
    const float v = relu(((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid]);
    s_feat[NF - C8 + tid] = v;
    if (tap8) tap8[(size_t)b * C8 + tid] = v;
  }
  __syncthreads();
  if (tid < NOUT) {
    float a0 = bo[tid], a1 = 0.f, a2 = 0.f, a3 = 0.f;   // four interleaved chains of 64 terms
    for (int k = 0; k < NF; k += 4) {
      a0 = fmaf(s_feat[k], wo[k * NOUT + tid], a0);
      a1 = fmaf(s_feat[k + 1], wo[(k + 1) * NOUT + tid], a1);
      a2 = fmaf(s_feat[k + 2], wo[(k + 2) * NOUT + tid], a2);
      a3 = fmaf(s_feat[k + 3], wo[(k + 3) * NOUT + tid], a3);
    }
    out[(size_t)b * ld_out + tid] = (a0 + a1) + (a2 + a3);
  }
}

// ------------------------------------------------------------------------------------------------ launchers
int ceil_to(int v, int m) { return (v + m - 1) / m * m; }

int launch_stem(const void* x, bool u8, const float* w1, const float* b1, const float* w2, const float* b2, float* out, float* sums,
                float* tap1, int batch, int hin, int win, hipStream_t s) {
  CASYNC_REQUIRE(x && w1 && b1 && w2 && b2 && out && sums, "pfld stem: null pointer");
  CASYNC_REQUIRE(batch > 0 && batch <= 65535 && hin >= 1 && win >= 1 && hin <= 4096 && win <= 4096, "pfld stem: B=%d %dx%d", batch, hin, win);
  const int ho = (hin - 1) / 2 + 1, wo = (win - 1) / 2 + 1;
  const int tx = (wo + ST - 1) / ST, ty = (ho + ST - 1) / ST;
  if (u8)
    return casync_launch(lmk_stem_kernel<true>, dim3(tx * ty, batch), dim3(256), 0, s, x, w1, b1, w2, b2, out, sums, tap1, hin, win, ho, wo, tx);
  return casync_launch(lmk_stem_kernel<false>, dim3(tx * ty, batch), dim3(256), 0, s, x, w1, b1, w2, b2, out, sums, tap1, hin, win, ho, wo, tx);
}
int stem_tiles(int hin, int win) { return (((hin - 1) / 2 + 1 + ST - 1) / ST) * (((win - 1) / 2 + 1 + ST - 1) / ST); }

int ghost_tiles(int h, int w) { return ((h + GT - 1) / GT) * ((w + GT - 1) / GT); }
int launch_ghost(const float* in, int ld_in, const float* wp, const float* bp, const float* wd, const float* bd, float* out,
                 int ld_out, float* sums, int batch, int h, int w, int cin, int half, bool act, hipStream_t s) {
  CASYNC_REQUIRE(in && wp && bp && wd && bd && out, "pfld ghost: null pointer");
  CASYNC_REQUIRE(batch > 0 && batch <= 65535 && h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "pfld ghost: B=%d %dx%d", batch, h, w);
  CASYNC_REQUIRE(cin >= 4 && cin % 4 == 0 && ld_in >= cin && ld_in % 4 == 0 && (uintptr_t)in % 16 == 0,
                 "pfld ghost: cin %d ld_in %d (multiples of 4, 16-B aligned rows)", cin, ld_in);
  CASYNC_REQUIRE(half >= 1 && half <= G_MAXN && ld_out >= 2 * half, "pfld ghost: half %d (1..%d), ld_out %d", half, G_MAXN, ld_out);
  CASYNC_REQUIRE(!sums || half <= 64, "pfld ghost: channel sums need half <= 64 (%d)", half);
  const int npad = ceil_to(half, 16), tx = (w + GT - 1) / GT, ty = (h + GT - 1) / GT;
  if (act)
    return casync_launch(lmk_ghost_kernel<true>, dim3(tx * ty, batch), dim3(256), 0, s, in, ld_in, wp, bp, wd, bd, out, ld_out, sums, h, w, cin, half, npad, tx);
  return casync_launch(lmk_ghost_kernel<false>, dim3(tx * ty, batch), dim3(256), 0, s, in, ld_in, wp, bp, wd, bd, out, ld_out, sums, h, w, cin, half, npad, tx);
}

int launch_dw_s2(const float* in, const float* w, const float* bias, float* out, int ld_out, int batch, int h, int wdt, int c,
                 hipStream_t s) {
  CASYNC_REQUIRE(in && w && bias && out, "pfld dw_s2: null pointer");
  CASYNC_REQUIRE(batch > 0 && h >= 1 && wdt >= 1 && c >= 1 && ld_out >= c, "pfld dw_s2: B=%d %dx%dx%d ld_out %d", batch, h, wdt, c, ld_out);
  const int ho = (h - 1) / 2 + 1, wo = (wdt - 1) / 2 + 1;
  const long long total = (long long)batch * ho * wo * c;
  CASYNC_REQUIRE((long long)batch * h * wdt * c < (1ll << 40), "pfld dw_s2: too large");
  const int grid = (int)((total + 255) / 256 > 65536 ? 65536 : (total + 255) / 256);
  return casync_launch(lmk_dw_s2_kernel, dim3(grid), dim3(256), 0, s, in, w, bias, out, ld_out, batch, h, wdt, c, ho, wo);
}

int launch_head(const HeadSums& S, const float* x6, const float* w7, const float* b7, const float* w8, const float* wo,
                const float* bo, float* out, int ld_out, float* tap7, float* tap8, int batch, hipStream_t s) {
  CASYNC_REQUIRE(x6 && w7 && b7 && w8 && wo && bo && out, "pfld head: null pointer");
  for (int j = 0; j < 4; ++j) CASYNC_REQUIRE(S.p[j] && S.nt[j] >= 1 && S.cnt[j] >= 1, "pfld head: sums %d", j);
  CASYNC_REQUIRE(batch > 0 && ld_out >= NOUT, "pfld head: B=%d ld_out %d", batch, ld_out);
  return casync_launch(lmk_head_kernel, dim3(batch), dim3(256), 0, s, S, x6, w7, b7, w8, wo, bo, out, ld_out, tap7, tap8);
}

// ------------------------------------------------------------------------------------------------ network, packed layout
struct Bneck {
  const char* name;
  int cin, hid, cout, stride;
};
const Bneck kBnecks[] = {
    {"conv3_1", 32, 48, 40, 2},  {"conv3_2", 40, 60, 40, 1},  {"conv3_3", 40, 60, 40, 1},  {"conv4_1", 40, 100, 48, 2},
    {"conv4_2", 48, 120, 48, 1}, {"conv4_3", 48, 120, 48, 1}, {"conv5_1", 48, 168, 72, 2}, {"conv5_2", 72, 252, 72, 1},
    {"conv5_3", 72, 252, 72, 1}, {"conv5_4", 72, 252, 72, 1}, {"conv6", 72, 108, 8, 1},
};
constexpr int kNB = 11;
constexpr int kIn = 192;
constexpr int kStages = 16;   // conv1, conv2, conv3_1..3, conv4_1..3, conv5_1..4, conv6, conv7, conv8, conv_out

PackedLayout make_lmk_layout() {
  PackedLayout L;
  L.add("conv1.w", 27 * SC), L.add("conv1.b", SC), L.add("conv2.w", 9 * SC), L.add("conv2.b", SC);
  for (const Bneck& k : kBnecks) {
    const std::string p = k.name;
    auto ghost = [&](const std::string& g, int cin, int cout) {
      const int np = ceil_to(cout / 2, 16);
      L.add(p + g + ".pw.w", (int64_t)ceil_to(cin, 16) * np), L.add(p + g + ".pw.b", np);
      L.add(p + g + ".dw.w", 9 * np), L.add(p + g + ".dw.b", np);
    };
    ghost(".g1", k.cin, k.hid);
    if (k.stride == 2) L.add(p + ".dw.w", 9 * k.hid), L.add(p + ".dw.b", k.hid);
    ghost(".g2", k.hid, k.cout);
  }
  L.add("conv7.w", 9 * C6 * C7), L.add("conv7.b", C7), L.add("conv8.w", (int64_t)HP * C7 * C8);
  L.add("conv_out.w", NF * NOUT), L.add("conv_out.b", NOUT);
  return L;
}
const PackedLayout& lmk_layout() {
  static const PackedLayout L = make_lmk_layout();
  return L;
}

constexpr int64_t kActFloats = 96 * 96 * 48;   // the largest activation of a frame: conv3_1's first ghost module
struct LmkWs {
  float *a, *b, *sum[4];
  int nt[4];
  int64_t floats;
  LmkWs(float* base, int batch) {
    const int hw[4] = {96, 48, 24, 12}, cw[4] = {32, 40, 48, 72};
    int64_t off = 0;
    auto take = [&](int64_t n) {
      float* p = base ? base + off : nullptr;
      off += round64(n);
      return p;
    };
    a = take(batch * kActFloats), b = take(batch * kActFloats);
    for (int j = 0; j < 4; ++j) {
      nt[j] = j == 0 ? stem_tiles(kIn, kIn) : ghost_tiles(hw[j], hw[j]);
      sum[j] = take((int64_t)batch * nt[j] * cw[j]);
    }
    floats = off;
  }
};

}  // namespace

// where every packed tensor of a forward lies: looked up by name once per handle (casync_pfld_create), so a forward
// builds no string and searches nothing
struct LmkOffsets {
  struct Ghost {
    int64_t pw_w, pw_b, dw_w, dw_b;
  };
  struct B {
    Ghost g1, g2;
    int64_t dw_w = -1, dw_b = -1;   // stride-2 bottlenecks only
  };
  int64_t conv1_w, conv1_b, conv2_w, conv2_b;
  B b[kNB];
  int64_t conv7_w, conv7_b, conv8_w, out_w, out_b;
  std::string missing;   // the first name the layout does not hold; empty when all were found

  LmkOffsets() {
    const PackedLayout& L = lmk_layout();
    auto get = [&](const std::string& n) {
      const int64_t o = L.off(n);
      if (o < 0 && missing.empty()) missing = n;
      return o;
    };
    conv1_w = get("conv1.w"), conv1_b = get("conv1.b"), conv2_w = get("conv2.w"), conv2_b = get("conv2.b");
    for (int i = 0; i < kNB; ++i) {
      const std::string p = kBnecks[i].name;
      auto ghost = [&](const std::string& g) { return Ghost{get(p + g + ".pw.w"), get(p + g + ".pw.b"), get(p + g + ".dw.w"), get(p + g + ".dw.b")}; };
      b[i].g1 = ghost(".g1"), b[i].g2 = ghost(".g2");
      if (kBnecks[i].stride == 2) b[i].dw_w = get(p + ".dw.w"), b[i].dw_b = get(p + ".dw.b");
    }
    conv7_w = get("conv7.w"), conv7_b = get("conv7.b"), conv8_w = get("conv8.w");
    out_w = get("conv_out.w"), out_b = get("conv_out.b");
  }
};

struct casync_pfld {
  int device = 0;
  PackedWeights pw;
  hipEvent_t ev_fwd = nullptr;   // forward gate slot
  LmkOffsets at;
};

namespace {
int64_t stage_floats(int stage) {   // per frame, NHWC
  static const int64_t n[kStages] = {96 * 96 * 32, 96 * 96 * 32, 48 * 48 * 40, 48 * 48 * 40, 48 * 48 * 40, 24 * 24 * 48,
                                     24 * 24 * 48, 24 * 24 * 48, 12 * 12 * 72, 12 * 12 * 72, 12 * 12 * 72, 12 * 12 * 72,
                                     12 * 12 * 8,  12 * 12 * 16, 64,           220};
  return stage >= 0 && stage < kStages ? n[stage] : -1;
}

// stage kStages - 1 = the landmarks [B,220]; a lower stage stops there and writes that NHWC intermediate to `out`
int lmk_run(casync_pfld* P, const void* x, bool u8, int batch, float* out, void* ws_dev, int64_t ws_bytes, hipStream_t s, int stage) {
  CASYNC_REQUIRE(P && x && out && ws_dev, "pfld forward: null pointer");
  CASYNC_REQUIRE(P->pw.w, "pfld forward: weights not loaded");
  CASYNC_REQUIRE(batch > 0 && batch <= 4096, "pfld forward: batch %d (1..4096)", batch);
  CASYNC_REQUIRE(stage >= 0 && stage < kStages, "pfld forward: stage %d (0..%d)", stage, kStages - 1);
  CASYNC_REQUIRE((uintptr_t)x % (u8 ? 1 : 4) == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)ws_dev % 256 == 0, "pfld forward: alignment");
  LmkWs ws(static_cast<float*>(ws_dev), batch);
  if (ws_bytes < ws.floats * 4) {
    casync_set_error("pfld forward: workspace %lld bytes, needs %lld", (long long)ws_bytes, (long long)ws.floats * 4);
    return CASYNC_ERR_STATE;
  }
  DeviceGuard guard(P->device);
  CASYNC_CHECK_HIP(guard.err);
  std::unique_lock<std::mutex> gate_lock;   // held until this forward is enqueued
  if (int st = casync_gate_enter(P->device, P, &P->ev_fwd, s, &gate_lock)) return st;
#define LM(call)                        \
  do {                                  \
    if (int st__ = (call)) return st__; \
  } while (0)
  auto copy_out = [&](const float* src, int64_t per_frame) -> int {
    CASYNC_CHECK_HIP(hipMemcpyAsync(out, src, (size_t)batch * per_frame * 4, hipMemcpyDeviceToDevice, s));
    return CASYNC_OK;
  };
  float *cur = ws.a, *nxt = ws.b;
  const LmkOffsets& at = P->at;
  const float* const w = P->pw.w;
  LM(launch_stem(x, u8, w + at.conv1_w, w + at.conv1_b, w + at.conv2_w, w + at.conv2_b, cur, ws.sum[0], stage == 0 ? out : nullptr,
                 batch, kIn, kIn, s));
  if (stage == 0) return CASYNC_OK;
  if (stage == 1) return copy_out(cur, stage_floats(1));
  int hw = 96, si = 1;   // si: the next per-tile sums to emit (x2, x3, x4)
  for (int i = 0; i < kNB; ++i) {
    const Bneck& k = kBnecks[i];
    const LmkOffsets::B& o = at.b[i];
    LM(launch_ghost(cur, k.cin, w + o.g1.pw_w, w + o.g1.pw_b, w + o.g1.dw_w, w + o.g1.dw_b, nxt, k.hid, nullptr, batch, hw, hw, k.cin,
                    k.hid / 2, true, s));
    std::swap(cur, nxt);
    if (k.stride == 2) {
      LM(launch_dw_s2(cur, w + o.dw_w, w + o.dw_b, nxt, k.hid, batch, hw, hw, k.hid, s));
      std::swap(cur, nxt);
      hw /= 2;
    }
    const bool last_of_stage = i == 2 || i == 5 || i == 9;
    LM(launch_ghost(cur, k.hid, w + o.g2.pw_w, w + o.g2.pw_b, w + o.g2.dw_w, w + o.g2.dw_b, nxt, k.cout,
                    last_of_stage ? ws.sum[si] : nullptr, batch, hw, hw, k.hid, k.cout / 2, false, s));
    std::swap(cur, nxt);
    if (last_of_stage) ++si;
    if (stage == 2 + i) return copy_out(cur, stage_floats(stage));
  }
  HeadSums S;
  const int cnt[4] = {96 * 96, 48 * 48, 24 * 24, 12 * 12};
  for (int j = 0; j < 4; ++j) S.p[j] = ws.sum[j], S.nt[j] = ws.nt[j], S.cnt[j] = cnt[j];
  float* head_out = stage == kStages - 1 ? out : nxt;   // a tap before the end discards the landmarks
  LM(launch_head(S, cur, w + at.conv7_w, w + at.conv7_b, w + at.conv8_w, w + at.out_w, w + at.out_b, head_out, NOUT,
                 stage == 13 ? out : nullptr, stage == 14 ? out : nullptr, batch, s));
#undef LM
  return CASYNC_OK;
}
}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

int casync_pfld_packed_count(void) { return lmk_layout().count(); }
const char* casync_pfld_packed_name(int i) { return lmk_layout().name(i); }
int64_t casync_pfld_packed_offset(int i) { return lmk_layout().offset(i); }
int64_t casync_pfld_packed_size(int i) { return lmk_layout().size(i); }
int64_t casync_pfld_packed_total(void) { return lmk_layout().total; }
int64_t casync_pfld_workspace_bytes(int batch) { return batch > 0 && batch <= 4096 ? LmkWs(nullptr, batch).floats * 4 : 0; }

int casync_pfld_create(int device_id, casync_pfld_handle* out) {
  CASYNC_REQUIRE(out, "pfld_create: null out");
  *out = nullptr;
  if (int st = casync_require_gfx950("pfld_create", device_id)) return st;
  casync_pfld* h = new casync_pfld();
  if (!h->at.missing.empty()) {
    casync_set_error("pfld_create: the packed layout has no tensor %s", h->at.missing.c_str());
    delete h;
    return CASYNC_ERR_STATE;
  }
  h->device = device_id;
  *out = h;
  return CASYNC_OK;
}

void casync_pfld_destroy(casync_pfld_handle h) {
  if (!h) return;
  DeviceGuard guard(h->device);
  casync_gate_forget(h->device, h, &h->ev_fwd);
  h->pw.release();
  delete h;
}

int casync_pfld_load_weights_host(casync_pfld_handle h, const float* packed, int64_t n_floats) {
  CASYNC_REQUIRE(h, "pfld_load_weights: null");
  return h->pw.load_host("pfld_load_weights", h->device, packed, n_floats, lmk_layout().total, false);
}

int casync_pfld_load_weights_device(casync_pfld_handle h, const float* packed_dev, int64_t n_floats) {
  CASYNC_REQUIRE(h, "pfld_load_weights_device: null");
  return h->pw.adopt_device("pfld_load_weights_device", h->device, packed_dev, n_floats, lmk_layout().total, false);
}

int casync_pfld_forward(casync_pfld_handle h, const float* x_dev, int batch, float* out_dev, void* workspace_dev,
                        int64_t workspace_bytes, casync_stream stream) {
  return lmk_run(h, x_dev, false, batch, out_dev, workspace_dev, workspace_bytes, (hipStream_t)stream, kStages - 1);
}
int casync_pfld_forward_u8(casync_pfld_handle h, const uint8_t* crops_dev, int batch, float* out_dev, void* workspace_dev,
                           int64_t workspace_bytes, casync_stream stream) {
  return lmk_run(h, crops_dev, true, batch, out_dev, workspace_dev, workspace_bytes, (hipStream_t)stream, kStages - 1);
}
int casync_pfld_forward_tap(casync_pfld_handle h, const void* in_dev, int input_u8, int batch, int stage, float* out_dev,
                            void* workspace_dev, int64_t workspace_bytes, casync_stream stream) {
  return lmk_run(h, in_dev, input_u8 != 0, batch, out_dev, workspace_dev, workspace_bytes, (hipStream_t)stream, stage);
}

int casync_op_pfld_stem(const void* x, int input_u8, const float* w1, const float* b1, const float* w2, const float* b2, float* out,
                        float* sums, float* conv1_out, int batch, int h, int w, casync_stream stream) {
  return launch_stem(x, input_u8 != 0, w1, b1, w2, b2, out, sums, conv1_out, batch, h, w, (hipStream_t)stream);
}
int casync_op_pfld_ghost(const float* in, int ld_in, const float* wp, const float* bp, const float* wd, const float* bd, float* out,
                         int ld_out, float* sums, int batch, int h, int w, int cin, int half, int act, casync_stream stream) {
  return launch_ghost(in, ld_in, wp, bp, wd, bd, out, ld_out, sums, batch, h, w, cin, half, act != 0, (hipStream_t)stream);
}
int casync_op_pfld_dw_s2(const float* in, const float* w, const float* bias, float* out, int ld_out, int batch, int h, int w_, int c,
                         casync_stream stream) {
  return launch_dw_s2(in, w, bias, out, ld_out, batch, h, w_, c, (hipStream_t)stream);
}
int casync_op_pfld_head(const float* const* sums, const int* tiles, const int* counts, const float* x6, const float* w7,
                        const float* b7, const float* w8, const float* wo, const float* bo, float* out, int ld_out, int batch,
                        casync_stream stream) {
  CASYNC_REQUIRE(sums && tiles && counts, "pfld head: null");
  HeadSums S;
  for (int j = 0; j < 4; ++j) S.p[j] = sums[j], S.nt[j] = tiles[j], S.cnt[j] = counts[j];
  return launch_head(S, x6, w7, b7, w8, wo, bo, out, ld_out, nullptr, nullptr, batch, (hipStream_t)stream);
}

}  // extern "C"
