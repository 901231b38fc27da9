// S3FD face detector of the reference's S3FDFaceDetector (utils/lip_detector/tools/detect_face.py; tools/s3fd/nets.py:28-171,
// box_utils.py:41-59,176-217): S3FDNet.forward up to the call of Detect.forward, plus PriorBox and decode.  fp32, NHWC, gfx950,
// frames of any equal size H x W.
//
//   det_stem_kernel<U8>     conv1_1 (3 -> 64, 3x3, pad 1) + ReLU from float NCHW (mean already subtracted) or uint8 HWC (the
//                           kernel subtracts (123, 117, 104)[c] itself: main.py:36-42, the two [2,1,0] swaps cancel).
//   det_maxpool_kernel      2x2 / 2 max pooling; the floor form drops an odd last row / column, the ceil form (pool 3) keeps a
//                           partial last window.
//   det_im2col_dil_kernel   the [B h w, 9 C] matrix of a dilated 3x3 conv (fc6: dilation 6, pad 6), zero where a tap is outside.
//   det_relu_kernel         ReLU in place behind the 1x1 convs and fc6 (the non-conv ring GEMM instances have no ReLU epilogue).
//   det_l2norm_kernel       x / (sqrt(sum_c x^2) + 1e-10) per pixel (nets.py:21-23); the weight is folded into the heads.
//   det_head_kernel         loc[i] and conf[i] of one source in one pass (3x3, pad 1, 4 + 4 outputs; conf[0]'s max-out of
//                           nets.py:144-145), one wave per four pixels of a row, the K = 9 C sum split over the lanes.
//   det_decode_kernel       PriorBox.forward + decode + the softmax's face probability -> det [B,P,5] = (score, x1, y1, x2, y2).
// conv1_2 .. conv5_3 and extras 1 and 3 run on the ring implicit-GEMM kernel (launch_conv3x3_gemm, ReLU epilogue), fc6 / fc7 and
// extras 0 and 2 on the data-parallel fp32 ring GEMM (launch_rows_gemm): no stream-K, no K split.  No kernel here sums across
// frames or uses an atomic: frame i of a batch has the bits of that frame forwarded alone.
//
// The network's order is written once, in det_pass<P>; a precision is a policy P (DetF32, DetBF16) that names its element type,
// its launchers and the weight image its matrices come from.  A handle made with precision 1 (casync_s3fd_create_ex) runs
// det_pass<DetBF16>: the same walk on bf16 activations, with the kernels of facedet_bf16.hip, the bf16 ring conv
// (launch_conv3x3_gemm, DT_BF16) and launch_rows_gemm_bf16 on a bf16 image of the packed buffer made at weight load; the stem,
// the heads and det_decode_kernel keep fp32 weights and outputs.  The fp32 handle launches what it launched before that
// precision existed.
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "handle.h"

namespace {

__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : 0.f; }

// ------------------------------------------------------------------------------------------------ stem
constexpr int SC = 64;   // channels of conv1_1

// w [(ky,kx,ci)=27][64], out [B,H,W,64]; 256 threads = 4 pixels x 64 channels
template <bool U8>
__global__ __launch_bounds__(256) void det_stem_kernel(const void* __restrict__ xin, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out, long long pixels,
                                                       int H, int W) {
  const int c = threadIdx.x % SC;
  const long long p = (long long)blockIdx.x * 4 + threadIdx.x / SC;
  if (p >= pixels) return;
  const int x = (int)(p % W);
  const long long r = p / W;
  const int y = (int)(r % H);
  const long long b = r / H;
  float v = bias[c];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = y + ky - 1;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = x + kx - 1;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
#pragma unroll
      for (int ci = 0; ci < 3; ++ci) {
        float in;
        if (U8) {
          const float mean = ci == 0 ? 123.f : ci == 1 ? 117.f : 104.f;
          in = (float)static_cast<const unsigned char*>(xin)[((b * H + iy) * W + ix) * 3 + ci] - mean;
        } else {
          in = static_cast<const float*>(xin)[((b * 3 + ci) * H + iy) * W + ix];
        }
        v = fmaf(w[((ky * 3 + kx) * 3 + ci) * SC + c], in, v);
      }
    }
  }
  out[p * SC + c] = relu(v);
}

// ------------------------------------------------------------------------------------------------ max pooling
// in [B,H,W,C] -> out [B,Ho,Wo,C], window 2x2 stride 2 clipped to the image (only the ceil form has a clipped window)
__global__ __launch_bounds__(256) void det_maxpool_kernel(const float* __restrict__ in, float* __restrict__ out, long long total4,
                                                          int H, int W, int C4, int Ho, int Wo) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total4) return;
  const int c4 = (int)(idx % C4);
  long long r = idx / C4;
  const int ox = (int)(r % Wo);
  r /= Wo;
  const int oy = (int)(r % Ho);
  const long long b = r / Ho;
  const int iy = 2 * oy, ix = 2 * ox;
  const float* src = in + (((b * H + iy) * W + ix) * C4 + c4) * 4;
  f32x4 m = *reinterpret_cast<const f32x4*>(src);
  auto take = [&](const float* p) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
  };
  const bool right = ix + 1 < W, below = iy + 1 < H;
  if (right) take(src + C4 * 4);
  if (below) take(src + (size_t)W * C4 * 4);
  if (right && below) take(src + ((size_t)W + 1) * C4 * 4);
  *reinterpret_cast<f32x4*>(out + idx * 4) = m;
}

// ------------------------------------------------------------------------------------------------ dilated im2col
// in [B,h,w,C] -> out [B h w][(ky,kx,c)]: tap (ky,kx) reads pixel (y + (ky-1) dil, x + (kx-1) dil), zero outside
__global__ __launch_bounds__(256) void det_im2col_dil_kernel(const float* __restrict__ in, float* __restrict__ out, long long total4,
                                                             int h, int w, int C4, int dil) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total4) return;
  const int c4 = (int)(idx % C4);
  long long r = idx / C4;
  const int tap = (int)(r % 9);
  r /= 9;
  const int x = (int)(r % w);
  r /= w;
  const int y = (int)(r % h);
  const long long b = r / h;
  const int iy = y + (tap / 3 - 1) * dil, ix = x + (tap % 3 - 1) * dil;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (iy >= 0 && iy < h && ix >= 0 && ix < w) v = *reinterpret_cast<const f32x4*>(in + (((b * h + iy) * w + ix) * C4 + c4) * 4);
  *reinterpret_cast<f32x4*>(out + idx * 4) = v;
}

// ------------------------------------------------------------------------------------------------ ReLU in place
__global__ __launch_bounds__(256) void det_relu_kernel(float* __restrict__ x, long long total4) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total4) return;
  f32x4 v = *reinterpret_cast<f32x4*>(x + idx * 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = relu(v[e]);
  *reinterpret_cast<f32x4*>(x + idx * 4) = v;
}

// ------------------------------------------------------------------------------------------------ L2Norm
__device__ __forceinline__ float wave_sum(float v) {   // butterfly: every lane ends with the same sum, fixed order
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wave per pixel: in [rows, C] -> out [rows, C] = x / (sqrt(sum_c x^2) + 1e-10)
__global__ __launch_bounds__(256) void det_l2norm_kernel(const float* __restrict__ in, float* __restrict__ out, long long rows, int C) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* src = in + row * C;
  float s = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) s = fmaf(v[e], v[e], s);
  }
  const float norm = sqrtf(wave_sum(s)) + 1e-10f;
  for (int c = lane * 4; c < C; c += 256) {
    f32x4 v = *reinterpret_cast<const f32x4*>(src + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] / norm;
    *reinterpret_cast<f32x4*>(out + row * C + c) = v;
  }
}

// ------------------------------------------------------------------------------------------------ heads
constexpr int HN = 8;     // 4 loc + 4 conf rows (conf[1..5] have two, the other two rows are zero)
constexpr int HPIX = 4;   // pixels of a row per wave: the weight vectors a lane loads serve all four

// in [B,h,w,C], wt [8][(ky,kx,c)], bias [8] -> loc [B,P,4] and conf [B,P,2] at priors p0 + y w + x
__global__ __launch_bounds__(256) void det_head_kernel(const float* __restrict__ in, const float* __restrict__ wt,
                                                       const float* __restrict__ bias, float* __restrict__ loc,
                                                       float* __restrict__ conf, long long groups, int h, int w, int C, int P, int p0,
                                                       int maxout) {
  const long long grp = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (grp >= groups) return;
  const int lane = threadIdx.x & 63;
  const int gx = (w + HPIX - 1) / HPIX;
  const int x0 = (int)(grp % gx) * HPIX;
  long long r = grp / gx;
  const int y = (int)(r % h);
  const long long b = r / h;
  float acc[HPIX][HN];
#pragma unroll
  for (int p = 0; p < HPIX; ++p)
#pragma unroll
    for (int o = 0; o < HN; ++o) acc[p][o] = 0.f;
  for (int t = 0; t < 9; ++t) {
    const int iy = y + t / 3 - 1, dx = t % 3 - 1;
    if (iy < 0 || iy >= h) continue;
    const float* row = in + (b * h + iy) * (long long)w * C;
    for (int c = lane * 4; c < C; c += 256) {
      f32x4 wv[HN];
#pragma unroll
      for (int o = 0; o < HN; ++o) wv[o] = *reinterpret_cast<const f32x4*>(wt + ((size_t)o * 9 + t) * C + c);
#pragma unroll
      for (int p = 0; p < HPIX; ++p) {
        const int ix = x0 + p + dx;
        if (ix < 0 || ix >= w) continue;
        const f32x4 xv = *reinterpret_cast<const f32x4*>(row + (size_t)ix * C + c);
#pragma unroll
        for (int o = 0; o < HN; ++o)
#pragma unroll
          for (int e = 0; e < 4; ++e) {   // the result pinned: keeps the compiler from packing two rows' FMAs around a scalar taken
            float a = fmaf(wv[o][e], xv[e], acc[p][o]);   // from the high half of a register pair (ir_common.h fma4_scalar)
            asm("" : "+v"(a));
            acc[p][o] = a;
          }
      }
    }
  }
#pragma unroll
  for (int p = 0; p < HPIX; ++p)
#pragma unroll
    for (int o = 0; o < HN; ++o) acc[p][o] = wave_sum(acc[p][o]);
  if (lane != 0) return;
#pragma unroll
  for (int p = 0; p < HPIX; ++p) {
    if (x0 + p >= w) continue;
    float v[HN];
#pragma unroll
    for (int o = 0; o < HN; ++o) v[o] = acc[p][o] + bias[o];
    const size_t q = (size_t)b * P + p0 + (size_t)y * w + x0 + p;
    *reinterpret_cast<f32x4*>(loc + q * 4) = f32x4{v[0], v[1], v[2], v[3]};
    if (maxout) {
      const float m01 = v[4] > v[5] ? v[4] : v[5];
      conf[q * 2] = m01 > v[6] ? m01 : v[6];
      conf[q * 2 + 1] = v[7];
    } else {
      conf[q * 2] = v[4];
      conf[q * 2 + 1] = v[5];
    }
  }
}

// ------------------------------------------------------------------------------------------------ priors, decode, score
struct DetGeom {
  int H, W;        // the network's input
  int h[6], w[6];  // the six source maps
  int off[7];      // first prior of each map; off[6] = P
};

// loc [B,P,4], conf [B,P,2] -> det [B,P,5].  The prior in double, rounded to float once, as PriorBox.forward's Python floats
// go through torch.FloatTensor (box_utils.py:195-212); decode (box_utils.py:54-58) in float without contraction, as separate
// tensor operations give it; the score is softmax(conf)[1] in the difference form 1 / (1 + exp(l0 - l1)).
__global__ __launch_bounds__(256) void det_decode_kernel(const float* __restrict__ loc, const float* __restrict__ conf,
                                                         float* __restrict__ det, long long total, DetGeom G) {
#pragma clang fp contract(off)
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int P = G.off[6], p = (int)(idx % P);
  int k = 0;
  while (k < 5 && p >= G.off[k + 1]) ++k;
  const int q = p - G.off[k], i = q / G.w[k], j = q - i * G.w[k];
  const double step = (double)(4 << k), min_size = (double)(16 << k);
  const double f_kw = (double)G.W / step, f_kh = (double)G.H / step;
  const float cx = (float)(((double)j + 0.5) / f_kw), cy = (float)(((double)i + 0.5) / f_kh);
  const float sw = (float)(min_size / (double)G.W), sh = (float)(min_size / (double)G.H);
  const f32x4 l = *reinterpret_cast<const f32x4*>(loc + idx * 4);
  const float bx = cx + l[0] * 0.1f * sw, by = cy + l[1] * 0.1f * sh;
  const float bw = sw * expf(l[2] * 0.2f), bh = sh * expf(l[3] * 0.2f);
  const float x1 = bx - bw / 2.f, y1 = by - bh / 2.f;
  float* d = det + idx * 5;
  d[0] = 1.f / (1.f + expf(conf[idx * 2] - conf[idx * 2 + 1]));
  d[1] = x1;
  d[2] = y1;
  d[3] = bw + x1;
  d[4] = bh + y1;
}

// ------------------------------------------------------------------------------------------------ launchers
constexpr long long kMaxBytes = 1ll << 31;   // no operand of one launch reaches 2 GiB

int grid_for(long long items, int per_block, unsigned* grid) {
  const long long g = (items + per_block - 1) / per_block;
  CASYNC_REQUIRE(g >= 1 && g < (1ll << 31), "s3fd: grid of %lld blocks", g);
  *grid = (unsigned)g;
  return CASYNC_OK;
}

int launch_det_stem(const void* x, bool u8, const float* w, const float* bias, float* out, int batch, int H, int W, hipStream_t s) {
  CASYNC_REQUIRE(x && w && bias && out, "s3fd stem: null pointer");
  CASYNC_REQUIRE(batch > 0 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192, "s3fd stem: B=%d %dx%d", batch, H, W);
  const long long pixels = (long long)batch * H * W;
  CASYNC_REQUIRE(pixels * SC * 4 < kMaxBytes, "s3fd stem: output of %lld bytes (2 GiB or more)", pixels * SC * 4);
  unsigned grid;
  if (int st = grid_for(pixels, 4, &grid)) return st;
  if (u8) return casync_launch(det_stem_kernel<true>, dim3(grid), dim3(256), 0, s, x, w, bias, out, pixels, H, W);
  return casync_launch(det_stem_kernel<false>, dim3(grid), dim3(256), 0, s, x, w, bias, out, pixels, H, W);
}

int launch_det_maxpool(const float* in, float* out, int batch, int H, int W, int C, bool ceil_mode, hipStream_t s) {
  CASYNC_REQUIRE(in && out, "s3fd maxpool: null pointer");
  CASYNC_REQUIRE(batch > 0 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "s3fd maxpool: B=%d %dx%dx%d (C a multiple of 4)", batch, H, W, C);
  CASYNC_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0, "s3fd maxpool: 16-B alignment");
  const int Ho = ceil_mode ? (H + 1) / 2 : H / 2, Wo = ceil_mode ? (W + 1) / 2 : W / 2;
  CASYNC_REQUIRE(Ho >= 1 && Wo >= 1, "s3fd maxpool: %dx%d pools to nothing", H, W);
  CASYNC_REQUIRE((long long)batch * H * W * C * 4 < kMaxBytes, "s3fd maxpool: input of 2 GiB or more");
  const long long total4 = (long long)batch * Ho * Wo * (C / 4);
  unsigned grid;
  if (int st = grid_for(total4, 256, &grid)) return st;
  return casync_launch(det_maxpool_kernel, dim3(grid), dim3(256), 0, s, in, out, total4, H, W, C / 4, Ho, Wo);
}

int launch_det_im2col_dil(const float* in, float* out, int batch, int h, int w, int C, int dil, hipStream_t s) {
  CASYNC_REQUIRE(in && out, "s3fd im2col: null pointer");
  CASYNC_REQUIRE(batch > 0 && h >= 1 && w >= 1 && C >= 4 && C % 4 == 0 && dil >= 1 && dil <= 64, "s3fd im2col: B=%d %dx%dx%d dilation %d",
                 batch, h, w, C, dil);
  CASYNC_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0, "s3fd im2col: 16-B alignment");
  const long long total4 = (long long)batch * h * w * 9 * (C / 4);
  CASYNC_REQUIRE(total4 * 16 < kMaxBytes, "s3fd im2col: output of 2 GiB or more");
  unsigned grid;
  if (int st = grid_for(total4, 256, &grid)) return st;
  return casync_launch(det_im2col_dil_kernel, dim3(grid), dim3(256), 0, s, in, out, total4, h, w, C / 4, dil);
}

int launch_det_relu(float* x, long long n, hipStream_t s) {
  CASYNC_REQUIRE(x && n > 0 && n % 4 == 0 && (uintptr_t)x % 16 == 0, "s3fd relu: n=%lld (a multiple of 4, 16-B aligned)", n);
  CASYNC_REQUIRE(n * 4 < kMaxBytes, "s3fd relu: 2 GiB or more");
  unsigned grid;
  if (int st = grid_for(n / 4, 256, &grid)) return st;
  return casync_launch(det_relu_kernel, dim3(grid), dim3(256), 0, s, x, n / 4);
}

int launch_det_l2norm(const float* in, float* out, long long rows, int C, hipStream_t s) {
  CASYNC_REQUIRE(in && out && rows > 0 && C >= 4 && C % 4 == 0, "s3fd l2norm: rows %lld C %d (a multiple of 4)", rows, C);
  CASYNC_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0, "s3fd l2norm: 16-B alignment");
  CASYNC_REQUIRE(rows * C * 4 < kMaxBytes, "s3fd l2norm: 2 GiB or more");
  unsigned grid;
  if (int st = grid_for(rows, 4, &grid)) return st;
  return casync_launch(det_l2norm_kernel, dim3(grid), dim3(256), 0, s, in, out, rows, C);
}

int launch_det_head(const float* in, const float* wt, const float* bias, float* loc, float* conf, int batch, int h, int w, int C, int P,
                    int p0, bool maxout, hipStream_t s) {
  CASYNC_REQUIRE(in && wt && bias && loc && conf, "s3fd head: null pointer");
  CASYNC_REQUIRE(batch > 0 && h >= 1 && w >= 1 && C >= 4 && C % 4 == 0, "s3fd head: B=%d %dx%dx%d (C a multiple of 4)", batch, h, w, C);
  CASYNC_REQUIRE(p0 >= 0 && (long long)p0 + (long long)h * w <= P, "s3fd head: priors %d + %dx%d of %d", p0, h, w, P);
  CASYNC_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)wt % 16 == 0 && (uintptr_t)loc % 16 == 0 && (uintptr_t)conf % 8 == 0,
                 "s3fd head: alignment");
  CASYNC_REQUIRE((long long)batch * h * w * C * 4 < kMaxBytes && (long long)batch * P * 16 < kMaxBytes, "s3fd head: 2 GiB or more");
  const long long groups = (long long)batch * h * ((w + HPIX - 1) / HPIX);
  unsigned grid;
  if (int st = grid_for(groups, 4, &grid)) return st;
  return casync_launch(det_head_kernel, dim3(grid), dim3(256), 0, s, in, wt, bias, loc, conf, groups, h, w, C, P, p0, maxout ? 1 : 0);
}

// the sizes S3FDNet.forward goes through (nets.py:34-75,81-86): pools 1, 2, 4, 5 floor, pool 3 ceil, the extras' stride-2 convs
bool det_geometry(int H, int W, DetGeom* G) {
  if (H < 1 || W < 1 || H > 8192 || W > 8192) return false;
  auto half = [](int v) { return v / 2; };
  auto s2 = [](int v) { return (v - 1) / 2 + 1; };
  G->H = H, G->W = W;
  const int h3 = half(half(H)), w3 = half(half(W));
  if (h3 < 1 || w3 < 1) return false;
  G->h[0] = h3, G->w[0] = w3;
  G->h[1] = (h3 + 1) / 2, G->w[1] = (w3 + 1) / 2;
  G->h[2] = half(G->h[1]), G->w[2] = half(G->w[1]);
  G->h[3] = half(G->h[2]), G->w[3] = half(G->w[2]);
  if (G->h[3] < 1 || G->w[3] < 1) return false;   // a pooled dimension of 0: the reference raises there too
  G->h[4] = s2(G->h[3]), G->w[4] = s2(G->w[3]);
  G->h[5] = s2(G->h[4]), G->w[5] = s2(G->w[4]);
  G->off[0] = 0;
  for (int k = 0; k < 6; ++k) G->off[k + 1] = G->off[k] + G->h[k] * G->w[k];
  return true;
}

int launch_det_decode(const float* loc, const float* conf, float* det, int batch, const DetGeom& G, hipStream_t s) {
  CASYNC_REQUIRE(loc && conf && det && batch > 0, "s3fd decode: null pointer or empty batch");
  CASYNC_REQUIRE((uintptr_t)loc % 16 == 0 && (uintptr_t)conf % 4 == 0 && (uintptr_t)det % 4 == 0, "s3fd decode: alignment");
  const long long total = (long long)batch * G.off[6];
  CASYNC_REQUIRE(total * 20 < kMaxBytes, "s3fd decode: 2 GiB or more");
  unsigned grid;
  if (int st = grid_for(total, 256, &grid)) return st;
  return casync_launch(det_decode_kernel, dim3(grid), dim3(256), 0, s, loc, conf, det, total, G);
}

// ------------------------------------------------------------------------------------------------ network, packed layout
struct DetConv {
  const char* name;
  int cin, cout;
};
// the dense 3x3 convs behind conv1_1, with the pool that follows (0 none, 1 floor, 2 ceil) and the source they are (-1 none)
struct VggStep {
  DetConv c;
  int pool, source, stage;
};
const VggStep kVgg[] = {
    {{"conv1_2", 64, 64}, 1, -1, 0},   {{"conv2_1", 64, 128}, 0, -1, -1},  {{"conv2_2", 128, 128}, 1, -1, 1},
    {{"conv3_1", 128, 256}, 0, -1, -1}, {{"conv3_2", 256, 256}, 0, -1, -1}, {{"conv3_3", 256, 256}, 2, 0, 2},
    {{"conv4_1", 256, 512}, 0, -1, -1}, {{"conv4_2", 512, 512}, 0, -1, -1}, {{"conv4_3", 512, 512}, 1, 1, 3},
    {{"conv5_1", 512, 512}, 0, -1, -1}, {{"conv5_2", 512, 512}, 0, -1, -1}, {{"conv5_3", 512, 512}, 1, 2, 4},
};
constexpr int kNVgg = 12;
const int kSrcC[6] = {256, 512, 512, 1024, 512, 256};
enum { ST_FC6 = 5, ST_FC7, ST_CONV6_2, ST_CONV7_2, ST_LOC, ST_CONF, ST_DET, kStages };

// the packed layout with every tensor's offset resolved once: a forward searches nothing
struct DetLayout {
  PackedLayout packed;
  int64_t stem_w, stem_b, vgg_w[kNVgg], vgg_b[kNVgg], fc6_w, fc6_b, fc7_w, fc7_b, ex_w[4], ex_b[4], head_w[6], head_b[6];
  DetLayout() {
    auto add = [this](const std::string& n, int64_t size) { return packed.add(n, size); };
    stem_w = add("conv1_1.w", 27 * SC), stem_b = add("conv1_1.b", SC);
    for (int i = 0; i < kNVgg; ++i) {
      const DetConv& c = kVgg[i].c;
      vgg_w[i] = add(std::string(c.name) + ".w", (int64_t)c.cout * 9 * c.cin), vgg_b[i] = add(std::string(c.name) + ".b", c.cout);
    }
    fc6_w = add("fc6.w", 1024ll * 9 * 512), fc6_b = add("fc6.b", 1024);
    fc7_w = add("fc7.w", 1024ll * 1024), fc7_b = add("fc7.b", 1024);
    ex_w[0] = add("conv6_1.w", 256ll * 1024), ex_b[0] = add("conv6_1.b", 256);
    ex_w[1] = add("conv6_2.w", 512ll * 9 * 256), ex_b[1] = add("conv6_2.b", 512);
    ex_w[2] = add("conv7_1.w", 128ll * 512), ex_b[2] = add("conv7_1.b", 128);
    ex_w[3] = add("conv7_2.w", 256ll * 9 * 128), ex_b[3] = add("conv7_2.b", 256);
    for (int k = 0; k < 6; ++k) {
      const std::string p = "head" + std::to_string(k);
      head_w[k] = add(p + ".w", (int64_t)HN * 9 * kSrcC[k]), head_b[k] = add(p + ".b", HN);
    }
  }
};
const DetLayout& det_layout() {
  static const DetLayout L;
  return L;
}

// frames of one pass through the network: the whole batch unless its largest activation (conv1's, H W 64 values a frame, of 4
// bytes in fp32 and 2 in bf16) would reach 2 GiB
int det_sub_batch(int batch, int H, int W, int bytes_per_value) {
  const long long per_frame = (long long)H * W * SC * bytes_per_value;
  const long long fit = (kMaxBytes - 1) / per_frame;
  return (int)(fit < batch ? fit : batch);
}

// the arena of one pass: two activations and fc6's im2col matrix of T, fp32 loc / conf, every part on a 256-B boundary.  In
// fp32 this is the rule in floats it replaces: round64(n) * 4 == (4 n + 255) / 256 * 256, so the offsets and the total are the same.
template <class T>
struct DetWs {
  T *a, *b, *col;
  float *loc, *conf;
  int64_t bytes;
  DetWs(void* base, int nb, const DetGeom& G) {
    int64_t off = 0;
    auto take = [&](int64_t n_bytes) {
      char* p = base ? static_cast<char*>(base) + off : nullptr;
      off += (n_bytes + 255) / 256 * 256;
      return p;
    };
    const int64_t act = (int64_t)nb * G.H * G.W * SC * sizeof(T);
    a = reinterpret_cast<T*>(take(act)), b = reinterpret_cast<T*>(take(act));
    col = reinterpret_cast<T*>(take((int64_t)nb * G.h[3] * G.w[3] * 9 * 512 * sizeof(T)));
    loc = reinterpret_cast<float*>(take((int64_t)nb * G.off[6] * 16)), conf = reinterpret_cast<float*>(take((int64_t)nb * G.off[6] * 8));
    bytes = off;
  }
};

}  // namespace

struct casync_s3fd {
  int device = 0;
  int precision = 0;             // 0 fp32 (DetF32), 1 bf16 (DetBF16)
  PackedWeights pw;              // precision 1: the conv / GEMM matrices are read from the bf16 image
  hipEvent_t ev_fwd = nullptr;   // forward gate slot
};

namespace {
#define DT(call)                        \
  do {                                  \
    if (int st__ = (call)) return st__; \
  } while (0)

// A precision of the handle: the element type of the activations, the launchers of that type (named where their arguments are
// what det_pass hands them, wrapped in a line where not) and the image the conv / GEMM matrices are read from.  What the network
// does is in det_pass.
struct DetF32 {
  using T = float;
  static constexpr auto stem = launch_det_stem;
  static constexpr auto l2norm = launch_det_l2norm;
  static constexpr auto maxpool = launch_det_maxpool;
  static constexpr auto im2col = launch_det_im2col_dil;
  static constexpr auto head = launch_det_head;
  static const T* mats(const casync_s3fd* D) { return D->pw.w; }
  static int conv3x3(const T* in, const T* w, T* out, int nb, int h, int wd, int cin, int cout, int stride, const GemmEpilogue& epi,
                     hipStream_t s) {
    return launch_conv3x3_gemm(in, w, out, cout, nb, h, wd, cin, cout, stride, stride, 1, epi, s);
  }
  static int dense(const T* a, int m, int k, const T* w, const float* bias, T* c, int n, hipStream_t s) {   // rows GEMM, ReLU pass
    GemmEpilogue epi;
    epi.bias = bias;
    DT(launch_rows_gemm(a, k, w, c, n, m, n, k, epi, s));
    return launch_det_relu(c, (long long)m * n, s);
  }
  static int tap_out(const T* src, float* out, int64_t n, hipStream_t s) {
    CASYNC_CHECK_HIP(hipMemcpyAsync(out, src, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    return CASYNC_OK;
  }
};

// the contract: DESIGN section 8d, "bf16 precision"; a tap of a bf16 stage is widened
struct DetBF16 {
  using T = bf16_t;
  static constexpr auto stem = launch_det16_stem;
  static constexpr auto l2norm = launch_det16_l2norm;
  static constexpr auto maxpool = launch_det16_maxpool;
  static constexpr auto im2col = launch_det16_im2col_dil;
  static constexpr auto head = launch_det16_head;
  static constexpr auto tap_out = launch_det16_widen;
  static const T* mats(const casync_s3fd* D) { return D->pw.w16; }
  static int conv3x3(const T* in, const T* w, T* out, int nb, int h, int wd, int cin, int cout, int stride, const GemmEpilogue& epi,
                     hipStream_t s) {
    return launch_conv3x3_gemm(in, w, out, cout, nb, h, wd, cin, cout, stride, stride, 1, epi, s, DT_BF16);
  }
  static int dense(const T* a, int m, int k, const T* w, const float* bias, T* c, int n, hipStream_t s) {
    DT(launch_rows_gemm_bf16(a, k, w, bias, c, n, m, n, k, s));
    return launch_det16_relu(c, (long long)m * n, s);
  }
};

// One pass of nb frames in the precision P; `out` is the stage's tensor for these frames.  Returns after the stage asked for.
// w is the fp32 packed buffer (biases, stem, heads), wm the image the 3x3 conv and GEMM matrices come from.
template <class P>
int det_pass(const casync_s3fd* D, const void* x, bool u8, int nb, const DetGeom& G, const DetWs<typename P::T>& ws, float* out, int stage,
             hipStream_t s) {
  using T = typename P::T;
  const DetLayout& L = det_layout();
  const float* w = D->pw.w;
  const T* wm = P::mats(D);
  const int np = G.off[6];
  auto head = [&](int k, const T* src) -> int {
    return P::head(src, w + L.head_w[k], w + L.head_b[k], ws.loc, ws.conf, nb, G.h[k], G.w[k], kSrcC[k], np, G.off[k], k == 0, s);
  };
  auto relu_bias = [&](int64_t b_off) {
    GemmEpilogue epi;
    epi.bias = w + b_off;
    epi.act = 2;
    return epi;
  };
  T *cur = ws.a, *nxt = ws.b;
  DT(P::stem(x, u8, w + L.stem_w, w + L.stem_b, cur, nb, G.H, G.W, s));
  int h = G.H, wd = G.W;
  for (int i = 0; i < kNVgg; ++i) {
    const VggStep& v = kVgg[i];
    DT(P::conv3x3(cur, wm + L.vgg_w[i], nxt, nb, h, wd, v.c.cin, v.c.cout, 1, relu_bias(L.vgg_b[i]), s));
    std::swap(cur, nxt);
    if (v.stage == stage) return P::tap_out(cur, out, (int64_t)nb * h * wd * v.c.cout, s);
    if (v.source >= 0) {   // the normalised map feeds the two heads only
      DT(P::l2norm(cur, nxt, (long long)nb * h * wd, v.c.cout, s));
      DT(head(v.source, nxt));
    }
    if (v.pool) {
      DT(P::maxpool(cur, nxt, nb, h, wd, v.c.cout, v.pool == 2, s));
      std::swap(cur, nxt);
      h = v.pool == 2 ? (h + 1) / 2 : h / 2, wd = v.pool == 2 ? (wd + 1) / 2 : wd / 2;
    }
  }
  // a 1x1 conv (or fc6 on its im2col matrix) + ReLU over m pixels
  auto dense = [&](const T* a, int m, int k, int64_t w_off, int64_t b_off, T* c, int n) -> int {
    return P::dense(a, m, k, wm + w_off, w + b_off, c, n, s);
  };
  const int m = nb * h * wd;   // pixels at 1/32 resolution
  DT(P::im2col(cur, ws.col, nb, h, wd, 512, 6, s));
  DT(dense(ws.col, m, 9 * 512, L.fc6_w, L.fc6_b, nxt, 1024));
  std::swap(cur, nxt);
  if (stage == ST_FC6) return P::tap_out(cur, out, (int64_t)m * 1024, s);
  DT(dense(cur, m, 1024, L.fc7_w, L.fc7_b, nxt, 1024));
  std::swap(cur, nxt);
  if (stage == ST_FC7) return P::tap_out(cur, out, (int64_t)m * 1024, s);
  DT(head(3, cur));
  const int ex_c[5] = {1024, 256, 512, 128, 256};
  for (int j = 0; j < 2; ++j) {   // extras 2j (1x1) and 2j + 1 (3x3, stride 2, pad 1): nets.py:135-138
    DT(dense(cur, nb * G.h[3 + j] * G.w[3 + j], ex_c[2 * j], L.ex_w[2 * j], L.ex_b[2 * j], nxt, ex_c[2 * j + 1]));
    DT(P::conv3x3(nxt, wm + L.ex_w[2 * j + 1], cur, nb, G.h[3 + j], G.w[3 + j], ex_c[2 * j + 1], ex_c[2 * j + 2], 2,
                  relu_bias(L.ex_b[2 * j + 1]), s));
    if (stage == ST_CONV6_2 + j) return P::tap_out(cur, out, (int64_t)nb * G.h[4 + j] * G.w[4 + j] * ex_c[2 * j + 2], s);
    DT(head(4 + j, cur));
  }
  if (stage == ST_LOC) return DetF32::tap_out(ws.loc, out, (int64_t)nb * np * 4, s);   // loc, conf and det are fp32 in both
  if (stage == ST_CONF) return DetF32::tap_out(ws.conf, out, (int64_t)nb * np * 2, s);
  return launch_det_decode(ws.loc, ws.conf, out, nb, G, s);
}

int64_t det_stage_floats(const DetGeom& G, int stage) {   // per frame
  const int c[5] = {64, 128, 256, 512, 512};
  if (stage == 0) return (int64_t)G.H * G.W * c[0];
  if (stage == 1) return (int64_t)(G.H / 2) * (G.W / 2) * c[1];
  if (stage >= 2 && stage <= 4) return (int64_t)G.h[stage - 2] * G.w[stage - 2] * c[stage];
  if (stage == ST_FC6 || stage == ST_FC7) return (int64_t)G.h[3] * G.w[3] * 1024;
  if (stage == ST_CONV6_2) return (int64_t)G.h[4] * G.w[4] * 512;
  if (stage == ST_CONV7_2) return (int64_t)G.h[5] * G.w[5] * 256;
  if (stage == ST_LOC) return (int64_t)G.off[6] * 4;
  if (stage == ST_CONF) return (int64_t)G.off[6] * 2;
  return (int64_t)G.off[6] * 5;
}

// the checked batch in passes of nb frames at the most, in the arena of the precision P
template <class P>
int det_batches(casync_s3fd* D, const void* x, bool u8, int batch, int nb, const DetGeom& G, float* out, void* ws_dev, int64_t ws_bytes,
                hipStream_t s, int stage) {
  const DetWs<typename P::T> ws(ws_dev, nb, G);
  if (ws_bytes < ws.bytes) {
    casync_set_error("s3fd forward: workspace %lld bytes, needs %lld", (long long)ws_bytes, (long long)ws.bytes);
    return CASYNC_ERR_STATE;
  }
  DeviceGuard guard(D->device);
  CASYNC_CHECK_HIP(guard.err);
  std::unique_lock<std::mutex> gate_lock;   // held until this forward is enqueued
  if (int st = casync_gate_enter(D->device, D, &D->ev_fwd, s, &gate_lock)) return st;
  const int64_t in_frame = (int64_t)G.H * G.W * 3 * (u8 ? 1 : 4), out_frame = det_stage_floats(G, stage);
  // every pass takes the tile choices of its own frame count; the kernels' sums do not depend on it (see the header comment)
  for (int b0 = 0; b0 < batch; b0 += nb) {
    const int n = batch - b0 < nb ? batch - b0 : nb;
    DT(det_pass<P>(D, static_cast<const char*>(x) + (size_t)b0 * in_frame, u8, n, G, ws, out + (size_t)b0 * out_frame, stage, s));
  }
  return CASYNC_OK;
}

int det_run(casync_s3fd* D, const void* x, bool u8, int batch, int H, int W, float* out, void* ws_dev, int64_t ws_bytes, hipStream_t s,
            int stage) {
  CASYNC_REQUIRE(D, "s3fd forward: null handle");
  const bool h16 = D->precision == 1;
  CASYNC_REQUIRE(D->pw.w && (!h16 || D->pw.w16), "s3fd forward: weights not loaded");
  CASYNC_REQUIRE(batch >= 0 && batch <= 65536, "s3fd forward: batch %d (0..65536)", batch);
  CASYNC_REQUIRE(stage >= 0 && stage < kStages, "s3fd forward: stage %d (0..%d)", stage, kStages - 1);
  DetGeom G;
  CASYNC_REQUIRE(det_geometry(H, W, &G), "s3fd forward: frames of %d x %d pool to nothing (or exceed 8192): the network needs 16 x 16 at least",
                 H, W);
  const int nb = det_sub_batch(batch, H, W, h16 ? 2 : 4);
  CASYNC_REQUIRE(batch == 0 || nb >= 1, "s3fd forward: one %d x %d frame alone has an activation of 2 GiB or more", H, W);
  if (batch == 0) return CASYNC_OK;
  CASYNC_REQUIRE(x && out && ws_dev, "s3fd forward: null pointer");
  CASYNC_REQUIRE((uintptr_t)x % (u8 ? 1 : 4) == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)ws_dev % 256 == 0, "s3fd forward: alignment");
  return h16 ? det_batches<DetBF16>(D, x, u8, batch, nb, G, out, ws_dev, ws_bytes, s, stage)
             : det_batches<DetF32>(D, x, u8, batch, nb, G, out, ws_dev, ws_bytes, s, stage);
}
#undef DT
}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

int casync_s3fd_packed_count(void) { return det_layout().packed.count(); }
const char* casync_s3fd_packed_name(int i) { return det_layout().packed.name(i); }
int64_t casync_s3fd_packed_offset(int i) { return det_layout().packed.offset(i); }
int64_t casync_s3fd_packed_size(int i) { return det_layout().packed.size(i); }
int64_t casync_s3fd_packed_total(void) { return det_layout().packed.total; }
int64_t casync_s3fd_priors(int h, int w) {
  DetGeom G;
  return det_geometry(h, w, &G) ? G.off[6] : 0;
}
int casync_s3fd_map_size(int h, int w, int k, int* map_h, int* map_w) {
  DetGeom G;
  CASYNC_REQUIRE(map_h && map_w && k >= 0 && k < 6 && det_geometry(h, w, &G), "s3fd_map_size: map %d of a %d x %d frame", k, h, w);
  *map_h = G.h[k], *map_w = G.w[k];
  return CASYNC_OK;
}
int64_t casync_s3fd_workspace_bytes_ex(int precision, int batch, int h, int w) {
  DetGeom G;
  if ((precision != 0 && precision != 1) || batch < 1 || batch > 65536 || !det_geometry(h, w, &G)) return 0;
  const int nb = det_sub_batch(batch, h, w, precision == 1 ? 2 : 4);
  if (nb < 1) return 0;
  return precision == 1 ? DetWs<bf16_t>(nullptr, nb, G).bytes : DetWs<float>(nullptr, nb, G).bytes;
}
int64_t casync_s3fd_workspace_bytes(int batch, int h, int w) { return casync_s3fd_workspace_bytes_ex(0, batch, h, w); }

int casync_s3fd_create(int device_id, casync_s3fd_handle* out) { return casync_s3fd_create_ex(device_id, 0, out); }
int casync_s3fd_precision(casync_s3fd_handle h) { return h ? h->precision : -1; }

int casync_s3fd_create_ex(int device_id, int precision, casync_s3fd_handle* out) {
  CASYNC_REQUIRE(out, "s3fd_create: null out");
  *out = nullptr;
  CASYNC_REQUIRE(precision == 0 || precision == 1, "s3fd_create: precision %d (0 fp32, 1 bf16)", precision);
  if (int st = casync_require_gfx950("s3fd_create", device_id)) return st;
  casync_s3fd* h = new casync_s3fd();
  h->device = device_id;
  h->precision = precision;
  *out = h;
  return CASYNC_OK;
}

void casync_s3fd_destroy(casync_s3fd_handle h) {
  if (!h) return;
  DeviceGuard guard(h->device);
  casync_gate_forget(h->device, h, &h->ev_fwd);
  h->pw.release();
  delete h;
}

int casync_s3fd_load_weights_host(casync_s3fd_handle h, const float* packed, int64_t n_floats) {
  CASYNC_REQUIRE(h, "s3fd_load_weights: null");
  return h->pw.load_host("s3fd_load_weights", h->device, packed, n_floats, det_layout().packed.total, h->precision == 1);
}

int casync_s3fd_load_weights_device(casync_s3fd_handle h, const float* packed_dev, int64_t n_floats) {
  CASYNC_REQUIRE(h, "s3fd_load_weights_device: null");
  return h->pw.adopt_device("s3fd_load_weights_device", h->device, packed_dev, n_floats, det_layout().packed.total,
                            h->precision == 1);
}

int casync_s3fd_forward(casync_s3fd_handle h, const float* x_dev, int batch, int H, int W, float* det_dev, void* workspace_dev,
                        int64_t workspace_bytes, casync_stream stream) {
  return det_run(h, x_dev, false, batch, H, W, det_dev, workspace_dev, workspace_bytes, (hipStream_t)stream, ST_DET);
}
int casync_s3fd_forward_u8(casync_s3fd_handle h, const uint8_t* frames_dev, int batch, int H, int W, float* det_dev, void* workspace_dev,
                           int64_t workspace_bytes, casync_stream stream) {
  return det_run(h, frames_dev, true, batch, H, W, det_dev, workspace_dev, workspace_bytes, (hipStream_t)stream, ST_DET);
}
int casync_s3fd_forward_tap(casync_s3fd_handle h, const void* in_dev, int input_u8, int batch, int H, int W, int stage, float* out_dev,
                            void* workspace_dev, int64_t workspace_bytes, casync_stream stream) {
  return det_run(h, in_dev, input_u8 != 0, batch, H, W, out_dev, workspace_dev, workspace_bytes, (hipStream_t)stream, stage);
}

int casync_op_s3fd_stem(const void* x, int input_u8, const float* w, const float* bias, float* out, int batch, int h, int w_,
                        casync_stream stream) {
  return launch_det_stem(x, input_u8 != 0, w, bias, out, batch, h, w_, (hipStream_t)stream);
}
int casync_op_s3fd_maxpool(const float* in, float* out, int batch, int h, int w_, int c, int ceil_mode, casync_stream stream) {
  return launch_det_maxpool(in, out, batch, h, w_, c, ceil_mode != 0, (hipStream_t)stream);
}
int casync_op_s3fd_im2col_dil(const float* in, float* out, int batch, int h, int w_, int c, int dilation, casync_stream stream) {
  return launch_det_im2col_dil(in, out, batch, h, w_, c, dilation, (hipStream_t)stream);
}
int casync_op_s3fd_relu(float* x, int64_t n, casync_stream stream) { return launch_det_relu(x, n, (hipStream_t)stream); }
int casync_op_s3fd_l2norm(const float* in, float* out, int64_t rows, int c, casync_stream stream) {
  return launch_det_l2norm(in, out, rows, c, (hipStream_t)stream);
}
int casync_op_s3fd_head(const float* in, const float* w, const float* bias, float* loc, float* conf, int batch, int h, int w_, int c,
                        int priors, int first_prior, int maxout, casync_stream stream) {
  return launch_det_head(in, w, bias, loc, conf, batch, h, w_, c, priors, first_prior, maxout != 0, (hipStream_t)stream);
}
int casync_op_s3fd_decode(const float* loc, const float* conf, float* det, int batch, int H, int W, casync_stream stream) {
  DetGeom G;
  CASYNC_REQUIRE(det_geometry(H, W, &G), "s3fd decode: frames of %d x %d pool to nothing", H, W);
  return launch_det_decode(loc, conf, det, batch, G, (hipStream_t)stream);
}

}  // extern "C"
