// The bf16 precision of the S3FD face detector (facedet.hip, casync_s3fd_create_ex with precision 1): the kernels that differ
// from the fp32 handle's.  Activations between the stages are bf16 NHWC, every sum is fp32, the stem and the six heads keep
// their fp32 weights.  Every kernel moves 16 bytes (8 values) per lane, channel fastest.
//
//   det16_stem_kernel<U8>     conv1_1 (3 -> 64, 3x3, pad 1) + ReLU in fp32 from float NCHW or uint8 HWC (the mean subtracted here),
//                             bf16 store.  A workgroup takes a 4 x 32 pixel tile: the 6 x 34 x 3 input patch and the 27 x 64
//                             weights are staged in LDS, a lane produces eight consecutive channels of four neighbouring pixels.
//   det16_maxpool_kernel      2x2 / 2 max pooling, floor or ceil form: exact.
//   det16_im2col_dil_kernel   the [B h w, 9 C] matrix of a dilated 3x3 conv (fc6), zero where a tap is outside: exact.
//   det16_relu_kernel         ReLU in place behind the bf16 rows GEMM (bias only in its epilogue): exact.
//   det16_l2norm_kernel       x / (sqrt(sum_c x^2) + 1e-10) per pixel: bf16 in, fp32 sum of squares, a true division, bf16 out.
//   det16_head_kernel         det_head_kernel's job from bf16 activations: fp32 weights and sums, fp32 loc / conf logits out.
//   det16_widen_kernel        bf16 -> fp32, the debug taps of the bf16 stages.
// conv1_2 .. conv5_3 and extras 1 and 3 run on the bf16 ring implicit-GEMM kernel (launch_conv3x3_gemm, DT_BF16), fc6 / fc7 and
// extras 0 and 2 on launch_rows_gemm_bf16; priors, decode and score stay on det_decode_kernel.  No kernel here sums across
// frames or uses an atomic.
#include "common.h"

namespace {

__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : 0.f; }

// ------------------------------------------------------------------------------------------------ stem
constexpr int SC = 64;             // channels of conv1_1
constexpr int TX = 32, TY = 4;     // pixels of a workgroup's tile: 8 x 4 lanes-groups of four neighbours in a row
constexpr int PW = TX + 2, PH = TY + 2;

// w [(ky,kx,ci)=27][64], out [B,H,W,64] bf16; 256 threads = 32 groups of four pixels x 8 groups of eight channels.
// The patch holds the same floats for both input forms (float32(u8) - mean is exact), so their outputs are bit-equal.
template <bool U8>
__global__ __launch_bounds__(256) void det16_stem_kernel(const void* __restrict__ xin, const float* __restrict__ w,
                                                         const float* __restrict__ bias, bf16_t* __restrict__ out, int H, int W,
                                                         int tiles_x, int tiles_y) {
  __shared__ __attribute__((aligned(16))) float s_w[27 * SC];
  __shared__ float s_in[3][PH][PW];
  const int tid = threadIdx.x;
  int t = blockIdx.x;
  const int tx = t % tiles_x;
  t /= tiles_x;
  const int ty = t % tiles_y;
  const long long b = t / tiles_y;
  const int xb = tx * TX, yb = ty * TY;
  for (int i = tid; i < 27 * SC; i += 256) s_w[i] = w[i];
  for (int i = tid; i < 3 * PH * PW; i += 256) {
    int ci, row, col;
    if (U8) {   // the bytes of a pixel are neighbours
      ci = i % 3, col = (i / 3) % PW, row = i / (3 * PW);
    } else {    // the columns of a plane are
      col = i % PW, row = (i / PW) % PH, ci = i / (PW * PH);
    }
    const int iy = yb + row - 1, ix = xb + col - 1;
    float v = 0.f;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
      if (U8) {
        const float mean = ci == 0 ? 123.f : ci == 1 ? 117.f : 104.f;
        v = (float)static_cast<const unsigned char*>(xin)[((b * H + iy) * W + ix) * 3 + ci] - mean;
      } else {
        v = static_cast<const float*>(xin)[((b * 3 + ci) * H + iy) * W + ix];
      }
    }
    s_in[ci][row][col] = v;
  }
  __syncthreads();
  const int cg = tid & 7, pg = tid >> 3;
  const int gx = pg & 7, gy = pg >> 3;
  const int y = yb + gy, x0 = xb + gx * 4;
  if (y >= H || x0 >= W) return;
  float acc[4][8];
  {
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bias + cg * 8), b1 = *reinterpret_cast<const f32x4*>(bias + cg * 8 + 4);
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[p][e] = b0[e], acc[p][4 + e] = b1[e];
  }
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) {
      float in6[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) in6[j] = s_in[ci][gy + ky][gx * 4 + j];
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const float* wp = s_w + ((ky * 3 + kx) * 3 + ci) * SC + cg * 8;
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp), w1 = *reinterpret_cast<const f32x4*>(wp + 4);
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int e = 0; e < 8; ++e) {   // the result pinned: no packed FMA around a scalar taken from a register pair's high half
            float a = fmaf(e < 4 ? w0[e & 3] : w1[e & 3], in6[p + kx], acc[p][e]);
            asm("" : "+v"(a));
            acc[p][e] = a;
          }
      }
    }
  }
  bf16_t* dst = out + (((b * H + y) * W + x0) * SC + cg * 8);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (x0 + p >= W) break;
    V16<bf16_t> o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.v[e] = relu(acc[p][e]);
    st16(dst + p * SC, o);
  }
}

// ------------------------------------------------------------------------------------------------ max pooling
__device__ __forceinline__ bf16x8 max8(bf16x8 a, bf16x8 b) {
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = (float)b[e] > (float)a[e] ? b[e] : a[e];
  return a;
}

// in [B,H,W,C] -> out [B,Ho,Wo,C], window 2x2 stride 2 clipped to the image (only the ceil form has a clipped window)
__global__ __launch_bounds__(256) void det16_maxpool_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, long long total8,
                                                            int H, int W, int C8, int Ho, int Wo) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total8) return;
  const int c8 = (int)(idx % C8);
  long long r = idx / C8;
  const int ox = (int)(r % Wo);
  r /= Wo;
  const int oy = (int)(r % Ho);
  const long long b = r / Ho;
  const int iy = 2 * oy, ix = 2 * ox;
  const bf16_t* src = in + (((b * H + iy) * W + ix) * C8 + c8) * 8;
  bf16x8 m = *reinterpret_cast<const bf16x8*>(src);
  const bool right = ix + 1 < W, below = iy + 1 < H;
  if (right) m = max8(m, *reinterpret_cast<const bf16x8*>(src + C8 * 8));
  if (below) m = max8(m, *reinterpret_cast<const bf16x8*>(src + (size_t)W * C8 * 8));
  if (right && below) m = max8(m, *reinterpret_cast<const bf16x8*>(src + ((size_t)W + 1) * C8 * 8));
  *reinterpret_cast<bf16x8*>(out + idx * 8) = m;
}

// ------------------------------------------------------------------------------------------------ dilated im2col
// in [B,h,w,C] -> out [B h w][(ky,kx,c)]: tap (ky,kx) reads pixel (y + (ky-1) dil, x + (kx-1) dil), zero outside
__global__ __launch_bounds__(256) void det16_im2col_dil_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out,
                                                               long long total8, int h, int w, int C8, int dil) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total8) return;
  const int c8 = (int)(idx % C8);
  long long r = idx / C8;
  const int tap = (int)(r % 9);
  r /= 9;
  const int x = (int)(r % w);
  r /= w;
  const int y = (int)(r % h);
  const long long b = r / h;
  const int iy = y + (tap / 3 - 1) * dil, ix = x + (tap % 3 - 1) * dil;
  u32x4 v = u32x4{0u, 0u, 0u, 0u};
  if (iy >= 0 && iy < h && ix >= 0 && ix < w) v = *reinterpret_cast<const u32x4*>(in + (((b * h + iy) * w + ix) * C8 + c8) * 8);
  *reinterpret_cast<u32x4*>(out + idx * 8) = v;
}

// ------------------------------------------------------------------------------------------------ ReLU in place
__global__ __launch_bounds__(256) void det16_relu_kernel(bf16_t* __restrict__ x, long long total8) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total8) return;
  bf16x8 v = *reinterpret_cast<bf16x8*>(x + idx * 8);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)v[e] > 0.f ? v[e] : (bf16_t)0.f;
  *reinterpret_cast<bf16x8*>(x + idx * 8) = v;
}

// ------------------------------------------------------------------------------------------------ bf16 -> fp32
__global__ __launch_bounds__(256) void det16_widen_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, long long total8) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total8) return;
  const V16<bf16_t> v = ld16(in + idx * 8);
  *reinterpret_cast<f32x4*>(out + idx * 8) = f32x4{v.v[0], v.v[1], v.v[2], v.v[3]};
  *reinterpret_cast<f32x4*>(out + idx * 8 + 4) = f32x4{v.v[4], v.v[5], v.v[6], v.v[7]};
}

// ------------------------------------------------------------------------------------------------ L2Norm
// in [rows, C] -> out [rows, C] = x / (sqrt(sum_c x^2) + 1e-10).  `lpr` lanes per row (32: two rows per wave, or 64), a lane
// owns columns 8 lane + 8 lpr j; the butterfly over the row's lanes gives every one of them the same sum in a fixed order.
__global__ __launch_bounds__(256) void det16_l2norm_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, long long rows, int C,
                                                           int lpr) {
  const int per_wave = 64 / lpr, lane = threadIdx.x & (lpr - 1);
  const long long row = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * per_wave + (threadIdx.x & 63) / lpr;
  const bool live = row < rows;
  const bf16_t* src = in + (live ? row : 0) * C;
  float s = 0.f;
  if (live)
    for (int c = lane * 8; c < C; c += lpr * 8) {
      const V16<bf16_t> v = ld16(src + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s = fmaf(v.v[e], v.v[e], s);
        asm("" : "+v"(s));   // a scalar chain
      }
    }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1)
    if (o < lpr) s += __shfl_xor(s, o, 64);
  if (!live) return;
  const float norm = sqrtf(s) + 1e-10f;
  for (int c = lane * 8; c < C; c += lpr * 8) {
    V16<bf16_t> v = ld16(src + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) v.v[e] = v.v[e] / norm;
    st16(out + row * C + c, v);
  }
}

// ------------------------------------------------------------------------------------------------ heads
constexpr int HN = 8;     // 4 loc + 4 conf rows (conf[1..5] have two, the other two rows are zero)
constexpr int HPIX = 4;   // pixels of a row per wave: the weight vectors a lane loads serve all four

__device__ __forceinline__ float wave_sum(float v) {   // butterfly: every lane ends with the same sum, fixed order
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// in [B,h,w,C] bf16, wt [8][(ky,kx,c)] fp32, bias [8] -> loc [B,P,4] and conf [B,P,2] at priors p0 + y w + x.  For one ky the
// taps (kx, c) of a pixel are 3 C consecutive values of the input row and of every weight row: the lanes split that range.
__global__ __launch_bounds__(256) void det16_head_kernel(const bf16_t* __restrict__ in, const float* __restrict__ wt,
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
  const int K3 = 3 * C;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = y + ky - 1;
    if (iy < 0 || iy >= h) continue;
    const bf16_t* row = in + (b * h + iy) * (long long)w * C;
    for (int j = lane * 8; j < K3; j += 512) {
      const int dx = j / C - 1;   // C is a multiple of 8: the lane's eight values belong to one kx
      bool any = false;
#pragma unroll
      for (int p = 0; p < HPIX; ++p) any = any || (x0 + p + dx >= 0 && x0 + p + dx < w);
      if (!any) continue;
      f32x4 wv[HN][2];
#pragma unroll
      for (int o = 0; o < HN; ++o) {
        const float* wp = wt + ((size_t)o * 9 + ky * 3) * C + j;
        wv[o][0] = *reinterpret_cast<const f32x4*>(wp), wv[o][1] = *reinterpret_cast<const f32x4*>(wp + 4);
      }
#pragma unroll
      for (int p = 0; p < HPIX; ++p) {
        const int ix = x0 + p + dx;
        if (ix < 0 || ix >= w) continue;
        const V16<bf16_t> xv = ld16(row + (long long)(x0 + p - 1) * C + j);
#pragma unroll
        for (int o = 0; o < HN; ++o)
#pragma unroll
          for (int e = 0; e < 8; ++e) {   // the result pinned, as in det_head_kernel
            float a = fmaf(wv[o][e >> 2][e & 3], xv.v[e], acc[p][o]);
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

// ------------------------------------------------------------------------------------------------ launchers
constexpr long long kMaxBytes = 1ll << 31;   // no operand of one launch reaches 2 GiB

int grid_for(long long items, int per_block, unsigned* grid) {
  const long long g = (items + per_block - 1) / per_block;
  CASYNC_REQUIRE(g >= 1 && g < (1ll << 31), "s3fd16: grid of %lld blocks", g);
  *grid = (unsigned)g;
  return CASYNC_OK;
}

}  // namespace

int launch_det16_stem(const void* x, bool u8, const float* w, const float* bias, void* out, int batch, int H, int W, hipStream_t s) {
  CASYNC_REQUIRE(x && w && bias && out, "s3fd16 stem: null pointer");
  CASYNC_REQUIRE(batch > 0 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192, "s3fd16 stem: B=%d %dx%d", batch, H, W);
  CASYNC_REQUIRE((uintptr_t)out % 16 == 0 && (uintptr_t)bias % 16 == 0 && (uintptr_t)x % (u8 ? 1 : 4) == 0, "s3fd16 stem: alignment");
  const long long pixels = (long long)batch * H * W;
  CASYNC_REQUIRE(pixels * SC * 2 < kMaxBytes, "s3fd16 stem: output of %lld bytes (2 GiB or more)", pixels * SC * 2);
  const int tiles_x = (W + TX - 1) / TX, tiles_y = (H + TY - 1) / TY;
  unsigned grid;
  if (int st = grid_for((long long)batch * tiles_x * tiles_y, 1, &grid)) return st;
  bf16_t* o = static_cast<bf16_t*>(out);
  if (u8) return casync_launch(det16_stem_kernel<true>, dim3(grid), dim3(256), 0, s, x, w, bias, o, H, W, tiles_x, tiles_y);
  return casync_launch(det16_stem_kernel<false>, dim3(grid), dim3(256), 0, s, x, w, bias, o, H, W, tiles_x, tiles_y);
}

int launch_det16_maxpool(const void* in, void* out, int batch, int H, int W, int C, bool ceil_mode, hipStream_t s) {
  CASYNC_REQUIRE(in && out, "s3fd16 maxpool: null pointer");
  CASYNC_REQUIRE(batch > 0 && H >= 1 && W >= 1 && C >= 8 && C % 8 == 0, "s3fd16 maxpool: B=%d %dx%dx%d (C a multiple of 8)", batch, H, W, C);
  CASYNC_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0, "s3fd16 maxpool: 16-B alignment");
  const int Ho = ceil_mode ? (H + 1) / 2 : H / 2, Wo = ceil_mode ? (W + 1) / 2 : W / 2;
  CASYNC_REQUIRE(Ho >= 1 && Wo >= 1, "s3fd16 maxpool: %dx%d pools to nothing", H, W);
  CASYNC_REQUIRE((long long)batch * H * W * C * 2 < kMaxBytes, "s3fd16 maxpool: input of 2 GiB or more");
  const long long total8 = (long long)batch * Ho * Wo * (C / 8);
  unsigned grid;
  if (int st = grid_for(total8, 256, &grid)) return st;
  return casync_launch(det16_maxpool_kernel, dim3(grid), dim3(256), 0, s, static_cast<const bf16_t*>(in), static_cast<bf16_t*>(out), total8,
                       H, W, C / 8, Ho, Wo);
}

int launch_det16_im2col_dil(const void* in, void* out, int batch, int h, int w, int C, int dil, hipStream_t s) {
  CASYNC_REQUIRE(in && out, "s3fd16 im2col: null pointer");
  CASYNC_REQUIRE(batch > 0 && h >= 1 && w >= 1 && C >= 8 && C % 8 == 0 && dil >= 1 && dil <= 64, "s3fd16 im2col: B=%d %dx%dx%d dilation %d",
                 batch, h, w, C, dil);
  CASYNC_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0, "s3fd16 im2col: 16-B alignment");
  const long long total8 = (long long)batch * h * w * 9 * (C / 8);
  CASYNC_REQUIRE(total8 * 16 < kMaxBytes, "s3fd16 im2col: output of 2 GiB or more");
  unsigned grid;
  if (int st = grid_for(total8, 256, &grid)) return st;
  return casync_launch(det16_im2col_dil_kernel, dim3(grid), dim3(256), 0, s, static_cast<const bf16_t*>(in), static_cast<bf16_t*>(out),
                       total8, h, w, C / 8, dil);
}

int launch_det16_relu(void* x, long long n, hipStream_t s) {
  CASYNC_REQUIRE(x && n > 0 && n % 8 == 0 && (uintptr_t)x % 16 == 0, "s3fd16 relu: n=%lld (a multiple of 8, 16-B aligned)", n);
  CASYNC_REQUIRE(n * 2 < kMaxBytes, "s3fd16 relu: 2 GiB or more");
  unsigned grid;
  if (int st = grid_for(n / 8, 256, &grid)) return st;
  return casync_launch(det16_relu_kernel, dim3(grid), dim3(256), 0, s, static_cast<bf16_t*>(x), n / 8);
}

int launch_det16_widen(const void* in, float* out, long long n, hipStream_t s) {
  CASYNC_REQUIRE(in && out && n > 0 && n % 8 == 0, "s3fd16 widen: n=%lld (a multiple of 8)", n);
  CASYNC_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0, "s3fd16 widen: 16-B alignment");
  CASYNC_REQUIRE(n * 4 < kMaxBytes, "s3fd16 widen: 2 GiB or more");
  unsigned grid;
  if (int st = grid_for(n / 8, 256, &grid)) return st;
  return casync_launch(det16_widen_kernel, dim3(grid), dim3(256), 0, s, static_cast<const bf16_t*>(in), out, n / 8);
}

int launch_det16_l2norm(const void* in, void* out, long long rows, int C, hipStream_t s) {
  CASYNC_REQUIRE(in && out && rows > 0 && C >= 8 && C % 8 == 0, "s3fd16 l2norm: rows %lld C %d (a multiple of 8)", rows, C);
  CASYNC_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0, "s3fd16 l2norm: 16-B alignment");
  CASYNC_REQUIRE(rows * C * 2 < kMaxBytes, "s3fd16 l2norm: 2 GiB or more");
  const int lpr = C <= 256 ? 32 : 64;
  unsigned grid;
  if (int st = grid_for(rows, 4 * (64 / lpr), &grid)) return st;
  return casync_launch(det16_l2norm_kernel, dim3(grid), dim3(256), 0, s, static_cast<const bf16_t*>(in), static_cast<bf16_t*>(out), rows, C,
                       lpr);
}

int launch_det16_head(const void* in, const float* wt, const float* bias, float* loc, float* conf, int batch, int h, int w, int C, int P,
                      int p0, bool maxout, hipStream_t s) {
  CASYNC_REQUIRE(in && wt && bias && loc && conf, "s3fd16 head: null pointer");
  CASYNC_REQUIRE(batch > 0 && h >= 1 && w >= 1 && C >= 8 && C % 8 == 0, "s3fd16 head: B=%d %dx%dx%d (C a multiple of 8)", batch, h, w, C);
  CASYNC_REQUIRE(p0 >= 0 && (long long)p0 + (long long)h * w <= P, "s3fd16 head: priors %d + %dx%d of %d", p0, h, w, P);
  CASYNC_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)wt % 16 == 0 && (uintptr_t)loc % 16 == 0 && (uintptr_t)conf % 8 == 0,
                 "s3fd16 head: alignment");
  CASYNC_REQUIRE((long long)batch * h * w * C * 2 < kMaxBytes && (long long)batch * P * 16 < kMaxBytes, "s3fd16 head: 2 GiB or more");
  const long long groups = (long long)batch * h * ((w + HPIX - 1) / HPIX);
  unsigned grid;
  if (int st = grid_for(groups, 4, &grid)) return st;
  return casync_launch(det16_head_kernel, dim3(grid), dim3(256), 0, s, static_cast<const bf16_t*>(in), wt, bias, loc, conf, groups, h, w, C,
                       P, p0, maxout ? 1 : 0);
}

// ---- C ABI: one entry per kernel (tests/kernel_ledger_det16.py) ------------------------------------------------------
extern "C" {

int casync_op_s3fd16_stem(const void* x, int input_u8, const float* w, const float* bias, void* out, int batch, int h, int w_,
                          casync_stream stream) {
  return launch_det16_stem(x, input_u8 != 0, w, bias, out, batch, h, w_, (hipStream_t)stream);
}
int casync_op_s3fd16_maxpool(const void* in, void* out, int batch, int h, int w_, int c, int ceil_mode, casync_stream stream) {
  return launch_det16_maxpool(in, out, batch, h, w_, c, ceil_mode != 0, (hipStream_t)stream);
}
int casync_op_s3fd16_im2col_dil(const void* in, void* out, int batch, int h, int w_, int c, int dilation, casync_stream stream) {
  return launch_det16_im2col_dil(in, out, batch, h, w_, c, dilation, (hipStream_t)stream);
}
int casync_op_s3fd16_relu(void* x, int64_t n, casync_stream stream) { return launch_det16_relu(x, n, (hipStream_t)stream); }
int casync_op_s3fd16_widen(const void* in, float* out, int64_t n, casync_stream stream) {
  return launch_det16_widen(in, out, n, (hipStream_t)stream);
}
int casync_op_s3fd16_l2norm(const void* in, void* out, int64_t rows, int c, casync_stream stream) {
  return launch_det16_l2norm(in, out, rows, c, (hipStream_t)stream);
}
int casync_op_s3fd16_head(const void* in, const float* w, const float* bias, float* loc, float* conf, int batch, int h, int w_, int c,
                          int priors, int first_prior, int maxout, casync_stream stream) {
  return launch_det16_head(in, w, bias, loc, conf, batch, h, w_, c, priors, first_prior, maxout != 0, (hipStream_t)stream);
}

}  // extern "C"
