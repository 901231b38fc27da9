// The trainer's loss and its gradient (include/casync_ploss.h): L1 + the VGG19 perceptual term of the reference's step
// (step2_train_unet.py:12-36,107-112), contentFunc = torchvision's vgg19().features up to and including index 14:
//   Conv(3,64) ReLU Conv(64,64) ReLU MaxPool Conv(64,128) ReLU Conv(128,128) ReLU MaxPool Conv(128,256) ReLU Conv(256,256) ReLU
//   Conv(256,256), every conv 3x3 pad 1 with bias, the pools 2x2 floor, no ReLU behind the last conv, no input normalisation.
// fp32, NHWC activations, gfx950.  The six convs behind the stem run on the ring implicit-GEMM kernel of lib/obj
// (launch_conv3x3_gemm): data-parallel tiles, no K split inside a launch, so image i has the same bits at any batch.  That
// kernel sums its K = 9 cin products in one fp32 chain, whose error grows with the square root of K: a conv of more than 64
// input channels (K = 2304 at 256) missed the handle's bar of 4x fp32 torch's error, the backward passes on signed dense gradients
// by a factor of 2.6.  Such a conv therefore runs as cin / 64 launches of K = 576 on channel slices (ploss_split_kernel) whose
// partial outputs ploss_combine_kernel sums as a tree with the bias and the ReLU; a conv of 64 input channels is one launch with
// the bias + ReLU epilogue as before.  The backward-data pass of a stride-1 pad-1 3x3 conv is the same conv on the taps flipped and the channel
// axes swapped: the six backward convs run on the same launcher on weights transformed once at load.  The VGG is frozen: no
// weight gradient is computed, no gradient reaches the label.
//
//   ploss_stem_kernel       conv1_1 (3 -> 64) + bias + ReLU from fp32 NCHW, one fmaf chain (ky, kx, ci) per output value.
//   ploss_pool_kernel       2x2 / 2 floor max pooling (an odd last row / column is dropped).
//   ploss_wflip_kernel      [cout][ky][kx][cin] -> [cin][2-ky][2-kx][cout]: the backward matrix of a ring conv.
//   ploss_split_kernel      [P][C] -> [C/64][P][64]: an activation (or a weight matrix, at load) cut into slices of 64 input channels.
//   ploss_combine_kernel    the partial outputs of the slices summed as a fixed tree, + bias, ReLU.
//   ploss_relu_bwd_kernel   g *= (a > 0) on the saved post-ReLU activation, in place.
//   ploss_pool_bwd_kernel   pool adjoint fused with the ReLU adjoint in front of it: of each window the first maximum in row-major
//                           order (torch's > rule) receives the gradient if it is positive; every other element, a dropped odd
//                           row / column included, is written as zero.
//   ploss_stem_bwd_kernel   conv1_1's backward-data pass with the pixel term folded in:
//                           grad_pred = s (perc_scale convT(g1) + pix_scale sign(pred - label)), s read from a device scalar.
//   ploss_sqdiff_kernel     d = F(pred) - F(label) stored, sum d^2 per workgroup (float64) into scratch.
//   ploss_absdiff_kernel    sum |pred - label| per workgroup (float64) into scratch.
//   ploss_finish_kernel     one workgroup: the partial sums in a fixed order -> losses[3] = {total, pixel, perceptual}.
// Every output element is written once by one lane; there is no global atomic; offsets are 64-bit; a tensor of 2 GiB or more is
// refused by name before a launch.
#include <string.h>

#include <mutex>
#include <string>

#include "../../include/casync_ploss.h"
#include "common.h"
#include "handle.h"

namespace {

constexpr int SC = 64;            // channels of conv1_1
constexpr int kMaxParts = 1024;   // workgroups of a reduction at the most: its partial sums in scratch
constexpr long long kMaxBytes = 1ll << 31;

// ------------------------------------------------------------------------------------------------ stem, forward
// x [B,3,H,W], w [(ky,kx,ci)=27][64], out [B,H,W,64]; 256 threads = 4 pixels x 64 channels
__global__ __launch_bounds__(256) void ploss_stem_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ out, long long pixels,
                                                         int H, int W) {
  const int c = threadIdx.x % SC;
  const long long p = (long long)blockIdx.x * 4 + threadIdx.x / SC;
  if (p >= pixels) return;
  const int px = (int)(p % W);
  const long long r = p / W;
  const int py = (int)(r % H);
  const long long b = r / H;
  float v = bias[c];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = py + ky - 1;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = px + kx - 1;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
#pragma unroll
      for (int ci = 0; ci < 3; ++ci) v = fmaf(w[((ky * 3 + kx) * 3 + ci) * SC + c], x[((b * 3 + ci) * H + iy) * W + ix], v);
    }
  }
  out[p * SC + c] = v > 0.f ? v : 0.f;
}

// ------------------------------------------------------------------------------------------------ max pooling, forward
// in [B,H,W,C] -> out [B,H/2,W/2,C]
__global__ __launch_bounds__(256) void ploss_pool_kernel(const float* __restrict__ in, float* __restrict__ out, long long total4, int H,
                                                         int W, int C4, int Ho, int Wo) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total4) return;
  const int c4 = (int)(idx % C4);
  long long r = idx / C4;
  const int ox = (int)(r % Wo);
  r /= Wo;
  const int oy = (int)(r % Ho);
  const long long b = r / Ho;
  const float* src = in + (((b * H + 2 * oy) * W + 2 * ox) * C4 + c4) * 4;
  const long long row = (long long)W * C4 * 4;
  f32x4 m = *reinterpret_cast<const f32x4*>(src);
  const f32x4 v01 = *reinterpret_cast<const f32x4*>(src + C4 * 4);
  const f32x4 v10 = *reinterpret_cast<const f32x4*>(src + row);
  const f32x4 v11 = *reinterpret_cast<const f32x4*>(src + row + C4 * 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    m[e] = v01[e] > m[e] ? v01[e] : m[e];
    m[e] = v10[e] > m[e] ? v10[e] : m[e];
    m[e] = v11[e] > m[e] ? v11[e] : m[e];
  }
  *reinterpret_cast<f32x4*>(out + idx * 4) = m;
}

// ------------------------------------------------------------------------------------------------ weight transform
// w [cout][t = ky*3+kx][cin] -> out [cin][8 - t][cout]; one thread per output element, cout fastest
__global__ __launch_bounds__(256) void ploss_wflip_kernel(const float* __restrict__ w, float* __restrict__ out, long long total, int cout,
                                                          int cin) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int co = (int)(idx % cout);
  long long r = idx / cout;
  const int t = (int)(r % 9);
  const long long ci = r / 9;
  out[idx] = w[((long long)co * 9 + (8 - t)) * cin + ci];
}

// ------------------------------------------------------------------------------------------------ channel slices
constexpr int SL = 64;   // input channels of one launch of a ring conv

// in [P][C] -> out [C / 64][P][64]; one thread per float4 of the output
__global__ __launch_bounds__(256) void ploss_split_kernel(const float* __restrict__ in, float* __restrict__ out, long long total4, long long P,
                                                          int C) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total4) return;
  const int j4 = (int)(idx % (SL / 4));
  long long r = idx / (SL / 4);
  const long long p = r % P;
  const long long g = r / P;
  *reinterpret_cast<f32x4*>(out + idx * 4) = *reinterpret_cast<const f32x4*>(in + p * C + g * SL + j4 * 4);
}

// part [G][n] (G = 2 or 4) -> out [n] = act(((p0 + p1) [+ (p2 + p3)]) + bias[column]); n4 float4, C4 float4 a row
__global__ __launch_bounds__(256) void ploss_combine_kernel(const float* __restrict__ part, int G, const float* __restrict__ bias,
                                                            float* __restrict__ out, long long n4, int C4, int relu) {
#pragma clang fp contract(off)
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n4) return;
  const long long n = n4 * 4;
  f32x4 v = *reinterpret_cast<const f32x4*>(part + idx * 4) + *reinterpret_cast<const f32x4*>(part + n + idx * 4);
  if (G == 4) v = v + (*reinterpret_cast<const f32x4*>(part + 2 * n + idx * 4) + *reinterpret_cast<const f32x4*>(part + 3 * n + idx * 4));
  if (bias) v = v + *reinterpret_cast<const f32x4*>(bias + (idx % C4) * 4);
  if (relu) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
  }
  *reinterpret_cast<f32x4*>(out + idx * 4) = v;
}

// ------------------------------------------------------------------------------------------------ ReLU adjoint
__global__ __launch_bounds__(256) void ploss_relu_bwd_kernel(float* __restrict__ g, const float* __restrict__ a, long long total4) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total4) return;
  f32x4 v = *reinterpret_cast<f32x4*>(g + idx * 4);
  const f32x4 m = *reinterpret_cast<const f32x4*>(a + idx * 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.f ? v[e] : 0.f;
  *reinterpret_cast<f32x4*>(g + idx * 4) = v;
}

// ------------------------------------------------------------------------------------------------ pool + ReLU adjoint
// gp [B,H/2,W/2,C], a [B,H,W,C] (post-ReLU, pre-pool) -> g [B,H,W,C].  One thread per window of the CEIL grid and four channels:
// a window the pool dropped (odd last row / column) only writes the zeros of its elements inside the image.
__global__ __launch_bounds__(256) void ploss_pool_bwd_kernel(const float* __restrict__ gp, const float* __restrict__ a,
                                                             float* __restrict__ g, long long total4, int H, int W, int C4, int Hc,
                                                             int Wc) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total4) return;
  const int c4 = (int)(idx % C4);
  long long r = idx / C4;
  const int ox = (int)(r % Wc);
  r /= Wc;
  const int oy = (int)(r % Hc);
  const long long b = r / Hc;
  const int Ho = H / 2, Wo = W / 2;
  const long long at = (((b * H + 2 * oy) * W + 2 * ox) * C4 + c4) * 4, row = (long long)W * C4 * 4;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  if (oy < Ho && ox < Wo) {
    const f32x4 a00 = *reinterpret_cast<const f32x4*>(a + at), a01 = *reinterpret_cast<const f32x4*>(a + at + C4 * 4);
    const f32x4 a10 = *reinterpret_cast<const f32x4*>(a + at + row), a11 = *reinterpret_cast<const f32x4*>(a + at + row + C4 * 4);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(gp + (((b * Ho + oy) * Wo + ox) * C4 + c4) * 4);
    f32x4 o00 = zero, o01 = zero, o10 = zero, o11 = zero;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int k = 0;
      float m = a00[e];
      if (a01[e] > m) m = a01[e], k = 1;
      if (a10[e] > m) m = a10[e], k = 2;
      if (a11[e] > m) m = a11[e], k = 3;
      const float v = m > 0.f ? gv[e] : 0.f;
      o00[e] = k == 0 ? v : 0.f;
      o01[e] = k == 1 ? v : 0.f;
      o10[e] = k == 2 ? v : 0.f;
      o11[e] = k == 3 ? v : 0.f;
    }
    *reinterpret_cast<f32x4*>(g + at) = o00;
    *reinterpret_cast<f32x4*>(g + at + C4 * 4) = o01;
    *reinterpret_cast<f32x4*>(g + at + row) = o10;
    *reinterpret_cast<f32x4*>(g + at + row + C4 * 4) = o11;
    return;
  }
  const bool right = 2 * ox + 1 < W, below = 2 * oy + 1 < H;   // (2 oy < H and 2 ox < W by the ceil grid)
  *reinterpret_cast<f32x4*>(g + at) = zero;
  if (right) *reinterpret_cast<f32x4*>(g + at + C4 * 4) = zero;
  if (below) *reinterpret_cast<f32x4*>(g + at + row) = zero;
  if (right && below) *reinterpret_cast<f32x4*>(g + at + row + C4 * 4) = zero;
}

// ------------------------------------------------------------------------------------------------ stem, backward
// g1 [B,H,W,64] (masked), w [(ky,kx,ci)=27][64] (the forward matrix: its 64 output channels are the contiguous axis this kernel
// sums over), pred / label / grad_pred [B,3,H,W].  16 lanes per pixel, each four of the 64 channels: a wave reads 1 KB of g1 in a
// row per tap.  Lane q's partial sums over (ky, kx) ascending, then a butterfly over the 16 lanes: a fixed order.
//   grad_pred = s * (perc_scale * sum + pix_scale * sign(pred - label)), sign(0) = 0, s = *grad_out
__global__ __launch_bounds__(256) void ploss_stem_bwd_kernel(const float* __restrict__ g1, const float* __restrict__ w,
                                                             const float* __restrict__ pred, const float* __restrict__ label,
                                                             const float* __restrict__ grad_out, float* __restrict__ grad_pred,
                                                             long long pixels, int H, int W, float perc_scale, float pix_scale) {
#pragma clang fp contract(off)
  const int q = threadIdx.x & 15;
  const long long p = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = p < pixels;           // (dead lanes keep step with the shuffles)
  const long long pp = live ? p : 0;
  const int px = (int)(pp % W);
  const long long r = pp / W;
  const int py = (int)(r % H);
  const long long b = r / H;
  float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = py - (ky - 1);
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = px - (kx - 1);
      if (!live || iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g1 + ((b * H + iy) * W + ix) * SC + q * 4);
#pragma unroll
      for (int ci = 0; ci < 3; ++ci) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + ((ky * 3 + kx) * 3 + ci) * SC + q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {   // the result pinned: keeps the compiler from packing two channels' FMAs around a gradient taken
          float t = __builtin_fmaf(wv[e], gv[e], acc[ci]);   // from the high half of a register pair (ir_common.h fma4_scalar)
          asm("" : "+v"(t));
          acc[ci] = t;
        }
      }
    }
  }
#pragma unroll
  for (int ci = 0; ci < 3; ++ci)
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) acc[ci] += __shfl_xor(acc[ci], o, 16);
  if (!live || q >= 3) return;
  const float sum = q == 0 ? acc[0] : q == 1 ? acc[1] : acc[2];
  const long long at = ((b * 3 + q) * H + py) * W + px;
  float v = perc_scale * sum;
  if (pred) {
    const float df = pred[at] - label[at];
    const float sg = df > 0.f ? 1.f : df < 0.f ? -1.f : 0.f;
    v = v + pix_scale * sg;
  }
  grad_pred[at] = grad_out[0] * v;
}

// ------------------------------------------------------------------------------------------------ reductions
// 256 doubles of a workgroup -> thread 0 holds their sum: a tree in a fixed order
__device__ __forceinline__ double block_sum(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) lds[threadIdx.x] += lds[threadIdx.x + o];
    __syncthreads();
  }
  return lds[0];
}

// d = fp - fl (n4 float4), part[blockIdx.x] = sum of d^2 over the items blockIdx.x * 256 + tid + k * gridDim.x * 256
__global__ __launch_bounds__(256) void ploss_sqdiff_kernel(const float* __restrict__ fp, const float* __restrict__ fl, float* __restrict__ d,
                                                           double* __restrict__ part, long long n4) {
  __shared__ double lds[256];
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(fp + i * 4), c = *reinterpret_cast<const f32x4*>(fl + i * 4);
    const f32x4 df = a - c;
    *reinterpret_cast<f32x4*>(d + i * 4) = df;
#pragma unroll
    for (int e = 0; e < 4; ++e) s += (double)df[e] * (double)df[e];
  }
  const double t = block_sum(s, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void ploss_absdiff_kernel(const float* __restrict__ pred, const float* __restrict__ label,
                                                            double* __restrict__ part, long long n) {
  __shared__ double lds[256];
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) s += (double)fabsf(pred[i] - label[i]);
  const double t = block_sum(s, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// losses = {w_pix * pixel + w_perc * perceptual, pixel, perceptual}: the means rounded to fp32 once, the total in fp32 as the
// reference's `loss_pixel + 0.1 * loss_perceptual` is.  n_abs == 0 (w_pix == 0): pixel = 0.
__global__ __launch_bounds__(256) void ploss_finish_kernel(const double* __restrict__ part_sq, int n_sq, double count_sq,
                                                           const double* __restrict__ part_abs, int n_abs, double count_abs, float w_pix,
                                                           float w_perc, float* __restrict__ losses) {
#pragma clang fp contract(off)
  __shared__ double lds[256];
  double s = 0.0, a = 0.0;
  for (int i = threadIdx.x; i < n_sq; i += 256) s += part_sq[i];
  for (int i = threadIdx.x; i < n_abs; i += 256) a += part_abs[i];
  const double ts = block_sum(s, lds);
  __syncthreads();
  const double ta = block_sum(a, lds);
  if (threadIdx.x != 0) return;
  const float perc = (float)(ts / count_sq), pix = n_abs > 0 ? (float)(ta / count_abs) : 0.f;
  const float wp = w_perc * perc;
  losses[0] = w_pix * pix + wp;
  losses[1] = pix;
  losses[2] = perc;
}

// ------------------------------------------------------------------------------------------------ launchers
int grid_for(long long items, int per_block, unsigned* grid) {
  const long long g = (items + per_block - 1) / per_block;
  CASYNC_REQUIRE(g >= 1 && g < (1ll << 31), "ploss: grid of %lld blocks", g);
  *grid = (unsigned)g;
  return CASYNC_OK;
}
bool al16(const void* p) { return (uintptr_t)p % 16 == 0; }
int parts_of(long long items) {   // workgroups of a reduction over `items` lane items: a function of the size alone
  const long long g = (items + 255) / 256;
  return (int)(g < 1 ? 1 : g > kMaxParts ? kMaxParts : g);
}

int launch_stem(const float* x, const float* w, const float* bias, float* out, int batch, int H, int W, hipStream_t s) {
  CASYNC_REQUIRE(x && w && bias && out, "ploss stem: null pointer");
  CASYNC_REQUIRE(batch > 0 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192, "ploss stem: B=%d %dx%d", batch, H, W);
  const long long pixels = (long long)batch * H * W;
  CASYNC_REQUIRE(pixels * SC * 4 < kMaxBytes, "ploss stem: output of %lld bytes (2 GiB or more)", pixels * SC * 4);
  unsigned grid;
  if (int st = grid_for(pixels, 4, &grid)) return st;
  return casync_launch(ploss_stem_kernel, dim3(grid), dim3(256), 0, s, x, w, bias, out, pixels, H, W);
}

int launch_pool(const float* in, float* out, int batch, int H, int W, int C, hipStream_t s) {
  CASYNC_REQUIRE(in && out && al16(in) && al16(out), "ploss pool: null or unaligned pointer");
  CASYNC_REQUIRE(batch > 0 && H >= 2 && W >= 2 && C >= 4 && C % 4 == 0, "ploss pool: B=%d %dx%dx%d (H, W >= 2, C a multiple of 4)", batch, H, W, C);
  CASYNC_REQUIRE((long long)batch * H * W * C * 4 < kMaxBytes, "ploss pool: input of 2 GiB or more");
  const long long total4 = (long long)batch * (H / 2) * (W / 2) * (C / 4);
  unsigned grid;
  if (int st = grid_for(total4, 256, &grid)) return st;
  return casync_launch(ploss_pool_kernel, dim3(grid), dim3(256), 0, s, in, out, total4, H, W, C / 4, H / 2, W / 2);
}

int launch_wflip(const float* w, float* out, int cout, int cin, hipStream_t s) {
  CASYNC_REQUIRE(w && out && w != out, "ploss weight transform: null pointer, or in place");
  CASYNC_REQUIRE(cout >= 1 && cin >= 1 && cout <= 65536 && cin <= 65536, "ploss weight transform: cout=%d cin=%d", cout, cin);
  const long long total = 9ll * cout * cin;
  CASYNC_REQUIRE(total * 4 < kMaxBytes, "ploss weight transform: matrix of 2 GiB or more");
  unsigned grid;
  if (int st = grid_for(total, 256, &grid)) return st;
  return casync_launch(ploss_wflip_kernel, dim3(grid), dim3(256), 0, s, w, out, total, cout, cin);
}

int launch_split(const float* in, float* out, long long P, int C, hipStream_t s) {
  CASYNC_REQUIRE(in && out && in != out && al16(in) && al16(out), "ploss split: null, unaligned or in-place pointer");
  CASYNC_REQUIRE(P >= 1 && C >= SL && C % SL == 0 && C <= 65536, "ploss split: %lld rows of %d (a multiple of %d)", P, C, SL);
  CASYNC_REQUIRE(P < (1ll << 31) && P * C * 4 < kMaxBytes, "ploss split: tensor of 2 GiB or more");
  const long long total4 = P * C / 4;
  unsigned grid;
  if (int st = grid_for(total4, 256, &grid)) return st;
  return casync_launch(ploss_split_kernel, dim3(grid), dim3(256), 0, s, in, out, total4, P, C);
}

int launch_combine(const float* part, int G, const float* bias, float* out, long long n, int C, bool relu, hipStream_t s) {
  CASYNC_REQUIRE(part && out && al16(part) && al16(out) && (!bias || al16(bias)), "ploss combine: null or unaligned pointer");
  CASYNC_REQUIRE(G == 2 || G == 4, "ploss combine: %d partial outputs (2 or 4)", G);
  CASYNC_REQUIRE(C >= 4 && C % 4 == 0 && n > 0 && n % C == 0 && (long long)G * n * 4 < kMaxBytes, "ploss combine: n=%lld C=%d (rows of C, C a multiple of 4, under 2 GiB)", n, C);
  unsigned grid;
  if (int st = grid_for(n / 4, 256, &grid)) return st;
  return casync_launch(ploss_combine_kernel, dim3(grid), dim3(256), 0, s, part, G, bias, out, n / 4, C / 4, relu ? 1 : 0);
}

int launch_relu_bwd(float* g, const float* a, long long n, hipStream_t s) {
  CASYNC_REQUIRE(g && a && al16(g) && al16(a) && n > 0 && n % 4 == 0, "ploss relu adjoint: n=%lld (a multiple of 4, 16-B aligned)", n);
  CASYNC_REQUIRE(n * 4 < kMaxBytes, "ploss relu adjoint: gradient of 2 GiB or more");
  unsigned grid;
  if (int st = grid_for(n / 4, 256, &grid)) return st;
  return casync_launch(ploss_relu_bwd_kernel, dim3(grid), dim3(256), 0, s, g, a, n / 4);
}

int launch_pool_bwd(const float* gp, const float* a, float* g, int batch, int H, int W, int C, hipStream_t s) {
  CASYNC_REQUIRE(gp && a && g && al16(gp) && al16(a) && al16(g), "ploss pool adjoint: null or unaligned pointer");
  CASYNC_REQUIRE(batch > 0 && H >= 2 && W >= 2 && C >= 4 && C % 4 == 0, "ploss pool adjoint: B=%d %dx%dx%d (H, W >= 2, C a multiple of 4)", batch, H, W,
                 C);
  CASYNC_REQUIRE((long long)batch * H * W * C * 4 < kMaxBytes, "ploss pool adjoint: gradient of 2 GiB or more");
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const long long total4 = (long long)batch * Hc * Wc * (C / 4);
  unsigned grid;
  if (int st = grid_for(total4, 256, &grid)) return st;
  return casync_launch(ploss_pool_bwd_kernel, dim3(grid), dim3(256), 0, s, gp, a, g, total4, H, W, C / 4, Hc, Wc);
}

int launch_stem_bwd(const float* g1, const float* w, const float* pred, const float* label, const float* grad_out, float* grad_pred,
                    int batch, int H, int W, float perc_scale, float pix_scale, hipStream_t s) {
  CASYNC_REQUIRE(g1 && w && grad_out && grad_pred && al16(g1) && al16(w), "ploss stem adjoint: null or unaligned pointer");
  CASYNC_REQUIRE((pred == nullptr) == (label == nullptr), "ploss stem adjoint: pred and label come together (both null: no pixel term)");
  CASYNC_REQUIRE(batch > 0 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192, "ploss stem adjoint: B=%d %dx%d", batch, H, W);
  const long long pixels = (long long)batch * H * W;
  CASYNC_REQUIRE(pixels * SC * 4 < kMaxBytes, "ploss stem adjoint: gradient of %lld bytes (2 GiB or more)", pixels * SC * 4);
  unsigned grid;
  if (int st = grid_for(pixels, 16, &grid)) return st;
  return casync_launch(ploss_stem_bwd_kernel, dim3(grid), dim3(256), 0, s, g1, w, pred, label, grad_out, grad_pred, pixels, H, W, perc_scale,
                       pix_scale);
}

int launch_sqdiff(const float* fp, const float* fl, float* d, long long n, double* part, hipStream_t s) {
  CASYNC_REQUIRE(fp && fl && d && part && al16(fp) && al16(fl) && al16(d) && (uintptr_t)part % 8 == 0, "ploss sqdiff: null or unaligned pointer");
  CASYNC_REQUIRE(n > 0 && n % 4 == 0 && n * 4 < kMaxBytes, "ploss sqdiff: n=%lld (a multiple of 4, under 2 GiB)", n);
  return casync_launch(ploss_sqdiff_kernel, dim3(parts_of(n / 4)), dim3(256), 0, s, fp, fl, d, part, n / 4);
}

int launch_absdiff(const float* pred, const float* label, long long n, double* part, hipStream_t s) {
  CASYNC_REQUIRE(pred && label && part && (uintptr_t)part % 8 == 0, "ploss absdiff: null or unaligned pointer");
  CASYNC_REQUIRE(n > 0 && n * 4 < kMaxBytes, "ploss absdiff: n=%lld (under 2 GiB)", n);
  return casync_launch(ploss_absdiff_kernel, dim3(parts_of(n)), dim3(256), 0, s, pred, label, part, n);
}

int launch_finish(const double* part_sq, int n_sq, long long count_sq, const double* part_abs, int n_abs, long long count_abs, float w_pix,
                  float w_perc, float* losses, hipStream_t s) {
  CASYNC_REQUIRE(part_sq && losses && n_sq >= 1 && n_sq <= kMaxParts && count_sq >= 1, "ploss finish: %d partial sums of %lld squares", n_sq, count_sq);
  CASYNC_REQUIRE(n_abs >= 0 && n_abs <= kMaxParts && (n_abs == 0 || (part_abs && count_abs >= 1)), "ploss finish: %d partial sums of %lld differences",
                 n_abs, count_abs);
  return casync_launch(ploss_finish_kernel, dim3(1), dim3(256), 0, s, part_sq, n_sq, (double)count_sq, part_abs, n_abs, (double)count_abs, w_pix,
                       w_perc, losses);
}

// ------------------------------------------------------------------------------------------------ network, packed layout
struct PConv {
  const char* name;
  int cin, cout;
  int relu;   // ReLU behind it
  int pool;   // floor pool behind that
};
const PConv kRing[6] = {{"conv1_2", 64, 64, 1, 1},   {"conv2_1", 64, 128, 1, 0},  {"conv2_2", 128, 128, 1, 1},
                        {"conv3_1", 128, 256, 1, 0}, {"conv3_2", 256, 256, 1, 0}, {"conv3_3", 256, 256, 0, 0}};
enum { FT_CONV1_1, FT_CONV1_2, FT_POOL1, FT_CONV2_1, FT_CONV2_2, FT_POOL2, FT_CONV3_1, FT_CONV3_2, FT_CONV3_3, FT_D, kFwdStages };
enum { kBwdStages = 13 };

struct PLayout {
  PackedLayout packed;
  int64_t stem_w, stem_b, w[6], b[6];
  int64_t wt[6], wt_total = 0;   // the transformed matrices, in a buffer of the handle's own
  PLayout() {
    stem_w = packed.add("conv1_1.w", 27 * SC), stem_b = packed.add("conv1_1.b", SC);
    for (int i = 0; i < 6; ++i) {
      const int64_t n = 9ll * kRing[i].cin * kRing[i].cout;
      w[i] = packed.add(std::string(kRing[i].name) + ".w", n), b[i] = packed.add(std::string(kRing[i].name) + ".b", kRing[i].cout);
      wt[i] = wt_total, wt_total += round64(n);
    }
  }
};
const PLayout& p_layout() {
  static const PLayout L;
  return L;
}

struct PGeom {
  int B, H, W, h2, w2, h3, w3;
  int64_t act;    // floats of the largest activation, [B,H,W,64]
  int64_t feat;   // floats of the features, [B,h3,w3,256]
  int64_t n_pix;
};
// CASYNC_ERR_ARG with the reason set, before anything runs
int p_geometry(const char* what, int batch, int H, int W, PGeom* G) {
  CASYNC_REQUIRE(batch >= 1 && batch <= 65536, "%s: batch %d (1..65536)", what, batch);
  CASYNC_REQUIRE(H >= 4 && W >= 4 && H <= 8192 && W <= 8192, "%s: images of %d x %d (4 x 4 at least, 8192 at the most)", what, H, W);
  G->B = batch, G->H = H, G->W = W, G->h2 = H / 2, G->w2 = W / 2, G->h3 = G->h2 / 2, G->w3 = G->w2 / 2;
  G->act = (int64_t)batch * H * W * SC;
  G->feat = (int64_t)batch * G->h3 * G->w3 * 256;
  G->n_pix = (int64_t)batch * 3 * H * W;
  CASYNC_REQUIRE(G->act * 4 < kMaxBytes, "%s: conv1's activation of a batch of %d images of %d x %d has %lld bytes (2 GiB or more)", what, batch, H, W,
                 (long long)G->act * 4);
  return CASYNC_OK;
}

int64_t up256(int64_t bytes) { return (bytes + 255) / 256 * 256; }

// `saved`: what backward reads of the prediction's forward
struct PSaved {
  float *a11, *a12, *a21, *a22, *a31, *a32, *d;
  int64_t bytes;
  PSaved(void* base, const PGeom& G) {
    int64_t off = 0;
    auto take = [&](int64_t floats) {
      float* p = base ? reinterpret_cast<float*>(static_cast<char*>(base) + off) : nullptr;
      off += up256(floats * 4);
      return p;
    };
    const int64_t s2 = (int64_t)G.B * G.h2 * G.w2 * 128;
    a11 = take(G.act), a12 = take(G.act), a21 = take(s2), a22 = take(s2), a31 = take(G.feat), a32 = take(G.feat), d = take(G.feat);
    bytes = off;
  }
};
// `scratch`: two activations, two feature tensors, the channel slices of a conv's input (at most [B,H/2,W/2,128]) and the partial
// outputs of its launches (at most 4 [B,H/4,W/4,256]), and the partial sums of the two reductions
struct PScratch {
  float *a, *b, *fp, *fl, *sp, *pt;
  double *part_sq, *part_abs;
  int64_t bytes;
  PScratch(void* base, const PGeom& G) {
    int64_t off = 0;
    auto take = [&](int64_t n_bytes) {
      char* p = base ? static_cast<char*>(base) + off : nullptr;
      off += up256(n_bytes);
      return p;
    };
    a = reinterpret_cast<float*>(take(G.act * 4)), b = reinterpret_cast<float*>(take(G.act * 4));
    fp = reinterpret_cast<float*>(take(G.feat * 4)), fl = reinterpret_cast<float*>(take(G.feat * 4));
    sp = reinterpret_cast<float*>(take(G.act * 2)), pt = reinterpret_cast<float*>(take(G.act * 4));
    part_sq = reinterpret_cast<double*>(take(kMaxParts * 8)), part_abs = reinterpret_cast<double*>(take(kMaxParts * 8));
    bytes = off;
  }
};

}  // namespace

struct casync_ploss {
  int device = 0;
  PackedWeights pw;
  float* wt = nullptr;           // three images of the six matrices, each p_layout().wt_total floats (ploss_wflip_kernel, ploss_split_kernel at
                                 // load): the backward matrices, the forward matrices in channel slices, the backward matrices in slices
  hipEvent_t ev_fwd = nullptr;   // forward gate slot
};

namespace {
#define PL(call)                        \
  do {                                  \
    if (int st__ = (call)) return st__; \
  } while (0)

int copy_out(const float* src, float* out, int64_t n, hipStream_t s) {
  CASYNC_CHECK_HIP(hipMemcpyAsync(out, src, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  return CASYNC_OK;
}

int64_t fwd_stage_floats(const PGeom& G, int stage) {   // of G.B images
  const int64_t s2 = (int64_t)G.B * G.h2 * G.w2;
  switch (stage) {
    case FT_CONV1_1: case FT_CONV1_2: return G.act;
    case FT_POOL1: return s2 * 64;
    case FT_CONV2_1: case FT_CONV2_2: return s2 * 128;
    case FT_POOL2: return G.feat / 2;
  }
  return G.feat;
}

// One ring conv, forward or backward-data: in [nb,h,wd,cin] -> out [nb,h,wd,cout].  w: the whole matrix [cout][9][cin], w_sl: the
// same in slices [cin / 64][cout][9][64].  bias may be null.
int ring_conv(const float* in, const float* w, const float* w_sl, const float* bias, bool relu, float* out, int nb, int h, int wd, int cin,
              int cout, const PScratch& ws, hipStream_t s) {
  GemmEpilogue epi;
  const int G = cin / SL;
  if (G == 1) {
    epi.bias = bias;
    epi.act = relu ? 2 : 0;
    return launch_conv3x3_gemm(in, w, out, cout, nb, h, wd, cin, cout, 1, 1, 1, epi, s);
  }
  const long long pixels = (long long)nb * h * wd;
  PL(launch_split(in, ws.sp, pixels, cin, s));
  for (int g = 0; g < G; ++g)
    PL(launch_conv3x3_gemm(ws.sp + g * pixels * SL, w_sl + (long long)g * cout * 9 * SL, ws.pt + g * pixels * cout, cout, nb, h, wd, SL, cout, 1, 1, 1,
                           epi, s));
  return launch_combine(ws.pt, G, bias, out, pixels * cout, cout, relu, s);
}

// One pass of G.B images through the seven convs; dst[k] receives stage k (FT_CONV1_1 .. FT_CONV3_3).  Returns behind `stage`
// with that tensor copied to tap_out where stage >= 0.
int fwd_pass(const casync_ploss* P, const float* x, const PGeom& G, const PScratch& ws, float* const dst[9], int stage, float* tap_out,
             hipStream_t s) {
  const PLayout& L = p_layout();
  const float* w = P->pw.w;
  PL(launch_stem(x, w + L.stem_w, w + L.stem_b, dst[FT_CONV1_1], G.B, G.H, G.W, s));
  if (stage == FT_CONV1_1) return copy_out(dst[FT_CONV1_1], tap_out, fwd_stage_floats(G, stage), s);
  int h = G.H, wd = G.W, k = FT_CONV1_1;
  for (int i = 0; i < 6; ++i) {
    const PConv& c = kRing[i];
    PL(ring_conv(dst[k], w + L.w[i], P->wt + L.wt_total + L.wt[i], w + L.b[i], c.relu != 0, dst[k + 1], G.B, h, wd, c.cin, c.cout, ws, s));
    ++k;
    if (stage == k) return copy_out(dst[k], tap_out, fwd_stage_floats(G, stage), s);
    if (c.pool) {
      PL(launch_pool(dst[k], dst[k + 1], G.B, h, wd, c.cout, s));
      ++k, h /= 2, wd /= 2;
      if (stage == k) return copy_out(dst[k], tap_out, fwd_stage_floats(G, stage), s);
    }
  }
  return CASYNC_OK;
}

struct FwdArgs {
  const float *pred, *label;
  float w_pix, w_perc;
  float* losses;
  void *saved, *scratch;
  int64_t saved_bytes, scratch_bytes;
  int stage;        // -1: the forward; else the tap
  float* tap_out;
};

int check_scratch(const char* what, const PScratch& ws, void* scratch, int64_t scratch_bytes) {
  CASYNC_REQUIRE(scratch && (uintptr_t)scratch % 256 == 0, "%s: scratch is null or not 256-B aligned", what);
  if (scratch_bytes < ws.bytes) {
    casync_set_error("%s: scratch of %lld bytes, needs %lld", what, (long long)scratch_bytes, (long long)ws.bytes);
    return CASYNC_ERR_STATE;
  }
  return CASYNC_OK;
}

int run_forward(casync_ploss* P, int batch, int H, int W, const FwdArgs& a, hipStream_t s) {
  const char* what = a.stage < 0 ? "ploss forward" : "ploss forward_tap";
  CASYNC_REQUIRE(P, "%s: null handle", what);
  CASYNC_REQUIRE(P->pw.w && P->wt, "%s: weights not loaded", what);
  PGeom G;
  PL(p_geometry(what, batch, H, W, &G));
  CASYNC_REQUIRE(a.pred && a.label && (uintptr_t)a.pred % 4 == 0 && (uintptr_t)a.label % 4 == 0, "%s: pred / label null or unaligned", what);
  CASYNC_REQUIRE(a.stage < kFwdStages, "%s: stage %d (0..%d)", what, a.stage, kFwdStages - 1);
  CASYNC_REQUIRE(a.stage < 0 ? a.losses != nullptr : (a.tap_out != nullptr && al16(a.tap_out)), "%s: null output", what);
  const PScratch ws(a.scratch, G);
  PL(check_scratch(what, ws, a.scratch, a.scratch_bytes));
  const PSaved sv(a.saved, G);
  if (a.saved) {
    CASYNC_REQUIRE((uintptr_t)a.saved % 256 == 0, "%s: saved is not 256-B aligned", what);
    if (a.saved_bytes < sv.bytes) {
      casync_set_error("%s: saved of %lld bytes, needs %lld", what, (long long)a.saved_bytes, (long long)sv.bytes);
      return CASYNC_ERR_STATE;
    }
  }
  DeviceGuard guard(P->device);
  CASYNC_CHECK_HIP(guard.err);
  std::unique_lock<std::mutex> gate_lock;   // held until this forward is enqueued
  PL(casync_gate_enter(P->device, P, &P->ev_fwd, s, &gate_lock));
  // the label first, through the two scratch activations; then the prediction, into `saved` where there is one
  float* const lab[9] = {ws.a, ws.b, ws.a, ws.b, ws.a, ws.b, ws.a, ws.b, ws.fl};
  float* const prd_ws[9] = {ws.a, ws.b, ws.a, ws.b, ws.a, ws.b, ws.a, ws.b, ws.fp};
  float* const prd_sv[9] = {sv.a11, sv.a12, ws.a, sv.a21, sv.a22, ws.a, sv.a31, sv.a32, ws.fp};
  const bool tap_f = a.stage >= 0 && a.stage <= FT_CONV3_3;   // [2B, ...]: the prediction's images, then the label's
  PL(fwd_pass(P, a.label, G, ws, lab, tap_f ? a.stage : -1, tap_f ? a.tap_out + fwd_stage_floats(G, a.stage) : nullptr, s));
  PL(fwd_pass(P, a.pred, G, ws, a.saved ? prd_sv : prd_ws, tap_f ? a.stage : -1, a.tap_out, s));
  if (tap_f) return CASYNC_OK;
  float* d = a.stage == FT_D ? a.tap_out : a.saved ? sv.d : ws.a;
  PL(launch_sqdiff(ws.fp, ws.fl, d, G.feat, ws.part_sq, s));
  if (a.stage == FT_D) return CASYNC_OK;
  const bool pix = a.w_pix != 0.f;
  if (pix) PL(launch_absdiff(a.pred, a.label, G.n_pix, ws.part_abs, s));
  return launch_finish(ws.part_sq, parts_of(G.feat / 4), G.feat, ws.part_abs, pix ? parts_of(G.n_pix) : 0, G.n_pix, a.w_pix, a.w_perc, a.losses, s);
}

struct BwdArgs {
  const float *pred, *label, *grad_out;
  float* grad_pred;
  float w_pix, w_perc;
  const void* saved;
  void* scratch;
  int64_t saved_bytes, scratch_bytes;
  int stage;   // -1: the backward; else the tap
  float* tap_out;
};

int64_t bwd_stage_floats(const PGeom& G, int stage) {
  const int64_t s2 = (int64_t)G.B * G.h2 * G.w2;
  if (stage <= 3) return G.feat;
  if (stage == 4) return G.feat / 2;
  if (stage <= 7) return s2 * 128;
  if (stage == 8) return s2 * 64;
  if (stage <= 11) return G.act;
  return G.n_pix;
}

int run_backward(casync_ploss* P, int batch, int H, int W, const BwdArgs& a, hipStream_t s) {
  const char* what = a.stage < 0 ? "ploss backward" : "ploss backward_tap";
  CASYNC_REQUIRE(P, "%s: null handle", what);
  CASYNC_REQUIRE(P->pw.w && P->wt, "%s: weights not loaded", what);
  PGeom G;
  PL(p_geometry(what, batch, H, W, &G));
  const bool pix = a.w_pix != 0.f;
  CASYNC_REQUIRE(a.grad_out && (uintptr_t)a.grad_out % 4 == 0, "%s: grad_out null or unaligned", what);
  CASYNC_REQUIRE(!pix || (a.pred && a.label && (uintptr_t)a.pred % 4 == 0 && (uintptr_t)a.label % 4 == 0), "%s: pred / label null or unaligned", what);
  CASYNC_REQUIRE(a.stage < kBwdStages, "%s: stage %d (0..%d)", what, a.stage, kBwdStages - 1);
  float* out = a.stage < 0 ? a.grad_pred : a.tap_out;
  CASYNC_REQUIRE(out && (uintptr_t)out % (a.stage < 0 || a.stage == kBwdStages - 1 ? 4 : 16) == 0, "%s: null or unaligned output", what);
  const PScratch ws(a.scratch, G);
  PL(check_scratch(what, ws, a.scratch, a.scratch_bytes));
  const PSaved sv(const_cast<void*>(a.saved), G);
  CASYNC_REQUIRE(a.saved && (uintptr_t)a.saved % 256 == 0, "%s: saved is null or not 256-B aligned", what);
  if (a.saved_bytes < sv.bytes) {
    casync_set_error("%s: saved of %lld bytes, needs %lld", what, (long long)a.saved_bytes, (long long)sv.bytes);
    return CASYNC_ERR_STATE;
  }
  DeviceGuard guard(P->device);
  CASYNC_CHECK_HIP(guard.err);
  std::unique_lock<std::mutex> gate_lock;
  PL(casync_gate_enter(P->device, P, &P->ev_fwd, s, &gate_lock));
  const PLayout& L = p_layout();
  // what each ring conv's adjoint is followed by: the ReLU mask on the saved activation in front of that conv, or the pool
  // adjoint (with its ReLU mask) on the saved pre-pool activation
  const float* mask_of[6] = {sv.a11, nullptr, sv.a21, nullptr, sv.a31, sv.a32};   // by ring conv index
  const float* pool_of[6] = {nullptr, sv.a12, nullptr, sv.a22, nullptr, nullptr};
  const int hs[6] = {G.H, G.h2, G.h2, G.h3, G.h3, G.h3}, wds[6] = {G.W, G.w2, G.w2, G.w3, G.w3, G.w3};
  const float* cur = sv.d;
  float *nxt = ws.a, *other = ws.b;
  int k = 0;   // the stage the next launch completes
  auto done = [&](const float* t) -> int { return copy_out(t, a.tap_out, bwd_stage_floats(G, a.stage), s); };
  for (int i = 5; i >= 0; --i) {
    const PConv& c = kRing[i];
    PL(ring_conv(cur, P->wt + L.wt[i], P->wt + 2 * L.wt_total + L.wt[i], nullptr, false, nxt, G.B, hs[i], wds[i], c.cout, c.cin, ws, s));
    cur = nxt, std::swap(nxt, other);
    if (a.stage == k++) return done(cur);
    if (mask_of[i]) {
      PL(launch_relu_bwd(const_cast<float*>(cur), mask_of[i], (long long)G.B * hs[i] * wds[i] * c.cin, s));
    } else {   // the conv's input is a pool's output: hs[i] x wds[i] is the pooled size, the saved activation twice that (or one more)
      const int ph = i == 1 ? G.H : G.h2, pwd = i == 1 ? G.W : G.w2;
      PL(launch_pool_bwd(cur, pool_of[i], nxt, G.B, ph, pwd, c.cin, s));
      cur = nxt, std::swap(nxt, other);
    }
    if (a.stage == k++) return done(cur);
  }
  const double n_feat = (double)G.feat;
  const float perc_scale = (float)((double)a.w_perc * 2.0 / n_feat), pix_scale = (float)((double)a.w_pix / (double)G.n_pix);
  return launch_stem_bwd(cur, P->pw.w + L.stem_w, pix ? a.pred : nullptr, pix ? a.label : nullptr, a.grad_out, out, G.B, G.H, G.W, perc_scale,
                         pix_scale, s);
}

// the six backward matrices, at weight load (not on the forward path)
int refresh_wt(casync_ploss* P) {
  const PLayout& L = p_layout();
  DeviceGuard guard(P->device);
  CASYNC_CHECK_HIP(guard.err);
  if (!P->wt) CASYNC_CHECK_HIP(hipMalloc((void**)&P->wt, 3 * L.wt_total * sizeof(float)));
  for (int i = 0; i < 6; ++i) {
    const PConv& c = kRing[i];
    PL(launch_wflip(P->pw.w + L.w[i], P->wt + L.wt[i], c.cout, c.cin, 0));
    if (c.cin > SL) PL(launch_split(P->pw.w + L.w[i], P->wt + L.wt_total + L.wt[i], 9ll * c.cout, c.cin, 0));           // forward: slices of cin
    if (c.cout > SL) PL(launch_split(P->wt + L.wt[i], P->wt + 2 * L.wt_total + L.wt[i], 9ll * c.cin, c.cout, 0));       // backward: slices of cout
  }
  CASYNC_CHECK_HIP(hipDeviceSynchronize());
  return CASYNC_OK;
}
#undef PL
}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

int casync_ploss_packed_count(void) { return p_layout().packed.count(); }
const char* casync_ploss_packed_name(int i) { return p_layout().packed.name(i); }
int64_t casync_ploss_packed_offset(int i) { return p_layout().packed.offset(i); }
int64_t casync_ploss_packed_size(int i) { return p_layout().packed.size(i); }
int64_t casync_ploss_packed_total(void) { return p_layout().packed.total; }

int64_t casync_ploss_saved_bytes(int batch, int H, int W) {
  PGeom G;
  if (p_geometry("ploss saved_bytes", batch, H, W, &G)) return 0;
  return PSaved(nullptr, G).bytes;
}
int64_t casync_ploss_scratch_bytes(int batch, int H, int W) {
  PGeom G;
  if (p_geometry("ploss scratch_bytes", batch, H, W, &G)) return 0;
  return PScratch(nullptr, G).bytes;
}
int64_t casync_ploss_tap_floats(int backward, int batch, int H, int W, int stage) {
  PGeom G;
  if (p_geometry("ploss tap_floats", batch, H, W, &G) || stage < 0 || stage >= (backward ? (int)kBwdStages : (int)kFwdStages)) return 0;
  if (backward) return bwd_stage_floats(G, stage);
  return stage <= FT_CONV3_3 ? 2 * fwd_stage_floats(G, stage) : fwd_stage_floats(G, stage);
}
int casync_ploss_partials(int64_t items) { return items < 1 ? 0 : parts_of(items); }

int casync_ploss_create(int device_id, casync_ploss_handle* out) {
  CASYNC_REQUIRE(out, "ploss_create: null out");
  *out = nullptr;
  if (int st = casync_require_gfx950("ploss_create", device_id)) return st;
  casync_ploss* h = new casync_ploss();
  h->device = device_id;
  *out = h;
  return CASYNC_OK;
}

void casync_ploss_destroy(casync_ploss_handle h) {
  if (!h) return;
  DeviceGuard guard(h->device);
  casync_gate_forget(h->device, h, &h->ev_fwd);
  if (h->wt) (void)hipFree(h->wt);
  h->pw.release();
  delete h;
}

int casync_ploss_load_weights_host(casync_ploss_handle h, const float* packed, int64_t n_floats) {
  CASYNC_REQUIRE(h, "ploss_load_weights: null");
  if (int st = h->pw.load_host("ploss_load_weights", h->device, packed, n_floats, p_layout().packed.total, false)) return st;
  return refresh_wt(h);
}

int casync_ploss_load_weights_device(casync_ploss_handle h, const float* packed_dev, int64_t n_floats) {
  CASYNC_REQUIRE(h, "ploss_load_weights_device: null");
  if (int st = h->pw.adopt_device("ploss_load_weights_device", h->device, packed_dev, n_floats, p_layout().packed.total, false)) return st;
  return refresh_wt(h);
}

int casync_ploss_forward(casync_ploss_handle h, const float* pred, const float* label, int batch, int H, int W, float w_pix, float w_perc,
                         float* losses_dev, void* saved, int64_t saved_bytes, void* scratch, int64_t scratch_bytes, casync_stream stream) {
  const FwdArgs a{pred, label, w_pix, w_perc, losses_dev, saved, scratch, saved_bytes, scratch_bytes, -1, nullptr};
  return run_forward(h, batch, H, W, a, (hipStream_t)stream);
}

int casync_ploss_forward_tap(casync_ploss_handle h, const float* pred, const float* label, int batch, int H, int W, int stage, float* out,
                             void* scratch, int64_t scratch_bytes, casync_stream stream) {
  CASYNC_REQUIRE(stage >= 0, "ploss forward_tap: stage %d", stage);
  const FwdArgs a{pred, label, 0.f, 0.f, nullptr, nullptr, scratch, 0, scratch_bytes, stage, out};
  return run_forward(h, batch, H, W, a, (hipStream_t)stream);
}

int casync_ploss_backward(casync_ploss_handle h, const float* pred, const float* label, const float* grad_out_dev, float* grad_pred, int batch,
                          int H, int W, float w_pix, float w_perc, const void* saved, int64_t saved_bytes, void* scratch, int64_t scratch_bytes,
                          casync_stream stream) {
  const BwdArgs a{pred, label, grad_out_dev, grad_pred, w_pix, w_perc, saved, scratch, saved_bytes, scratch_bytes, -1, nullptr};
  return run_backward(h, batch, H, W, a, (hipStream_t)stream);
}

int casync_ploss_backward_tap(casync_ploss_handle h, const float* pred, const float* label, const float* grad_out_dev, int batch, int H, int W,
                              float w_pix, float w_perc, const void* saved, int64_t saved_bytes, int stage, float* out, void* scratch,
                              int64_t scratch_bytes, casync_stream stream) {
  CASYNC_REQUIRE(stage >= 0, "ploss backward_tap: stage %d", stage);
  const BwdArgs a{pred, label, grad_out_dev, nullptr, w_pix, w_perc, saved, scratch, saved_bytes, scratch_bytes, stage, out};
  return run_backward(h, batch, H, W, a, (hipStream_t)stream);
}

int casync_op_ploss_stem(const float* x, const float* w, const float* bias, float* out, int batch, int H, int W, casync_stream stream) {
  return launch_stem(x, w, bias, out, batch, H, W, (hipStream_t)stream);
}
int casync_op_ploss_pool(const float* in, float* out, int batch, int H, int W, int C, casync_stream stream) {
  return launch_pool(in, out, batch, H, W, C, (hipStream_t)stream);
}
int casync_op_ploss_weight_transform(const float* w, float* out, int cout, int cin, casync_stream stream) {
  return launch_wflip(w, out, cout, cin, (hipStream_t)stream);
}
int casync_op_ploss_split(const float* in, float* out, int64_t rows, int c, casync_stream stream) {
  return launch_split(in, out, rows, c, (hipStream_t)stream);
}
int casync_op_ploss_combine(const float* partials, int g, const float* bias, float* out, int64_t n, int c, int relu, casync_stream stream) {
  return launch_combine(partials, g, bias, out, n, c, relu != 0, (hipStream_t)stream);
}
int casync_op_ploss_relu_bwd(float* g, const float* a, int64_t n, casync_stream stream) { return launch_relu_bwd(g, a, n, (hipStream_t)stream); }
int casync_op_ploss_pool_bwd(const float* g_pool, const float* a, float* g, int batch, int H, int W, int C, casync_stream stream) {
  return launch_pool_bwd(g_pool, a, g, batch, H, W, C, (hipStream_t)stream);
}
int casync_op_ploss_stem_bwd(const float* g1, const float* w, const float* pred, const float* label, const float* grad_out_dev, float* grad_pred,
                             int batch, int H, int W, float perc_scale, float pix_scale, casync_stream stream) {
  return launch_stem_bwd(g1, w, pred, label, grad_out_dev, grad_pred, batch, H, W, perc_scale, pix_scale, (hipStream_t)stream);
}
int casync_op_ploss_sqdiff(const float* fp, const float* fl, float* d, int64_t n, double* partials, casync_stream stream) {
  return launch_sqdiff(fp, fl, d, n, partials, (hipStream_t)stream);
}
int casync_op_ploss_absdiff(const float* pred, const float* label, int64_t n, double* partials, casync_stream stream) {
  return launch_absdiff(pred, label, n, partials, (hipStream_t)stream);
}
int casync_op_ploss_finish(const double* partials_sq, int n_sq, int64_t count_sq, const double* partials_abs, int n_abs, int64_t count_abs,
                           float w_pix, float w_perc, float* losses_dev, casync_stream stream) {
  return launch_finish(partials_sq, n_sq, count_sq, partials_abs, n_abs, count_abs, w_pix, w_perc, losses_dev, (hipStream_t)stream);
}

}  // extern "C"
