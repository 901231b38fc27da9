// SyncNet_color of the reference (module/syncnet.py:155-246), the lip-sync judge: a face encoder (17 blocks) and an audio encoder
// (14 blocks) of conv(bias) -> BatchNorm(eval) -> (+ x) -> ReLU, both ending in [B,512,3,3]; then view(B,-1) of the NCHW tensor,
// x / max(|x|_2, 1e-12), LeakyReLU(0.01).  BatchNorm is folded into the convs on the host.  fp32, NHWC, gfx950.
//
//   sync_stem7_kernel    face.0: 7x7, pad 3, 3 -> 32, + bias, ReLU, from float NCHW; a 16 x 16 output tile per workgroup, its input
//                        with the 3-pixel halo and the 147 x 32 weights in LDS, 16-byte stores.
//   sync_conv_kernel<KS> face.1 (KS 5: stride 2, pad 1, 32 -> 64) and the 27 3x3 blocks (KS 3: stride 1, 2, (1,2); pad 0, 1, 2;
//                        cin 32 .. 512, cout 64 .. 512), + bias (+ x, added before the ReLU), ReLU as an implicit GEMM on
//                        v_mfma_f32_32x32x2_f32: 64 output pixels x 64 channels per workgroup, each tap of a pixel a contiguous run
//                        of the NHWC input (zero outside the image); no im2col buffer.  K is summed in chunks of 32 (see the kernel).
//   sync_relu_kernel     ReLU in place behind the two 1x1 blocks (the ring GEMM instances they run on have no ReLU epilogue).
//   sync_to_nchw_kernel  a block's NHWC output in the reference's NCHW order (casync_sync_forward_tap).
//   sync_embed_kernel    [B,3,3,512] -> [B,4608] at c * 9 + y * 3 + x, normalised and LeakyReLU'd; one workgroup per frame, the norm
//                        summed in float64 by a fixed-order wave / LDS reduction.
//   sync_curve_kernel    sim[s + S, i] = cos(face_i, audio_(i+s)) in F.cosine_similarity's form, one wave per pair, sums in float64.
// The 3x3 blocks do not run on the ring implicit-GEMM kernel (launch_conv3x3_gemm): its single fma chain over K = 9 cin put the
// audio encoder at 4.1 .. 4.7 times the reference's own float32 error, above the bar of 4 this handle is held to (measured; DESIGN
// section 8k).  The two 1x1 blocks (K = 512) run on the data-parallel ring GEMM (launch_rows_gemm), the audio window goes to NHWC
// with launch_nchw_to_nhwc: no stream-K, no K split.  No kernel here sums across frames or uses an atomic: frame i of a batch has
// the bits of that frame forwarded alone.
// The block table, the handle and what the bf16 precision of this handle (syncnet_bf16.hip) calls of this file are declared in
// syncnet_common.h; a handle of precision 1 takes sync_run's checks and gate and then that file's pass.
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "syncnet_common.h"

namespace {

__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : 0.f; }

// ------------------------------------------------------------------------------------------------ stem (7x7)
constexpr int S7_T = 16;            // output tile
constexpr int S7_IN = S7_T + 6;     // with the halo
constexpr int S7_LD = S7_IN + 1;    // LDS row stride (odd)
constexpr int S7_C = 32, S7_K = 147;

// x [B,3,H,W], w [(ky,kx,ci)=147][32], out [B,H,W,32]; one thread per output pixel of the tile, all 32 channels
__global__ __launch_bounds__(256) void sync_stem7_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ out, int H, int W, int tiles_x,
                                                         int tiles_y) {
  __shared__ float xs[3][S7_IN][S7_LD];
  __shared__ __attribute__((aligned(16))) float ws[S7_K * S7_C];
  const int tid = threadIdx.x;
  long long t = blockIdx.x;
  const int tx = (int)(t % tiles_x);
  t /= tiles_x;
  const int ty = (int)(t % tiles_y);
  const long long b = t / tiles_y;
  const int x0 = tx * S7_T, y0 = ty * S7_T;
  for (int i = tid; i < S7_K * S7_C / 4; i += 256) reinterpret_cast<f32x4*>(ws)[i] = reinterpret_cast<const f32x4*>(w)[i];
  for (int i = tid; i < 3 * S7_IN * S7_IN; i += 256) {
    const int ci = i / (S7_IN * S7_IN), r = i - ci * (S7_IN * S7_IN), ly = r / S7_IN, lx = r - ly * S7_IN;
    const int iy = y0 + ly - 3, ix = x0 + lx - 3;
    float v = 0.f;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = x[((b * 3 + ci) * H + iy) * (long long)W + ix];
    xs[ci][ly][lx] = v;
  }
  __syncthreads();
  const int px = tid & (S7_T - 1), py = tid / S7_T;
  float acc[S7_C];
#pragma unroll
  for (int c = 0; c < S7_C; ++c) acc[c] = bias[c];
#pragma unroll 1
  for (int ky = 0; ky < 7; ++ky) {
#pragma unroll 1
    for (int kx = 0; kx < 7; ++kx) {
#pragma unroll
      for (int ci = 0; ci < 3; ++ci) {
        const float in = xs[ci][py + ky][px + kx];
        const float* wr = ws + ((ky * 7 + kx) * 3 + ci) * S7_C;
#pragma unroll
        for (int c4 = 0; c4 < S7_C / 4; ++c4) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + c4 * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {   // the result pinned: no packed FMA around a scalar from the high half of a register pair
            float a = fmaf(wv[e], in, acc[c4 * 4 + e]);   // (ir_common.h fma4_scalar)
            asm("" : "+v"(a));
            acc[c4 * 4 + e] = a;
          }
        }
      }
    }
  }
  const int oy = y0 + py, ox = x0 + px;
  if (oy >= H || ox >= W) return;
  float* o = out + ((b * H + oy) * (long long)W + ox) * S7_C;
#pragma unroll
  for (int c4 = 0; c4 < S7_C / 4; ++c4)
    *reinterpret_cast<f32x4*>(o + c4 * 4) = f32x4{relu(acc[c4 * 4]), relu(acc[c4 * 4 + 1]), relu(acc[c4 * 4 + 2]), relu(acc[c4 * 4 + 3])};
}

// ------------------------------------------------------------------------------------------------ dense KS x KS conv
constexpr int CV_BM = 64, CV_BN = 64, CV_BK = 32, CV_LD = 36;

// in [B,H,W,cin], w [cout][(ky,kx,cin)], res (optional) and out [M = B Ho Wo][cout]: out = relu(conv + bias (+ res)).  A 64 x 64
// tile per workgroup, four waves of a 32 x 32 quarter each; per k-chunk (one tap, 32 channels: a contiguous 128 bytes of a pixel,
// zero outside the image) the 64 input rows and the 64 weight rows go through LDS (row stride 36 floats: conflict-free b128
// reads), a lane half kh taking k = 8 g + 4 kh .. + 3 of every group of 8 for both operands.  Each chunk is summed from zero
// (a 32-step fma chain on the matrix pipe) and its sum added to the running total: one chain over the whole of K = 4608 leaves
// six times the error of the reference's own float32 convolution, the chunked sum 1.2 times.  Every output
// walks every chunk in the same order whatever tile it lies in: no K split, the bits do not depend on the batch.
template <int KS>
__global__ __launch_bounds__(256) void sync_conv_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                        const float* __restrict__ bias, const float* __restrict__ res,
                                                        float* __restrict__ out, long long M, int H, int W, int Ho, int Wo, int cin, int cout,
                                                        int sh, int sw, int pad) {
  __shared__ __attribute__((aligned(16))) float As[CV_BM * CV_LD];
  __shared__ __attribute__((aligned(16))) float Bs[CV_BN * CV_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.x * CV_BM;
  const int n0 = blockIdx.y * CV_BN;
  const int K = KS * KS * cin;
  const int ch = tid & 7, r0 = tid >> 3;   // staging: 16-byte chunk `ch` of rows r0 and r0 + 32
  long long base[2];
  int iy0[2], ix0[2];
  bool ok[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long long m = m0 + r0 + 32 * j;
    ok[j] = m < M;
    const long long mm = ok[j] ? m : 0, hw = (long long)Ho * Wo, b = mm / hw;
    const int rem = (int)(mm - b * hw), oy = rem / Wo, ox = rem - oy * Wo;
    iy0[j] = oy * sh - pad, ix0[j] = ox * sw - pad;
    base[j] = b * H * (long long)W;
  }
  f32x4 ra[2], rb[2];
  auto load = [&](int tap, int c0) {
    const int ky = tap / KS, kx = tap - ky * KS;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int iy = iy0[j] + ky, ix = ix0[j] + kx;
      ra[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ok[j] && iy >= 0 && iy < H && ix >= 0 && ix < W)
        ra[j] = *reinterpret_cast<const f32x4*>(in + (base[j] + (long long)iy * W + ix) * cin + c0 + ch * 4);
      rb[j] = *reinterpret_cast<const f32x4*>(w + (size_t)(n0 + r0 + 32 * j) * K + tap * cin + c0 + ch * 4);
    }
  };
  const int wm = wave & 1, wn = wave >> 1, kh = lane >> 5;
  const float* ap = As + (wm * 32 + (lane & 31)) * CV_LD + 4 * kh;
  const float* bp = Bs + (wn * 32 + (lane & 31)) * CV_LD + 4 * kh;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  int tap = 0, c0 = 0;
  load(0, 0);
#pragma unroll 1
  for (int q = K / CV_BK; q > 0; --q) {
    __syncthreads();   // the previous chunk's fragments have been read
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      *reinterpret_cast<f32x4*>(As + (r0 + 32 * j) * CV_LD + ch * 4) = ra[j];
      *reinterpret_cast<f32x4*>(Bs + (r0 + 32 * j) * CV_LD + ch * 4) = rb[j];
    }
    __syncthreads();
    c0 += CV_BK;
    if (c0 == cin) c0 = 0, ++tap;
    if (q > 1) load(tap, c0);
    f32x16 part;
#pragma unroll
    for (int i = 0; i < 16; ++i) part[i] = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(ap + 8 * g);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(bp + 8 * g);
#pragma unroll
      for (int s = 0; s < 4; ++s) part = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bv[s], part, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] += part[i];
  }
  // C/D: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int n = n0 + wn * 32 + (lane & 31);
  const float bn = bias[n];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const long long m = m0 + wm * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * kh;
    if (m >= M) continue;
    float v = acc[reg] + bn;
    if (res) v += res[m * cout + n];
    out[m * cout + n] = relu(v);
  }
}

// ------------------------------------------------------------------------------------------------ ReLU in place
__global__ __launch_bounds__(256) void sync_relu_kernel(float* __restrict__ x, long long total4) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total4) return;
  f32x4 v = *reinterpret_cast<f32x4*>(x + idx * 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = relu(v[e]);
  *reinterpret_cast<f32x4*>(x + idx * 4) = v;
}

// ------------------------------------------------------------------------------------------------ NHWC -> NCHW
// in [B,HW,C] -> out [B,C,HW] (a debug tap: one element per lane)
__global__ __launch_bounds__(256) void sync_to_nchw_kernel(const float* __restrict__ in, float* __restrict__ out, long long total, int HW,
                                                           int C) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int p = (int)(idx % HW);
  const long long r = idx / HW;
  const int c = (int)(r % C);
  const long long b = r / C;
  out[idx] = in[(b * HW + p) * C + c];
}

// ------------------------------------------------------------------------------------------------ embedding
constexpr int EMB_C = 512, EMB_P = 9, EMB_D = EMB_C * EMB_P;

__device__ __forceinline__ double wave_sum(double v) {   // butterfly: every lane ends with the same sum, fixed order
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// in [B,9,512] -> out [B,4608]: out[c * 9 + p] = lrelu(in[p][c] / max(|in|_2, 1e-12)); one workgroup per frame
__global__ __launch_bounds__(256) void sync_embed_kernel(const float* __restrict__ in, float* __restrict__ out) {
  __shared__ double part[4];
  const int tid = threadIdx.x;
  const float* src = in + (long long)blockIdx.x * EMB_D;
  double s = 0.0;
  for (int j = tid; j < EMB_D; j += 256) {
    const double v = (double)src[j];
    s += v * v;
  }
  s = wave_sum(s);
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  const double total = ((part[0] + part[1]) + part[2]) + part[3];
  const float norm = fmaxf((float)sqrt(total), 1e-12f);
  float* dst = out + (long long)blockIdx.x * EMB_D;
  for (int j = tid; j < EMB_D; j += 256) {
    const int c = j / EMB_P, p = j - c * EMB_P;
    dst[j] = lrelu(src[p * EMB_C + c] / norm);
  }
}

// ------------------------------------------------------------------------------------------------ shift curve
// f, a [n,d] -> sim [(2 S + 1), n]; pair = (s + S) n + i, one wave each
__global__ __launch_bounds__(256) void sync_curve_kernel(const float* __restrict__ f, const float* __restrict__ a, float* __restrict__ sim,
                                                         long long pairs, int n, int d, int S) {
  const long long pair = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= pairs) return;
  const int lane = threadIdx.x & 63;
  const int i = (int)(pair % n);
  const long long j = (long long)i + (pair / n) - S;
  if (j < 0 || j >= n) {
    if (lane == 0) sim[pair] = 0.f;
    return;
  }
  const float *fp = f + (long long)i * d, *ap = a + j * d;
  double dot = 0.0, nf = 0.0, na = 0.0;
  for (int c = lane * 4; c < d; c += 256) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(fp + c), v = *reinterpret_cast<const f32x4*>(ap + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double ue = (double)u[e], ve = (double)v[e];
      dot += ue * ve, nf += ue * ue, na += ve * ve;
    }
  }
  dot = wave_sum(dot), nf = wave_sum(nf), na = wave_sum(na);
  if (lane != 0) return;
  const double den = sqrt(nf) * sqrt(na);
  sim[pair] = (float)(dot / (den > 1e-8 ? den : 1e-8));
}

// ------------------------------------------------------------------------------------------------ launchers
constexpr long long kMaxBytes = 1ll << 31;   // no operand of one launch reaches 2 GiB

int grid_for(long long items, int per_block, unsigned* grid) {
  const long long g = (items + per_block - 1) / per_block;
  CASYNC_REQUIRE(g >= 1 && g < (1ll << 31), "sync: grid of %lld blocks", g);
  *grid = (unsigned)g;
  return CASYNC_OK;
}

int launch_sync_stem7(const float* x, const float* w, const float* bias, float* out, int batch, int H, int W, hipStream_t s) {
  CASYNC_REQUIRE(x && w && bias && out, "sync stem7: null pointer");
  CASYNC_REQUIRE(batch > 0 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192, "sync stem7: B=%d %dx%d", batch, H, W);
  CASYNC_REQUIRE((uintptr_t)w % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)x % 4 == 0, "sync stem7: alignment");
  CASYNC_REQUIRE((long long)batch * H * W * S7_C * 4 < kMaxBytes, "sync stem7: output of 2 GiB or more");
  const int tiles_x = (W + S7_T - 1) / S7_T, tiles_y = (H + S7_T - 1) / S7_T;
  unsigned grid;
  if (int st = grid_for((long long)batch * tiles_x * tiles_y, 1, &grid)) return st;
  return casync_launch(sync_stem7_kernel, dim3(grid), dim3(256), 0, s, x, w, bias, out, H, W, tiles_x, tiles_y);
}

// ks 3 or 5; res (optional) [B Ho Wo][cout] is added before the ReLU
int launch_sync_conv(int ks, const float* in, const float* w, const float* bias, const float* res, float* out, int batch, int H, int W,
                     int cin, int cout, int sh, int sw, int pad, hipStream_t s) {
  CASYNC_REQUIRE(in && w && bias && out, "sync conv: null pointer");
  CASYNC_REQUIRE(ks == 3 || ks == 5, "sync conv: kernel size %d (3 or 5)", ks);
  CASYNC_REQUIRE(batch > 0 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192 && sh >= 1 && sw >= 1 && sh <= 8 && sw <= 8 && pad >= 0 && pad <= 8 &&
                     H + 2 * pad >= ks && W + 2 * pad >= ks,
                 "sync conv: B=%d %dx%d stride (%d,%d) pad %d kernel %d", batch, H, W, sh, sw, pad, ks);
  CASYNC_REQUIRE(cin >= CV_BK && cin % CV_BK == 0 && cin <= 4096 && cout >= CV_BN && cout % CV_BN == 0 && cout <= 4096,
                 "sync conv: cin=%d (a multiple of %d), cout=%d (a multiple of %d)", cin, CV_BK, cout, CV_BN);
  CASYNC_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)w % 16 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)res % 4 == 0 && (uintptr_t)bias % 4 == 0,
                 "sync conv: alignment");
  const int Ho = (H + 2 * pad - ks) / sh + 1, Wo = (W + 2 * pad - ks) / sw + 1;
  const long long M = (long long)batch * Ho * Wo;
  CASYNC_REQUIRE((long long)batch * H * W * cin * 4 < kMaxBytes && M * cout * 4 < kMaxBytes, "sync conv: an operand of 2 GiB or more");
  unsigned grid;
  if (int st = grid_for(M, CV_BM, &grid)) return st;
  const dim3 g(grid, (unsigned)(cout / CV_BN));
  if (ks == 5) return casync_launch(sync_conv_kernel<5>, g, dim3(256), 0, s, in, w, bias, res, out, M, H, W, Ho, Wo, cin, cout, sh, sw, pad);
  return casync_launch(sync_conv_kernel<3>, g, dim3(256), 0, s, in, w, bias, res, out, M, H, W, Ho, Wo, cin, cout, sh, sw, pad);
}

int launch_sync_relu(float* x, long long n, hipStream_t s) {
  CASYNC_REQUIRE(x && n > 0 && n % 4 == 0 && (uintptr_t)x % 16 == 0, "sync relu: n=%lld (a multiple of 4, 16-B aligned)", n);
  CASYNC_REQUIRE(n * 4 < kMaxBytes, "sync relu: 2 GiB or more");
  unsigned grid;
  if (int st = grid_for(n / 4, 256, &grid)) return st;
  return casync_launch(sync_relu_kernel, dim3(grid), dim3(256), 0, s, x, n / 4);
}

}  // namespace

// (declared in syncnet_common.h: the bf16 pass of syncnet_bf16.hip calls these two)
int launch_sync_to_nchw(const float* in, float* out, int batch, int hw, int c, hipStream_t s) {
  CASYNC_REQUIRE(in && out && batch > 0 && hw >= 1 && c >= 1, "sync to_nchw: B=%d hw=%d c=%d", batch, hw, c);
  const long long total = (long long)batch * hw * c;
  CASYNC_REQUIRE(total * 4 < kMaxBytes, "sync to_nchw: 2 GiB or more");
  unsigned grid;
  if (int st = grid_for(total, 256, &grid)) return st;
  return casync_launch(sync_to_nchw_kernel, dim3(grid), dim3(256), 0, s, in, out, total, hw, c);
}

int launch_sync_embed(const float* in, float* out, int batch, hipStream_t s) {
  CASYNC_REQUIRE(in && out && batch > 0 && batch <= 65536, "sync embed: null pointer or batch %d (1..65536)", batch);
  CASYNC_REQUIRE((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0, "sync embed: alignment");
  return casync_launch(sync_embed_kernel, dim3((unsigned)batch), dim3(256), 0, s, in, out);
}

namespace {

int launch_sync_curve(const float* f, const float* a, int n, int d, int max_shift, float* sim, hipStream_t s) {
  CASYNC_REQUIRE(f && a && sim, "sync curve: null pointer");
  CASYNC_REQUIRE(n >= 1 && n <= (1 << 24) && d >= 4 && d % 4 == 0 && d <= (1 << 20) && max_shift >= 0 && max_shift <= 4096,
                 "sync curve: n=%d d=%d (a multiple of 4) max_shift=%d (0..4096)", n, d, max_shift);
  CASYNC_REQUIRE((uintptr_t)f % 16 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)sim % 4 == 0, "sync curve: alignment");
  const long long pairs = (long long)(2 * max_shift + 1) * n;
  unsigned grid;
  if (int st = grid_for(pairs, 4, &grid)) return st;
  return casync_launch(sync_curve_kernel, dim3(grid), dim3(256), 0, s, f, a, sim, pairs, n, d, max_shift);
}

// ------------------------------------------------------------------------------------------------ network, packed layout
// (the block table SyncNet, sync_net() and the handle: syncnet_common.h)
constexpr int kFaceBlocks = kSyncFaceBlocks, kBlocks = kSyncBlocks, kFaceHW = kSyncFaceHW, kMaxPass = kSyncMaxPass;

// the arena of one pass: two activations, each on a 256-B boundary
struct SyncWs {
  float *a, *b;
  int64_t bytes;
  SyncWs(void* base, int nb, const SyncNet& N) {
    const int64_t act = round64((int64_t)nb * N.act_floats);
    a = static_cast<float*>(base), b = base ? a + act : nullptr;
    bytes = 2 * act * 4;
  }
};

#define DT(call)                        \
  do {                                  \
    if (int st__ = (call)) return st__; \
  } while (0)

constexpr int ST_FULL = kBlocks;   // both embeddings

// Blocks first .. last of one encoder on nb frames; x is the encoder's NCHW input.  *res is the NHWC output of block `last`.
int sync_blocks(const casync_sync* D, int first, int last, const float* x, int nb, const SyncWs& ws, const float** res, hipStream_t s) {
  const SyncNet& N = sync_net(D->mode);
  const float* w = D->pw.w;
  const float* in = x;
  float *dst = ws.a, *other = ws.b;
  if (first != 0) {   // the audio window to NHWC; the stem reads NCHW itself
    DT(launch_nchw_to_nhwc(x, ws.a, nb, N.audio_c, N.audio_h * N.audio_w, s));
    in = ws.a, dst = ws.b, other = ws.a;
  }
  for (int i = first; i <= last; ++i) {
    const SyncBlock& b = N.blk[i];
    const int h = N.h_in[i], wd = N.w_in[i];
    const float *wt = w + N.w_off[i], *bias = w + N.b_off[i];
    if (b.k == 7) {
      DT(launch_sync_stem7(in, wt, bias, dst, nb, h, wd, s));
    } else if (b.k > 1) {   // the residual is added before the ReLU
      DT(launch_sync_conv(b.k, in, wt, bias, b.res ? in : nullptr, dst, nb, h, wd, b.cin, b.cout, b.sh, b.sw, b.pad, s));
    } else {
      GemmEpilogue epi;
      epi.bias = bias;
      const int m = nb * h * wd;
      DT(launch_rows_gemm(in, b.cin, wt, dst, b.cout, m, b.cout, b.cin, epi, s));
      DT(launch_sync_relu(dst, (long long)m * b.cout, s));
    }
    in = dst;
    std::swap(dst, other);
  }
  *res = in;
  return CASYNC_OK;
}

// One pass of nb frames; stage < kBlocks: that block's output in NCHW order to `out`; ST_FULL: the two embeddings.
int sync_pass(const casync_sync* D, const float* face, const float* audio, int nb, const SyncWs& ws, int stage, float* out,
              float* audio_emb, float* face_emb, hipStream_t s) {
  const SyncNet& N = sync_net(D->mode);
  const float* res = nullptr;
  if (stage < kBlocks) {
    const bool is_face = stage < kFaceBlocks;
    DT(sync_blocks(D, is_face ? 0 : kFaceBlocks, stage, is_face ? face : audio, nb, ws, &res, s));
    return launch_sync_to_nchw(res, out, nb, N.h_out[stage] * N.w_out[stage], N.blk[stage].cout, s);
  }
  DT(sync_blocks(D, 0, kFaceBlocks - 1, face, nb, ws, &res, s));
  DT(launch_sync_embed(res, face_emb, nb, s));
  DT(sync_blocks(D, kFaceBlocks, kBlocks - 1, audio, nb, ws, &res, s));
  return launch_sync_embed(res, audio_emb, nb, s);
}

int sync_run(casync_sync* D, const float* face, const float* audio, int batch, int stage, float* out, float* audio_emb, float* face_emb,
             void* ws_dev, int64_t ws_bytes, hipStream_t s) {
  CASYNC_REQUIRE(D, "sync forward: null handle");
  CASYNC_REQUIRE(D->pw.w, "sync forward: weights not loaded");
  CASYNC_REQUIRE(batch >= 0 && batch <= 65536, "sync forward: batch %d (0..65536)", batch);
  CASYNC_REQUIRE(stage >= 0 && stage <= ST_FULL, "sync forward: stage %d (0..%d)", stage, ST_FULL - 1);
  if (batch == 0) return CASYNC_OK;
  const bool need_face = stage < kFaceBlocks || stage == ST_FULL, need_audio = stage >= kFaceBlocks;
  CASYNC_REQUIRE((!need_face || face) && (!need_audio || audio) && ws_dev, "sync forward: null pointer");
  CASYNC_REQUIRE(stage == ST_FULL ? (audio_emb && face_emb) : out != nullptr, "sync forward: null output");
  CASYNC_REQUIRE((uintptr_t)face % 16 == 0 && (uintptr_t)audio % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)audio_emb % 16 == 0 &&
                     (uintptr_t)face_emb % 16 == 0 && (uintptr_t)ws_dev % 256 == 0,
                 "sync forward: alignment");
  const SyncNet& N = sync_net(D->mode);
  const int nb = batch < kMaxPass ? batch : kMaxPass;
  const SyncWs ws(ws_dev, nb, N);
  const bool bf16 = D->precision == 1;   // its pass (syncnet_bf16.hip) lays out its own, smaller arena
  const int64_t need = bf16 ? sync16_ws_bytes(nb, N) : ws.bytes;
  if (ws_bytes < need) {
    casync_set_error("sync forward: workspace %lld bytes, needs %lld", (long long)ws_bytes, (long long)need);
    return CASYNC_ERR_STATE;
  }
  CASYNC_REQUIRE(!bf16 || D->pw.w16, "sync forward: bf16 weight image not made");
  DeviceGuard guard(D->device);
  CASYNC_CHECK_HIP(guard.err);
  std::unique_lock<std::mutex> gate_lock;   // held until this forward is enqueued
  if (int st = casync_gate_enter(D->device, D, &D->ev_fwd, s, &gate_lock)) return st;
  const int64_t face_frame = 3ll * kFaceHW * kFaceHW, audio_frame = (int64_t)N.audio_c * N.audio_h * N.audio_w;
  const int64_t out_frame = stage < kBlocks ? N.out_floats(stage) : 0;
  // every pass takes the tile choices of its own frame count; the kernels' sums do not depend on it (see the header comment)
  for (int b0 = 0; b0 < batch; b0 += nb) {
    const int n = batch - b0 < nb ? batch - b0 : nb;
    const float *fp = face ? face + (size_t)b0 * face_frame : nullptr, *ap = audio ? audio + (size_t)b0 * audio_frame : nullptr;
    float* op = out ? out + (size_t)b0 * out_frame : nullptr;
    float *ae = audio_emb ? audio_emb + (size_t)b0 * EMB_D : nullptr, *fe = face_emb ? face_emb + (size_t)b0 * EMB_D : nullptr;
    if (bf16) DT(sync16_pass(D, fp, ap, n, ws_dev, stage, op, ae, fe, s));
    else DT(sync_pass(D, fp, ap, n, ws, stage, op, ae, fe, s));
  }
  return CASYNC_OK;
}
#undef DT
}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

int casync_sync_packed_count(int mode) { return sync_mode_ok(mode) ? sync_net(mode).packed.count() : 0; }
const char* casync_sync_packed_name(int mode, int i) { return sync_mode_ok(mode) ? sync_net(mode).packed.name(i) : nullptr; }
int64_t casync_sync_packed_offset(int mode, int i) { return sync_mode_ok(mode) ? sync_net(mode).packed.offset(i) : -1; }
int64_t casync_sync_packed_size(int mode, int i) { return sync_mode_ok(mode) ? sync_net(mode).packed.size(i) : -1; }
int64_t casync_sync_packed_total(int mode) { return sync_mode_ok(mode) ? sync_net(mode).packed.total : 0; }
int64_t casync_sync_workspace_bytes(int mode, int batch) {
  if (!sync_mode_ok(mode) || batch < 1 || batch > 65536) return 0;
  return SyncWs(nullptr, batch < kMaxPass ? batch : kMaxPass, sync_net(mode)).bytes;
}

int64_t casync_syncnet_workspace_bytes_ex(int mode, int precision, int batch) {
  if (precision == 0) return casync_sync_workspace_bytes(mode, batch);
  if (precision != 1 || !sync_mode_ok(mode) || batch < 1 || batch > 65536) return 0;
  return sync16_ws_bytes(batch < kMaxPass ? batch : kMaxPass, sync_net(mode));
}

int casync_syncnet_create_ex(int device_id, int mode, int precision, casync_sync_handle* out) {
  CASYNC_REQUIRE(out, "sync_create: null out");
  *out = nullptr;
  CASYNC_REQUIRE(sync_mode_ok(mode), "sync_create: mode %d (0 hubert, 1 wenet)", mode);
  CASYNC_REQUIRE(precision == 0 || precision == 1, "sync_create: precision %d (0 fp32, 1 bf16)", precision);
  if (int st = casync_require_gfx950("sync_create", device_id)) return st;
  casync_sync* h = new casync_sync();
  h->device = device_id;
  h->mode = mode;
  h->precision = precision;
  *out = h;
  return CASYNC_OK;
}
int casync_sync_create(int device_id, int mode, casync_sync_handle* out) { return casync_syncnet_create_ex(device_id, mode, 0, out); }
int casync_syncnet_precision(casync_sync_handle h) { return h ? h->precision : -1; }

void casync_sync_destroy(casync_sync_handle h) {
  if (!h) return;
  DeviceGuard guard(h->device);
  casync_gate_forget(h->device, h, &h->ev_fwd);
  h->pw.release();
  delete h;
}

int casync_sync_load_weights_host(casync_sync_handle h, const float* packed, int64_t n_floats) {
  CASYNC_REQUIRE(h, "sync_load_weights: null");
  return h->pw.load_host("sync_load_weights", h->device, packed, n_floats, sync_net(h->mode).packed.total, h->precision == 1);
}

int casync_sync_load_weights_device(casync_sync_handle h, const float* packed_dev, int64_t n_floats) {
  CASYNC_REQUIRE(h, "sync_load_weights_device: null");
  return h->pw.adopt_device("sync_load_weights_device", h->device, packed_dev, n_floats, sync_net(h->mode).packed.total, h->precision == 1);
}

int casync_sync_forward(casync_sync_handle h, const float* face_dev, const float* audio_dev, int batch, float* audio_emb_dev,
                        float* face_emb_dev, void* workspace_dev, int64_t workspace_bytes, casync_stream stream) {
  return sync_run(h, face_dev, audio_dev, batch, ST_FULL, nullptr, audio_emb_dev, face_emb_dev, workspace_dev, workspace_bytes,
                  (hipStream_t)stream);
}
int casync_sync_forward_tap(casync_sync_handle h, const float* face_dev, const float* audio_dev, int batch, int stage, float* out_dev,
                            void* workspace_dev, int64_t workspace_bytes, casync_stream stream) {
  CASYNC_REQUIRE(stage >= 0 && stage < kBlocks, "sync_forward_tap: stage %d (0..%d)", stage, kBlocks - 1);
  return sync_run(h, face_dev, audio_dev, batch, stage, out_dev, nullptr, nullptr, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

int casync_op_sync_stem7(const float* x, const float* w, const float* bias, float* out, int batch, int h, int w_, casync_stream stream) {
  return launch_sync_stem7(x, w, bias, out, batch, h, w_, (hipStream_t)stream);
}
int casync_op_sync_conv5(const float* in, const float* w, const float* bias, float* out, int batch, int h, int w_, casync_stream stream) {
  return launch_sync_conv(5, in, w, bias, nullptr, out, batch, h, w_, 32, 64, 2, 2, 1, (hipStream_t)stream);
}
int casync_op_sync_conv3(const float* in, const float* w, const float* bias, const float* res, float* out, int batch, int h, int w_, int cin,
                         int cout, int stride_h, int stride_w, int pad, casync_stream stream) {
  return launch_sync_conv(3, in, w, bias, res, out, batch, h, w_, cin, cout, stride_h, stride_w, pad, (hipStream_t)stream);
}
int casync_op_sync_relu(float* x, int64_t n, casync_stream stream) { return launch_sync_relu(x, n, (hipStream_t)stream); }
int casync_op_sync_to_nchw(const float* in, float* out, int batch, int hw, int c, casync_stream stream) {
  return launch_sync_to_nchw(in, out, batch, hw, c, (hipStream_t)stream);
}
int casync_op_sync_embed(const float* in, float* out, int batch, casync_stream stream) {
  return launch_sync_embed(in, out, batch, (hipStream_t)stream);
}
int casync_op_sync_curve(const float* face_emb, const float* audio_emb, int n, int d, int max_shift, float* sim, casync_stream stream) {
  return launch_sync_curve(face_emb, audio_emb, n, d, max_shift, sim, (hipStream_t)stream);
}

}  // extern "C"
