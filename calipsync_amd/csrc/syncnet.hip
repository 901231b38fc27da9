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
// The network's order is written once, in sync_blocks<P> / sync_pass<P>; a precision is a policy P (SyncF32, SyncBF16) that names
// its element type, its launchers and the image its matrices come from.  sync_pass<SyncBF16> is the same walk on bf16
// activations with the kernels of syncnet_bf16.hip.  The block table, the handle and the stem / to_nchw bodies both objects
// compile are in syncnet_common.h.
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "syncnet_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ stem (7x7)
// sync_stem7_body (syncnet_common.h) with the fp32 store
__global__ __launch_bounds__(256) void sync_stem7_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ out, int H, int W, int tiles_x,
                                                         int tiles_y) {
  sync_stem7_body(x, w, bias, out, H, W, tiles_x, tiles_y);
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
// in [B,HW,C] -> out [B,C,HW]: sync_to_nchw_body (syncnet_common.h) on fp32
__global__ __launch_bounds__(256) void sync_to_nchw_kernel(const float* __restrict__ in, float* __restrict__ out, long long total, int HW,
                                                           int C) {
  sync_to_nchw_body(in, out, total, HW, C);
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
int launch_sync_stem7(const float* x, const float* w, const float* bias, float* out, int batch, int H, int W, hipStream_t s) {
  CASYNC_REQUIRE(x && w && bias && out, "sync stem7: null pointer");
  CASYNC_REQUIRE(batch > 0 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192, "sync stem7: B=%d %dx%d", batch, H, W);
  CASYNC_REQUIRE((uintptr_t)w % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)x % 4 == 0, "sync stem7: alignment");
  CASYNC_REQUIRE((long long)batch * H * W * S7_C * 4 < kMaxBytes, "sync stem7: output of 2 GiB or more");
  const int tiles_x = (W + S7_T - 1) / S7_T, tiles_y = (H + S7_T - 1) / S7_T;
  unsigned grid;
  if (int st = grid_for("sync", (long long)batch * tiles_x * tiles_y, 1, &grid)) return st;
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
  if (int st = grid_for("sync", M, CV_BM, &grid)) return st;
  const dim3 g(grid, (unsigned)(cout / CV_BN));
  if (ks == 5) return casync_launch(sync_conv_kernel<5>, g, dim3(256), 0, s, in, w, bias, res, out, M, H, W, Ho, Wo, cin, cout, sh, sw, pad);
  return casync_launch(sync_conv_kernel<3>, g, dim3(256), 0, s, in, w, bias, res, out, M, H, W, Ho, Wo, cin, cout, sh, sw, pad);
}

int launch_sync_relu(float* x, long long n, hipStream_t s) {
  CASYNC_REQUIRE(x && n > 0 && n % 4 == 0 && (uintptr_t)x % 16 == 0, "sync relu: n=%lld (a multiple of 4, 16-B aligned)", n);
  CASYNC_REQUIRE(n * 4 < kMaxBytes, "sync relu: 2 GiB or more");
  unsigned grid;
  if (int st = grid_for("sync", n / 4, 256, &grid)) return st;
  return casync_launch(sync_relu_kernel, dim3(grid), dim3(256), 0, s, x, n / 4);
}

int launch_sync_to_nchw(const float* in, float* out, int batch, int hw, int c, hipStream_t s) {
  CASYNC_REQUIRE(in && out && batch > 0 && hw >= 1 && c >= 1, "sync to_nchw: B=%d hw=%d c=%d", batch, hw, c);
  const long long total = (long long)batch * hw * c;
  CASYNC_REQUIRE(total * 4 < kMaxBytes, "sync to_nchw: 2 GiB or more");
  unsigned grid;
  if (int st = grid_for("sync", total, 256, &grid)) return st;
  return casync_launch(sync_to_nchw_kernel, dim3(grid), dim3(256), 0, s, in, out, total, hw, c);
}

int launch_sync_embed(const float* in, float* out, int batch, hipStream_t s) {
  CASYNC_REQUIRE(in && out && batch > 0 && batch <= 65536, "sync embed: null pointer or batch %d (1..65536)", batch);
  CASYNC_REQUIRE((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0, "sync embed: alignment");
  return casync_launch(sync_embed_kernel, dim3((unsigned)batch), dim3(256), 0, s, in, out);
}

int launch_sync_curve(const float* f, const float* a, int n, int d, int max_shift, float* sim, hipStream_t s) {
  CASYNC_REQUIRE(f && a && sim, "sync curve: null pointer");
  CASYNC_REQUIRE(n >= 1 && n <= (1 << 24) && d >= 4 && d % 4 == 0 && d <= (1 << 20) && max_shift >= 0 && max_shift <= 4096,
                 "sync curve: n=%d d=%d (a multiple of 4) max_shift=%d (0..4096)", n, d, max_shift);
  CASYNC_REQUIRE((uintptr_t)f % 16 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)sim % 4 == 0, "sync curve: alignment");
  const long long pairs = (long long)(2 * max_shift + 1) * n;
  unsigned grid;
  if (int st = grid_for("sync", pairs, 4, &grid)) return st;
  return casync_launch(sync_curve_kernel, dim3(grid), dim3(256), 0, s, f, a, sim, pairs, n, d, max_shift);
}

// ------------------------------------------------------------------------------------------------ network, packed layout
// (the block table SyncNet, sync_net() and the handle: syncnet_common.h)
constexpr int kFaceBlocks = kSyncFaceBlocks, kBlocks = kSyncBlocks, kFaceHW = kSyncFaceHW, kMaxPass = kSyncMaxPass;

// the arena of one pass: two activations of nb * act_floats values of T, each on a 256-B boundary.  In fp32 this is the rule in
// floats it replaces, round64(n) * 4 == (4 n + 255) / 256 * 256, in bf16 the 128-element rounding, (n + 127) / 128 * 128 * 2 ==
// (2 n + 255) / 256 * 256: the offsets and the totals are the same.
template <class T>
struct SyncWs {
  T *a, *b;
  int64_t bytes;
  SyncWs(void* base, int nb, const SyncNet& N) {
    const int64_t act = ((int64_t)nb * N.act_floats * (int64_t)sizeof(T) + 255) / 256 * 256;
    a = static_cast<T*>(base), b = base ? a + act / (int64_t)sizeof(T) : nullptr;
    bytes = 2 * act;
  }
};

// frames of one pass through the network, and the workspace of (mode, precision, batch): 0 for what no handle takes
int sync_pass_frames(int batch) { return batch < kMaxPass ? batch : kMaxPass; }
int64_t sync_ws_bytes(int mode, int precision, int batch) {
  if (!sync_mode_ok(mode) || (precision != 0 && precision != 1) || batch < 1 || batch > 65536) return 0;
  const int nb = sync_pass_frames(batch);
  return precision == 1 ? SyncWs<bf16_t>(nullptr, nb, sync_net(mode)).bytes : SyncWs<float>(nullptr, nb, sync_net(mode)).bytes;
}

#define DT(call)                        \
  do {                                  \
    if (int st__ = (call)) return st__; \
  } while (0)

constexpr int ST_FULL = kBlocks;   // both embeddings

// A precision of the handle: the element type of the activations, the dtype the audio window is converted to, the image the
// conv / GEMM matrices are read from, the stem, one dense block (k 1, 3 or 5; f32: the block's output stays fp32) and how a tap
// leaves.  What the network does is in sync_blocks and sync_pass.
struct SyncF32 {
  using T = float;
  static constexpr int dtype = DT_F32;
  static constexpr auto stem = launch_sync_stem7;
  static const T* mats(const casync_sync* D) { return D->pw.w; }
  static int block(const SyncBlock& b, const T* in, const T* wt, const float* bias, const T* res, T* dst, bool, int nb, int h, int wd,
                   hipStream_t s) {
    if (b.k > 1) return launch_sync_conv(b.k, in, wt, bias, res, dst, nb, h, wd, b.cin, b.cout, b.sh, b.sw, b.pad, s);
    GemmEpilogue epi;   // the two 1x1 blocks: rows GEMM, ReLU pass
    epi.bias = bias;
    const int m = nb * h * wd;
    DT(launch_rows_gemm(in, b.cin, wt, dst, b.cout, m, b.cout, b.cin, epi, s));
    return launch_sync_relu(dst, (long long)m * b.cout, s);
  }
  static int tap_out(const void* src, bool, float* out, int nb, int hw, int c, hipStream_t s) {
    return launch_sync_to_nchw(static_cast<const float*>(src), out, nb, hw, c, s);
  }
};

// the contract: DESIGN section 8l; the last block of each encoder stores fp32, every other tap is widened
struct SyncBF16 {
  using T = bf16_t;
  static constexpr int dtype = DT_BF16;
  static constexpr auto stem = launch_sync16_stem7;
  static const T* mats(const casync_sync* D) { return D->pw.w16; }
  static int block(const SyncBlock& b, const T* in, const T* wt, const float* bias, const T* res, T* dst, bool f32, int nb, int h, int wd,
                   hipStream_t s) {
    return launch_sync16_conv(b.k, in, wt, bias, res, dst, f32, nb, h, wd, b.cin, b.cout, b.sh, b.sw, b.pad, s);
  }
  static int tap_out(const void* src, bool f32, float* out, int nb, int hw, int c, hipStream_t s) {
    return f32 ? SyncF32::tap_out(src, f32, out, nb, hw, c, s) : launch_sync16_to_nchw(src, out, nb, hw, c, s);
  }
};

bool sync_last_of_encoder(int i) { return i == kFaceBlocks - 1 || i == kBlocks - 1; }   // face.16, audio.13: fp32 out in both precisions

// Blocks first .. last of one encoder on nb frames in the precision P; x is the encoder's fp32 NCHW input.  *res is the NHWC
// output of block `last`: of P::T, or fp32 when that is the encoder's last block.
template <class P>
int sync_blocks(const casync_sync* D, int first, int last, const float* x, int nb, const SyncWs<typename P::T>& ws, const void** res,
                hipStream_t s) {
  using T = typename P::T;
  const SyncNet& N = sync_net(D->mode);
  const float* w = D->pw.w;   // biases and the stem's weights; wm: the image the matrices come from
  const T* wm = P::mats(D);
  const T* in = nullptr;
  T *dst = ws.a, *other = ws.b;
  if (first != 0) {   // the audio window to NHWC of T; the stem reads fp32 NCHW itself
    DT(launch_nchw_to_nhwc(x, ws.a, nb, N.audio_c, N.audio_h * N.audio_w, s, P::dtype));
    in = ws.a, dst = ws.b, other = ws.a;
  }
  for (int i = first; i <= last; ++i) {
    const SyncBlock& b = N.blk[i];
    const int h = N.h_in[i], wd = N.w_in[i];
    const float* bias = w + N.b_off[i];
    if (b.k == 7) DT(P::stem(x, w + N.w_off[i], bias, dst, nb, h, wd, s));
    else DT(P::block(b, in, wm + N.w_off[i], bias, b.res ? in : nullptr, dst, sync_last_of_encoder(i), nb, h, wd, s));   // + x before the ReLU
    in = dst;
    std::swap(dst, other);
  }
  *res = in;
  return CASYNC_OK;
}

// One pass of nb frames; stage < kBlocks: that block's output in fp32 NCHW order to `out`; ST_FULL: the two embeddings.
template <class P>
int sync_pass(const casync_sync* D, const float* face, const float* audio, int nb, const SyncWs<typename P::T>& ws, int stage, float* out,
              float* audio_emb, float* face_emb, hipStream_t s) {
  const SyncNet& N = sync_net(D->mode);
  const void* res = nullptr;
  if (stage < kBlocks) {
    const bool is_face = stage < kFaceBlocks;
    DT(sync_blocks<P>(D, is_face ? 0 : kFaceBlocks, stage, is_face ? face : audio, nb, ws, &res, s));
    return P::tap_out(res, sync_last_of_encoder(stage), out, nb, N.h_out[stage] * N.w_out[stage], N.blk[stage].cout, s);
  }
  DT(sync_blocks<P>(D, 0, kFaceBlocks - 1, face, nb, ws, &res, s));
  DT(launch_sync_embed(static_cast<const float*>(res), face_emb, nb, s));
  DT(sync_blocks<P>(D, kFaceBlocks, kBlocks - 1, audio, nb, ws, &res, s));
  return launch_sync_embed(static_cast<const float*>(res), audio_emb, nb, s);
}

// the checked batch in passes of nb frames at the most, in the arena of the precision P
template <class P>
int sync_batches(casync_sync* D, const float* face, const float* audio, int batch, int nb, int stage, float* out, float* audio_emb,
                 float* face_emb, void* ws_dev, hipStream_t s) {
  const SyncNet& N = sync_net(D->mode);
  const SyncWs<typename P::T> ws(ws_dev, nb, N);
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
    DT(sync_pass<P>(D, fp, ap, n, ws, stage, op, ae, fe, s));
  }
  return CASYNC_OK;
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
  const bool bf16 = D->precision == 1;
  const int64_t need = sync_ws_bytes(D->mode, D->precision, batch);
  if (ws_bytes < need) {
    casync_set_error("sync forward: workspace %lld bytes, needs %lld", (long long)ws_bytes, (long long)need);
    return CASYNC_ERR_STATE;
  }
  CASYNC_REQUIRE(!bf16 || D->pw.w16, "sync forward: bf16 weight image not made");
  const int nb = sync_pass_frames(batch);
  return bf16 ? sync_batches<SyncBF16>(D, face, audio, batch, nb, stage, out, audio_emb, face_emb, ws_dev, s)
              : sync_batches<SyncF32>(D, face, audio, batch, nb, stage, out, audio_emb, face_emb, ws_dev, s);
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
int64_t casync_sync_workspace_bytes(int mode, int batch) { return sync_ws_bytes(mode, 0, batch); }
int64_t casync_syncnet_workspace_bytes_ex(int mode, int precision, int batch) { return sync_ws_bytes(mode, precision, batch); }

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
