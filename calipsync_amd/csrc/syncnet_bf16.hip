// The kernels of the bf16 precision of the SyncNet_color handle and their launchers.  The network's walk is sync_pass<SyncBF16> of
// syncnet.hip, which holds the fp32 kernels; syncnet_common.h is what the two share.  Activations are bf16 NHWC, every conv
// weight but face.0's is read from the handle's bf16 image of the packed buffer, biases stay fp32.
//
//   sync16_stem7_kernel       face.0: sync_stem7_kernel's body (fp32 weights on the fp32 NCHW input, the same fma order), one
//                             rounding to bf16 on the store.
//   sync16_conv_kernel<KS,BN> every other block, KS 1, 3 or 5: relu(conv + bias (+ x)) as an implicit GEMM on
//                             v_mfma_f32_16x16x32_bf16, fp32 accumulation; the residual (bf16, widened) is added in fp32 before the
//                             ReLU; one rounding to bf16 on the store, or an fp32 store (the last block of each encoder).
//                             BN = 64: 64 pixels x 64 channels per workgroup; BN = 16: 64 pixels x 16 channels, for launches whose
//                             64-channel tiles would be fewer than 64 workgroups (the 3x3 / 5x5 / 25-pixel tails of both encoders
//                             at small batches: four times as many workgroups stream a block's weights).
//   sync16_to_nchw_kernel     a bf16 NHWC block output widened into the reference's fp32 NCHW order (casync_sync_forward_tap).
// Both tiles issue the same instruction over the same k order (chunks of 64 in (ky, kx, cin) order, two instructions of 32 each,
// one accumulator per output from zero to K): the tile an output lies in does not touch its bits, so a frame of a batch has the
// bits of that frame forwarded alone.  No K split, no atomics, no sum across frames.  The audio window goes to bf16 NHWC with
// launch_nchw_to_nhwc, the weight image is launch_f32_to_bf16's (PackedWeights), the embedding launch_sync_embed on the fp32
// output of the last block: existing instances of lib/obj and lib/obj_sync.
#include <stdint.h>

#include "syncnet_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ stem (7x7)
// sync_stem7_body (syncnet_common.h) with the bf16 store
__global__ __launch_bounds__(256) void sync16_stem7_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, bf16_t* __restrict__ out, int H, int W,
                                                           int tiles_x, int tiles_y) {
  sync_stem7_body(x, w, bias, out, H, W, tiles_x, tiles_y);
}

// ------------------------------------------------------------------------------------------------ dense KS x KS conv
constexpr int C16_BM = 64, C16_BK = 64;   // pixels of a tile; k of a chunk: LDS rows of 128 B, eight 16-B slots
constexpr int C16_D = 4;                  // chunks between a global load and its use (even)

// Element offset of 16-B slot `slot` of LDS row `row`.  Rows are not padded; the slot is XORed with (row >> 1) & 7.  A fragment
// read has lane l on row 16 t + (l & 15), slot 4 s + (l >> 4): in each of ds_read_b128's four lane groups (rows {0-3, 12-15}
// of one slot with rows 4-11 of the next, or the other way round) the sixteen lanes fall on sixteen different slots of the
// 256-B bank row -- even rows on the low eight, odd rows on the high eight, (row >> 1) ^ slot a different value in each.
__device__ __forceinline__ int c16_off(int row, int slot) { return row * C16_BK + ((slot ^ ((row >> 1) & 7)) << 3); }

// in [B,H,W,cin], w [cout][(ky,kx,cin)], res (optional) [M = B Ho Wo][cout]: bf16; bias fp32; out [M][cout] bf16 or fp32:
// out = relu(conv + bias (+ res)).  256 threads stage a chunk (64 k of the 64 pixels and of the BN channels: each 16-B piece
// 8 channels of one tap of one pixel, zero outside the image, past M and past K) through registers into the LDS buffer the
// waves do not read, while they multiply the other one: one barrier per chunk.  The loads run C16_D chunks ahead of their use (a
// register ring): the small-M blocks stream 4.7 MB of weights through a few dozen workgroups and are bound by load latency.  Weights are the A operand and pixels the B
// operand, so a lane ends with four consecutive channels of one pixel: 8- or 16-byte stores.
template <int KS, int BN>
__global__ __launch_bounds__(256) void sync16_conv_kernel(const bf16_t* __restrict__ in, const bf16_t* __restrict__ w,
                                                          const float* __restrict__ bias, const bf16_t* __restrict__ res,
                                                          void* __restrict__ out, int out_f32, long long M, int H, int W, int Ho, int Wo,
                                                          int cin, int cout, int sh, int sw, int pad) {
  static_assert(BN == 64 || BN == 16, "tile");
  constexpr int NJ = BN == 64 ? 2 : 1;   // 16 x 16 instruction tiles of a wave along pixels and along channels
  __shared__ __attribute__((aligned(16))) bf16_t As[2][C16_BM * C16_BK];
  __shared__ __attribute__((aligned(16))) bf16_t Bs[2][BN * C16_BK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.x * C16_BM;
  const int n0 = blockIdx.y * BN;
  const int K = KS * KS * cin;
  const int ch = tid & 7, r0 = tid >> 3;   // staging: slot `ch` of rows r0 and r0 + 32
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
  int tap = 0, c = ch * 8;   // this thread's k = 64 q + 8 ch as (tap, channel)
  while (c >= cin) c -= cin, ++tap;
  const bool stage_b = BN == 64 || r0 < BN;
  // a ring of C16_D chunks in registers: slot d holds chunk d (mod C16_D) from its global load until it is staged into LDS
  u32x4 ra[C16_D][2], rb[C16_D][NJ];   // 8 bf16 each
  const u32x4 zero8 = {0u, 0u, 0u, 0u};
  auto load = [&](int d) {   // the chunk at (tap, c): zeros past K (no access), then on to the next chunk
    const bool kin = tap < KS * KS;
    const int ky = tap / KS, kx = tap - ky * KS;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int iy = iy0[j] + ky, ix = ix0[j] + kx;
      ra[d][j] = zero8;
      if (kin && ok[j] && iy >= 0 && iy < H && ix >= 0 && ix < W)
        ra[d][j] = *reinterpret_cast<const u32x4*>(in + (base[j] + (long long)iy * W + ix) * cin + c);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      rb[d][j] = zero8;
      if (kin && stage_b) rb[d][j] = *reinterpret_cast<const u32x4*>(w + (size_t)(n0 + r0 + 32 * j) * K + tap * cin + c);
    }
    c += C16_BK;
    while (c >= cin) c -= cin, ++tap;
  };
  auto stage = [&](int buf, int d) {
#pragma unroll
    for (int j = 0; j < 2; ++j) *reinterpret_cast<u32x4*>(&As[buf][c16_off(r0 + 32 * j, ch)]) = ra[d][j];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (stage_b) *reinterpret_cast<u32x4*>(&Bs[buf][c16_off(r0 + 32 * j, ch)]) = rb[d][j];
  };
  const int l15 = lane & 15, g = lane >> 4;
  const int mw = BN == 64 ? (wave & 1) * 32 : wave * 16;   // this wave's pixels and channels inside the tile
  const int nw = BN == 64 ? (wave >> 1) * 32 : 0;
  f32x4 acc[NJ][NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nq = (K + C16_BK - 1) / C16_BK;
#pragma unroll
  for (int d = 0; d < C16_D; ++d) load(d);   // chunks 0 .. C16_D - 1 in flight
  stage(0, 0);
  load(0);                                   // chunk C16_D
  __syncthreads();
#pragma unroll 1
  for (int q = 0; q < nq; q += C16_D) {
#pragma unroll
    for (int d = 0; d < C16_D; ++d) {        // chunk q + d is in LDS buffer d & 1 (C16_D is even), chunk q + d + 1 in slot (d + 1) % C16_D
      if (q + d < nq) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          bf16x8 px[NJ], wt[NJ];
#pragma unroll
          for (int i = 0; i < NJ; ++i) px[i] = *reinterpret_cast<const bf16x8*>(&As[d & 1][c16_off(mw + 16 * i + l15, 4 * s + g)]);
#pragma unroll
          for (int j = 0; j < NJ; ++j) wt[j] = *reinterpret_cast<const bf16x8*>(&Bs[d & 1][c16_off(nw + 16 * j + l15, 4 * s + g)]);
#pragma unroll
          for (int i = 0; i < NJ; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[j], px[i], acc[i][j], 0, 0, 0);
        }
      }
      if (q + d + 1 < nq) {
        stage((d + 1) & 1, (d + 1) % C16_D);   // (that buffer was read last before the previous barrier)
        load((d + 1) % C16_D);                 // chunk q + d + 1 + C16_D
      }
      __syncthreads();
    }
  }
  // C/D: column (pixel) = lane & 15, row (channel) = 4 (lane >> 4) + reg
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    const long long m = m0 + mw + 16 * i + l15;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int n = n0 + nw + 16 * j + 4 * g;
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias + n);
      f32x4 v = acc[i][j];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += b4[e];
      if (res) {
        const bf16x4 r4 = *reinterpret_cast<const bf16x4*>(res + m * cout + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += (float)r4[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = relu(v[e]);
      if (out_f32) *reinterpret_cast<f32x4*>(static_cast<float*>(out) + m * cout + n) = v;
      else *reinterpret_cast<bf16x4*>(static_cast<bf16_t*>(out) + m * cout + n) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
    }
  }
}

// ------------------------------------------------------------------------------------------------ bf16 NHWC -> fp32 NCHW
// in [B,HW,C] bf16 -> out [B,C,HW] fp32: sync_to_nchw_body (syncnet_common.h) on bf16
__global__ __launch_bounds__(256) void sync16_to_nchw_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, long long total, int HW,
                                                             int C) {
  sync_to_nchw_body(in, out, total, HW, C);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ launchers
int launch_sync16_stem7(const float* x, const float* w, const float* bias, void* out, int batch, int H, int W, hipStream_t s) {
  CASYNC_REQUIRE(x && w && bias && out, "sync16 stem7: null pointer");
  CASYNC_REQUIRE(batch > 0 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192, "sync16 stem7: B=%d %dx%d", batch, H, W);
  CASYNC_REQUIRE((uintptr_t)w % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)x % 4 == 0 && (uintptr_t)bias % 4 == 0, "sync16 stem7: alignment");
  CASYNC_REQUIRE((long long)batch * H * W * S7_C * 2 < kMaxBytes, "sync16 stem7: output of 2 GiB or more");
  const int tiles_x = (W + S7_T - 1) / S7_T, tiles_y = (H + S7_T - 1) / S7_T;
  unsigned grid;
  if (int st = grid_for("sync16", (long long)batch * tiles_x * tiles_y, 1, &grid)) return st;
  return casync_launch(sync16_stem7_kernel, dim3(grid), dim3(256), 0, s, x, w, bias, static_cast<bf16_t*>(out), H, W, tiles_x, tiles_y);
}

// tile: 64 or 16 channels of a workgroup (3x3 only), 0 = 16 where 64 would make fewer than 64 workgroups; the 5x5 block takes 64,
// the 1x1 blocks 16.  The choice does not touch an output's bits (see the header comment).
int launch_sync16_conv(int ks, const void* in, const void* w, const float* bias, const void* res, void* out, bool out_f32, int batch, int H,
                       int W, int cin, int cout, int sh, int sw, int pad, hipStream_t s, int tile) {
  CASYNC_REQUIRE(in && w && bias && out, "sync16 conv: null pointer");
  CASYNC_REQUIRE(ks == 1 || ks == 3 || ks == 5, "sync16 conv: kernel size %d (1, 3 or 5)", ks);
  CASYNC_REQUIRE(tile == 0 || (ks == 3 && (tile == 16 || tile == 64)), "sync16 conv: tile %d (0; 16 or 64 for the 3x3 kernel)", tile);
  CASYNC_REQUIRE(batch > 0 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192 && sh >= 1 && sw >= 1 && sh <= 8 && sw <= 8 && pad >= 0 && pad <= 8 &&
                     H + 2 * pad >= ks && W + 2 * pad >= ks,
                 "sync16 conv: B=%d %dx%d stride (%d,%d) pad %d kernel %d", batch, H, W, sh, sw, pad, ks);
  CASYNC_REQUIRE(cin >= 32 && cin % 32 == 0 && cin <= 4096 && cout >= 64 && cout % 64 == 0 && cout <= 4096,
                 "sync16 conv: cin=%d (a multiple of 32), cout=%d (a multiple of 64)", cin, cout);
  CASYNC_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)w % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)res % 8 == 0 && (uintptr_t)bias % 16 == 0,
                 "sync16 conv: alignment");
  const int Ho = (H + 2 * pad - ks) / sh + 1, Wo = (W + 2 * pad - ks) / sw + 1;
  const long long M = (long long)batch * Ho * Wo;
  CASYNC_REQUIRE((long long)batch * H * W * cin * 2 < kMaxBytes && M * cout * 4 < kMaxBytes && (long long)cout * ks * ks * cin * 2 < kMaxBytes,
                 "sync16 conv: an operand of 2 GiB or more");
  unsigned grid;
  if (int st = grid_for("sync16", M, C16_BM, &grid)) return st;
  const bf16_t *i16 = static_cast<const bf16_t*>(in), *w16 = static_cast<const bf16_t*>(w), *r16 = static_cast<const bf16_t*>(res);
  const int f32 = out_f32 ? 1 : 0;
  const dim3 wide(grid, (unsigned)(cout / 64)), narrow(grid, (unsigned)(cout / 16));
  if (ks == 5)
    return casync_launch(sync16_conv_kernel<5, 64>, wide, dim3(256), 0, s, i16, w16, bias, r16, out, f32, M, H, W, Ho, Wo, cin, cout, sh, sw, pad);
  if (ks == 1)
    return casync_launch(sync16_conv_kernel<1, 16>, narrow, dim3(256), 0, s, i16, w16, bias, r16, out, f32, M, H, W, Ho, Wo, cin, cout, sh, sw, pad);
  if (tile == 0) tile = (long long)grid * (cout / 64) < 64 ? 16 : 64;
  if (tile == 16)
    return casync_launch(sync16_conv_kernel<3, 16>, narrow, dim3(256), 0, s, i16, w16, bias, r16, out, f32, M, H, W, Ho, Wo, cin, cout, sh, sw, pad);
  return casync_launch(sync16_conv_kernel<3, 64>, wide, dim3(256), 0, s, i16, w16, bias, r16, out, f32, M, H, W, Ho, Wo, cin, cout, sh, sw, pad);
}

int launch_sync16_to_nchw(const void* in, float* out, int batch, int hw, int c, hipStream_t s) {
  CASYNC_REQUIRE(in && out && batch > 0 && hw >= 1 && c >= 1, "sync16 to_nchw: B=%d hw=%d c=%d", batch, hw, c);
  const long long total = (long long)batch * hw * c;
  CASYNC_REQUIRE(total * 4 < kMaxBytes, "sync16 to_nchw: 2 GiB or more");
  unsigned grid;
  if (int st = grid_for("sync16", total, 256, &grid)) return st;
  return casync_launch(sync16_to_nchw_kernel, dim3(grid), dim3(256), 0, s, static_cast<const bf16_t*>(in), out, total, hw, c);
}

// ---- C ABI: one entry per kernel (tests/kernel_ledger_sync16.py) ------------------------------------------------------
extern "C" {

int casync_op_sync16_stem7(const float* x, const float* w, const float* bias, void* out, int batch, int h, int w_, casync_stream stream) {
  return launch_sync16_stem7(x, w, bias, out, batch, h, w_, (hipStream_t)stream);
}
int casync_op_sync16_conv5(const void* in, const void* w, const float* bias, void* out, int batch, int h, int w_, casync_stream stream) {
  return launch_sync16_conv(5, in, w, bias, nullptr, out, false, batch, h, w_, 32, 64, 2, 2, 1, (hipStream_t)stream);
}
int casync_op_sync16_conv3(const void* in, const void* w, const float* bias, const void* res, void* out, int batch, int h, int w_, int cin,
                           int cout, int stride_h, int stride_w, int pad, int tile, casync_stream stream) {
  CASYNC_REQUIRE(tile == 16 || tile == 64, "sync16_conv3: tile %d (16 or 64)", tile);
  return launch_sync16_conv(3, in, w, bias, res, out, false, batch, h, w_, cin, cout, stride_h, stride_w, pad, (hipStream_t)stream, tile);
}
int casync_op_sync16_conv1(const void* in, const void* w, const float* bias, float* out, int batch, int h, int w_, int cin, int cout,
                           casync_stream stream) {
  return launch_sync16_conv(1, in, w, bias, nullptr, out, true, batch, h, w_, cin, cout, 1, 1, 0, (hipStream_t)stream);
}
int casync_op_sync16_to_nchw(const void* in, float* out, int batch, int hw, int c, casync_stream stream) {
  return launch_sync16_to_nchw(in, out, batch, hw, c, (hipStream_t)stream);
}

}  // extern "C"
