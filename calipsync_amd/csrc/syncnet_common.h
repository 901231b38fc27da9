// What the two precisions of the SyncNet_color handle share (syncnet.hip: fp32 and the walk of both, syncnet_bf16.hip: the bf16
// kernels): the block table of the network with its packed layout, the handle itself, the bf16 launchers the walk calls, and, in
// the anonymous namespace, the device bodies of the stem and of the NHWC -> NCHW tap with what their launchers need.  The two
// objects stay independent translation units: each has its own __global__ kernels, under its own names, around these bodies.
#pragma once

#include <string>

#include "common.h"
#include "handle.h"

struct SyncBlock {
  int k, cin, cout, sh, sw, pad, res;
};
constexpr int kSyncFaceBlocks = 17, kSyncAudioBlocks = 14, kSyncBlocks = kSyncFaceBlocks + kSyncAudioBlocks;
constexpr int kSyncFaceHW = 160, kSyncMaxPass = 256;   // frames of one pass through the network
constexpr int kSyncEmbed = 4608;                       // 512 channels x 3 x 3

// the 31 blocks of one mode with their sizes and the packed layout, every offset resolved once
struct SyncNet {
  SyncBlock blk[kSyncBlocks];
  int h_in[kSyncBlocks], w_in[kSyncBlocks], h_out[kSyncBlocks], w_out[kSyncBlocks];
  PackedLayout packed;
  int64_t w_off[kSyncBlocks], b_off[kSyncBlocks];
  int audio_c, audio_h, audio_w;
  int64_t act_floats = 0;   // the largest activation of one frame
  explicit SyncNet(int mode) {
    const bool wenet = mode == CASYNC_AUDIO_WENET;
    audio_c = wenet ? 256 : 32, audio_h = wenet ? 16 : 32, audio_w = 32;
    int n = 0;
    auto add = [&](int k, int cin, int cout, int sh, int sw, int pad, int res) { blk[n++] = SyncBlock{k, cin, cout, sh, sw, pad, res}; };
    auto stage = [&](int cin, int cout, int sh, int sw, int pad, int n_res) {   // a 3x3 conv and the residual blocks behind it
      add(3, cin, cout, sh, sw, pad, 0);
      for (int i = 0; i < n_res; ++i) add(3, cout, cout, 1, 1, 1, 1);
    };
    add(7, 3, 32, 1, 1, 3, 0);
    add(5, 32, 64, 2, 2, 1, 0);
    add(3, 64, 64, 1, 1, 1, 1), add(3, 64, 64, 1, 1, 1, 1);
    stage(64, 128, 2, 2, 1, 3), stage(128, 256, 2, 2, 1, 2), stage(256, 512, 2, 2, 1, 2);
    stage(512, 512, 2, 2, 1, 0), stage(512, 512, 1, 1, 0, 0);
    add(1, 512, 512, 1, 1, 0, 0);
    stage(audio_c, 256, 1, 1, 1, 2), stage(256, 256, wenet ? 1 : 2, 2, 1, 2), stage(256, 256, 2, 2, 2, 2), stage(256, 512, 2, 2, 1, 2);
    stage(512, 512, 1, 1, 0, 0);
    add(1, 512, 512, 1, 1, 0, 0);
    for (int i = 0; i < kSyncBlocks; ++i) {
      const SyncBlock& b = blk[i];
      const bool first = i == 0 || i == kSyncFaceBlocks;
      h_in[i] = first ? (i == 0 ? kSyncFaceHW : audio_h) : h_out[i - 1];
      w_in[i] = first ? (i == 0 ? kSyncFaceHW : audio_w) : w_out[i - 1];
      h_out[i] = (h_in[i] + 2 * b.pad - b.k) / b.sh + 1, w_out[i] = (w_in[i] + 2 * b.pad - b.k) / b.sw + 1;
      const int64_t act = (int64_t)h_out[i] * w_out[i] * b.cout;
      act_floats = act > act_floats ? act : act_floats;
      const std::string p = i < kSyncFaceBlocks ? "face." + std::to_string(i) : "audio." + std::to_string(i - kSyncFaceBlocks);
      w_off[i] = packed.add(p + ".w", (int64_t)b.cout * b.k * b.k * b.cin), b_off[i] = packed.add(p + ".b", b.cout);
    }
    const int64_t audio_in = (int64_t)audio_c * audio_h * audio_w;
    act_floats = audio_in > act_floats ? audio_in : act_floats;
  }
  int64_t out_floats(int i) const { return (int64_t)h_out[i] * w_out[i] * blk[i].cout; }
};
inline bool sync_mode_ok(int mode) { return mode == CASYNC_AUDIO_HUBERT || mode == CASYNC_AUDIO_WENET; }
inline const SyncNet& sync_net(int mode) {
  static const SyncNet nets[2] = {SyncNet(CASYNC_AUDIO_HUBERT), SyncNet(CASYNC_AUDIO_WENET)};
  return nets[mode == CASYNC_AUDIO_WENET ? 1 : 0];
}

struct casync_sync {
  int device = 0;
  int mode = 0;
  int precision = 0;             // 0 fp32, 1 bf16 (pw.w16 is then the bf16 image of the packed buffer)
  PackedWeights pw;
  hipEvent_t ev_fwd = nullptr;   // forward gate slot
};

// ---- syncnet_bf16.hip (pointers named void* are bf16, NHWC) ----
int launch_sync16_stem7(const float* x, const float* w, const float* bias, void* out, int batch, int H, int W, hipStream_t s);
// ks 1, 3 or 5 (tile: see the launcher); w [cout][(ky,kx,cin)] bf16; res (optional, bf16) [B Ho Wo][cout] is added before the ReLU; out bf16 or, out_f32, fp32
int launch_sync16_conv(int ks, const void* in, const void* w, const float* bias, const void* res, void* out, bool out_f32, int batch, int H,
                       int W, int cin, int cout, int sh, int sw, int pad, hipStream_t s, int tile = 0);
int launch_sync16_to_nchw(const void* in, float* out, int batch, int hw, int c, hipStream_t s);

namespace {

__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : 0.f; }

// ------------------------------------------------------------------------------------------------ stem (7x7)
constexpr int S7_T = 16;            // output tile
constexpr int S7_IN = S7_T + 6;     // with the halo
constexpr int S7_LD = S7_IN + 1;    // LDS row stride (odd)
constexpr int S7_C = 32, S7_K = 147;

// x [B,3,H,W] fp32, w [(ky,kx,ci)=147][32] fp32, out [B,H,W,32] of TO (float: 16-byte stores; bf16_t: one rounding on the store);
// one thread per output pixel of the tile, all 32 channels.  A workgroup of 256 threads, one tile each.
template <class TO>
__device__ __forceinline__ void sync_stem7_body(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                TO* __restrict__ out, int H, int W, int tiles_x, int tiles_y) {
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
  TO* o = out + ((b * H + oy) * (long long)W + ox) * S7_C;
  if constexpr (sizeof(TO) == 4) {
#pragma unroll
    for (int c4 = 0; c4 < S7_C / 4; ++c4)
      *reinterpret_cast<f32x4*>(o + c4 * 4) = f32x4{relu(acc[c4 * 4]), relu(acc[c4 * 4 + 1]), relu(acc[c4 * 4 + 2]), relu(acc[c4 * 4 + 3])};
  } else {
#pragma unroll
    for (int c8 = 0; c8 < S7_C / 8; ++c8) {
      bf16x8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (bf16_t)relu(acc[c8 * 8 + e]);
      *reinterpret_cast<bf16x8*>(o + c8 * 8) = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------ NHWC -> NCHW
// in [B,HW,C] of TI -> out [B,C,HW] fp32 (a debug tap: one element per lane)
template <class TI>
__device__ __forceinline__ void sync_to_nchw_body(const TI* __restrict__ in, float* __restrict__ out, long long total, int HW, int C) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int p = (int)(idx % HW);
  const long long r = idx / HW;
  const int c = (int)(r % C);
  const long long b = r / C;
  out[idx] = (float)in[(b * HW + p) * C + c];
}

// ------------------------------------------------------------------------------------------------ for the launchers
constexpr long long kMaxBytes = 1ll << 31;   // no operand of one launch reaches 2 GiB

int grid_for(const char* who, long long items, int per_block, unsigned* grid) {   // who: "sync" or "sync16"
  const long long g = (items + per_block - 1) / per_block;
  CASYNC_REQUIRE(g >= 1 && g < (1ll << 31), "%s: grid of %lld blocks", who, g);
  *grid = (unsigned)g;
  return CASYNC_OK;
}

}  // namespace
