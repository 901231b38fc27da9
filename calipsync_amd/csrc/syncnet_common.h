// What the two precisions of the SyncNet_color handle share (syncnet.hip: fp32, syncnet_bf16.hip: bf16): the block table of the
// network with its packed layout, the handle itself, and the launchers of syncnet.hip that the bf16 pass calls (their kernels
// stay in lib/obj_sync; the bf16 object instantiates none of them).  Host code only.
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

// ---- syncnet.hip (fp32 NHWC) ----
int launch_sync_to_nchw(const float* in, float* out, int batch, int hw, int c, hipStream_t s);
int launch_sync_embed(const float* in, float* out, int batch, hipStream_t s);

// ---- syncnet_bf16.hip (pointers named void* are bf16, NHWC) ----
int launch_sync16_stem7(const float* x, const float* w, const float* bias, void* out, int batch, int H, int W, hipStream_t s);
// ks 1, 3 or 5 (tile: see the launcher); w [cout][(ky,kx,cin)] bf16; res (optional, bf16) [B Ho Wo][cout] is added before the ReLU; out bf16 or, out_f32, fp32
int launch_sync16_conv(int ks, const void* in, const void* w, const float* bias, const void* res, void* out, bool out_f32, int batch, int H,
                       int W, int cin, int cout, int sh, int sw, int pad, hipStream_t s, int tile = 0);
int launch_sync16_to_nchw(const void* in, float* out, int batch, int hw, int c, hipStream_t s);
// the arena of one bf16 pass of nb frames, and the pass itself (arguments as sync_pass of syncnet.hip; ws 256-B aligned)
int64_t sync16_ws_bytes(int nb, const SyncNet& N);
int sync16_pass(const casync_sync* D, const float* face, const float* audio, int nb, void* ws, int stage, float* out, float* audio_emb,
                float* face_emb, hipStream_t s);
