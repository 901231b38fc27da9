// The forward plan of the CASync U-Net on one MI355X: packed-weight layout, workspace
// arena and the launch sequence that replaces Model.forward (reference
// module/unet.py:314-345).  Mirrors calipsync_amd/arch.py (tests/test_abi.py checks the two
// agree).  Everything is NHWC fp32 inside; NCHW only at the boundary.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "handle.h"

// ------------------------------------------------------------------ error text
static thread_local char g_err[512] = "";
void casync_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* casync_last_error(void) { return g_err; }

// diagnostic: device buffer of 8 x grid words that the GEMM launches of this thread stamp (null = off; see
// casync_debug_gemm_stamps).  Never set on the product path.
static thread_local unsigned long long* g_gemm_stamps = nullptr;

namespace {

// ------------------------------------------------------------------ architecture table
struct IR {  // inverted residual: PW expand -> DW3x3 -> PW project (module/unet.py:8-40)
  const char* prefix;
  int id;         // its weights: UNetLayout::ir[id] (the two audio encoders' conv1 / conv2 share a slot: a layout holds one of them)
  int cin, cout, stride, res, hw_in;
  int w_in = 0;   // frame width when it differs from the height (AudioConvWenet's 16x32 blocks, stride 1 only); 0 = square
  int cexp() const { return cin * 2; }
  int wd() const { return w_in ? w_in : hw_in; }
  bool square() const { return wd() == hw_in; }
  int hw_out() const { return stride == 1 ? hw_in : (hw_in + 2 - 3) / 2 + 1; }
  int wd_out() const { return stride == 1 ? wd() : (wd() + 2 - 3) / 2 + 1; }
};

const IR kDown[4][2] = {
    {{"down1.maxpool_conv.0.double_conv.0", 0, 32, 64, 2, 0, 160}, {"down1.maxpool_conv.0.double_conv.1", 1, 64, 64, 1, 1, 80}},
    {{"down2.maxpool_conv.0.double_conv.0", 2, 64, 128, 2, 0, 80}, {"down2.maxpool_conv.0.double_conv.1", 3, 128, 128, 1, 1, 40}},
    {{"down3.maxpool_conv.0.double_conv.0", 4, 128, 256, 2, 0, 40}, {"down3.maxpool_conv.0.double_conv.1", 5, 256, 256, 1, 1, 20}},
    {{"down4.maxpool_conv.0.double_conv.0", 6, 256, 512, 2, 0, 20}, {"down4.maxpool_conv.0.double_conv.1", 7, 512, 512, 1, 1, 10}}};
const IR kAudio[5] = {{"audio_model.conv1", 8, 32, 64, 1, 0, 32},
                      {"audio_model.conv2", 9, 64, 128, 1, 0, 32},
                      {"audio_model.conv4", 10, 256, 256, 1, 1, 16},
                      {"audio_model.conv6", 11, 512, 512, 1, 1, 10},
                      {"audio_model.conv7", 12, 512, 512, 1, 1, 10}};
// AudioConvWenet (module/unet.py:109-144): conv1 / conv2 are 256 -> 512 -> 256 residual blocks on 16x32 frames; conv4, conv6
// and conv7 are the HuBERT encoder's blocks of the same names (kAudio[2..4])
const IR kAudioW[2] = {{"audio_model.conv1", 8, 256, 256, 1, 1, 16, 32}, {"audio_model.conv2", 9, 256, 256, 1, 1, 16, 32}};
// per-frame floats of the NCHW audio window at the boundary
inline int64_t audio_frame_floats(int mode) { return mode == CASYNC_AUDIO_WENET ? 256ll * 16 * 32 : 32ll * 32 * 32; }
inline bool audio_mode_ok(int mode) { return mode == CASYNC_AUDIO_HUBERT || mode == CASYNC_AUDIO_WENET; }
const IR kFuse[4] = {{"fuse_conv.0.double_conv.0", 13, 1024, 512, 1, 0, 10},
                     {"fuse_conv.0.double_conv.1", 14, 512, 512, 1, 1, 10},
                     {"fuse_conv.1.double_conv.0", 15, 512, 256, 1, 0, 10},
                     {"fuse_conv.1.double_conv.1", 16, 256, 256, 1, 1, 10}};
const IR kUp[4][2] = {
    {{"up1.conv.double_conv.0", 17, 512, 128, 1, 0, 20}, {"up1.conv.double_conv.1", 18, 128, 128, 1, 1, 20}},
    {{"up2.conv.double_conv.0", 19, 256, 64, 1, 0, 40}, {"up2.conv.double_conv.1", 20, 64, 64, 1, 1, 40}},
    {{"up3.conv.double_conv.0", 21, 128, 32, 1, 0, 80}, {"up3.conv.double_conv.1", 22, 32, 32, 1, 1, 80}},
    {{"up4.conv.double_conv.0", 23, 64, 32, 1, 0, 160}, {"up4.conv.double_conv.1", 24, 32, 32, 1, 1, 160}}};
constexpr int kIRs = 25;            // inverted residuals of one network
constexpr int kBlocks = 4;          // attention blocks
constexpr int kKV = 64 + 512;       // per-block [K | V] projection columns
const char* const kAttName[kBlocks] = {"attention_blocks.0", "attention_blocks.1", "attention_blocks.2", "attention_blocks.3"};
const char* const kUpName[4] = {"up1", "up2", "up3", "up4"};

// ------------------------------------------------------------------ packed weights
// The packed buffer of one audio mode and the offset of every tensor in it, resolved once as the table is built: a forward
// builds no name and searches nothing (the casync_packed_* accessors read `packed`).
constexpr int64_t kNoWeight = -1;   // "no such tensor": a bias a GEMM does not add, a tensor the mode does not have
struct UNetLayout {
  struct IRW {
    int64_t pw1_w, pw1_b, dw_w, dw_b, pw2_w, pw2_b;
    // the first block of an Up stage: the two K-halves of its expand matrix as matrices of their own -- [cexp][cin/2] for the
    // upsampled input (applied at the low resolution: upsample and 1x1 conv commute) and for the skip
    int64_t pw1a_w = kNoWeight, pw1b_w = kNoWeight;
  };
  struct Att {
    int64_t p1_w, p1_b, q_w, q_b, p1q_w, p1q_b, gamma, b1_w, b1_b, b1_rs;
  };
  PackedLayout packed;
  IRW ir[kIRs];
  Att att[kBlocks];
  int64_t inc, conv3_w, conv3_b, conv5_w, conv5_b, bn7_s = kNoWeight, bn7_t = kNoWeight, fc1_w, fc1_b, fc2_w, fc2_b, fc2_rs, kv_w, kv_b,
      bn_kx_s, bn_kx_t, outc_w, outc_b;

  explicit UNetLayout(int mode) {
    const bool wenet = mode == CASYNC_AUDIO_WENET;
    auto add = [this](const std::string& n, int64_t size) { return packed.add(n, size); };
    auto add_ir = [&](const IR& b) {
      const std::string p = b.prefix;
      IRW& w = ir[b.id];
      w.pw1_w = add(p + ".pw1.w", (int64_t)b.cexp() * b.cin);
      w.pw1_b = add(p + ".pw1.b", b.cexp());
      w.dw_w = add(p + ".dw.w", 9 * (int64_t)b.cexp());
      w.dw_b = add(p + ".dw.b", b.cexp());
      w.pw2_w = add(p + ".pw2.w", (int64_t)b.cout * b.cexp());
      w.pw2_b = add(p + ".pw2.b", b.cout);
    };
    inc = add("inc.inconv.0.fused", 620);  // [w1T 6x12][b1 12][wd 9x12][bd 12][w2T 12x32][b2 32]
    for (auto& st : kDown)
      for (auto& b : st) add_ir(b);
    add_ir(wenet ? kAudioW[0] : kAudio[0]);
    add_ir(wenet ? kAudioW[1] : kAudio[1]);
    conv3_w = add("audio_model.conv3.w", 256ll * 9 * (wenet ? 256 : 128));  // [N][(ky,kx,cin)]
    conv3_b = add("audio_model.conv3.b", 256);
    add_ir(kAudio[2]);
    conv5_w = add("audio_model.conv5.w", 512ll * 9 * 256);
    conv5_b = add("audio_model.conv5.b", 512);
    add_ir(kAudio[3]);
    add_ir(kAudio[4]);
    if (!wenet) {   // AudioConvWenet ends at conv7: no bn7 / relu7 (module/unet.py:135-144)
      bn7_s = add("audio_model.bn7.s", 512);
      bn7_t = add("audio_model.bn7.t", 512);
    }
    fc1_w = add("mlp_fusion.fc1.w", 1024ll * 1024);
    fc1_b = add("mlp_fusion.fc1.b", 1024);
    fc2_w = add("mlp_fusion.fc2.w", 1024ll * 1024);  // bn2 and bn_tx folded in
    fc2_b = add("mlp_fusion.fc2.b", 1024);
    fc2_rs = add("mlp_fusion.fc2.rs", 1024);         // bn_tx scale on the cat(x5, a) residual
    kv_w = add("att.kv.w", (int64_t)kBlocks * kKV * 512);  // rows: blk0 K(64) V(512), blk1 ...
    kv_b = add("att.kv.b", kBlocks * kKV);
    for (int i = 0; i < kBlocks; ++i) {
      const std::string p = kAttName[i];
      Att& a = att[i];
      a.p1_w = add(p + ".p1.w", 512ll * 1024);
      a.p1_b = add(p + ".p1.b", 512);
      a.q_w = add(p + ".q.w", 64ll * 512);
      a.q_b = add(p + ".q.b", 64);
      // rows 0..511 = p_1, rows 512..575 = query_conv o p_1 composed on the host in float64
      // (module/unet.py:201,209,256,264): q comes out of the p_1 GEMM as 64 extra columns
      a.p1q_w = add(p + ".p1q.w", 576ll * 1024);
      a.p1q_b = add(p + ".p1q.b", 576);
      a.gamma = add(p + ".gamma", 1);
      a.b1_w = add(p + ".b1.w", 1024ll * 512);  // block bn folded in
      a.b1_b = add(p + ".b1.b", 1024);
      a.b1_rs = add(p + ".b1.rs", 1024);        // block bn scale on the tx residual
    }
    bn_kx_s = add("bn_kx.s", 1024);
    bn_kx_t = add("bn_kx.t", 1024);
    for (auto& b : kFuse) add_ir(b);
    for (auto& st : kUp)
      for (auto& b : st) add_ir(b);
    for (auto& st : kUp) {
      ir[st[0].id].pw1a_w = add(std::string(st[0].prefix) + ".pw1a.w", (int64_t)st[0].cexp() * (st[0].cin / 2));
      ir[st[0].id].pw1b_w = add(std::string(st[0].prefix) + ".pw1b.w", (int64_t)st[0].cexp() * (st[0].cin / 2));
    }
    outc_w = add("outc.w", 96);  // [3][32], outc_bn folded in
    outc_b = add("outc.b", 3);
  }
};

// the layout of an audio mode (anything but CASYNC_AUDIO_WENET: the HuBERT one)
const UNetLayout& layout(int mode = CASYNC_AUDIO_HUBERT) {
  static const UNetLayout L[2] = {UNetLayout(CASYNC_AUDIO_HUBERT), UNetLayout(CASYNC_AUDIO_WENET)};
  return L[mode == CASYNC_AUDIO_WENET ? 1 : 0];
}

// ------------------------------------------------------------------ workspace arena
// An activation pointer that knows its element size: `p + n` advances n ELEMENTS of the engine's
// storage type (fp32 or bf16) and it converts to void* at the kernel launchers.
struct Ptr {
  char* p = nullptr;
  int esz = 4;
  Ptr operator+(long long n) const { return Ptr{p + n * esz, esz}; }
  operator void*() const { return p; }
  operator const void*() const { return p; }
};

// How one inverted residual computes its expanded (2x) tensor and the depthwise conv behind it.  THE place that decides it:
// Plan::ir() switches on the answer, the arena sizes E1 / E2 by it and up_mode() asks it what an Up block can take.
enum class Expand {
  Fused,    // ir_fused_kernel: the whole block in one launch, E never leaves LDS
  Rect,     // expand + depthwise in one launch on rectangular frames (AudioConvWenet's 16x32 blocks): whole-frame tiles
  Square,   // expand GEMM whose output tile is whole frames or strips: the depthwise conv runs on the tile in LDS, E never reaches HBM
  Gemm,     // expand GEMM into E1, depthwise E1 -> E2
  None      // bf16 with an upsampled addend that no bf16 kernel takes
};
// `frames` per launch; `ups`: the expand conv runs over the skip half (cin / 2 channels) and adds the upsampled G = W1a . lo of
// an Up block in front of its activation; `extra`: the project GEMM has epilogue work the fused kernel does not do
Expand expand_path(const CasyncOptions& o, const IR& b, int dtype, int frames, bool ups, bool extra = false) {
  const bool f32 = dtype == DT_F32, sq = b.square();
  const int k_in = ups ? b.cin / 2 : b.cin;
  if (!extra && !ups && o.fuse_ir && sq && b.hw_in >= o.fuse_min_hw && ir_fused_supported(b.cin, b.cout, b.stride)) return Expand::Fused;
  // the precision's switch (1: below 40x40 only) and the frames per launch from which whole-frame tiles fill the chip (fp32: from
  // fuse_dw_min = 12, below that they are too few -- B=1 0.92 vs 0.82 ms)
  const int on = f32 ? o.fuse_dw : o.fuse_dw_bf16, whole = f32 ? o.fuse_dw_min : o.fuse_dw_bf16_min;
  if (on && !sq && !ups && frames >= whole && (f32 ? pw_dw_rect_supported : pw_dw_bf16_rect_supported)(b.hw_in, b.wd(), k_in, b.cexp(), b.stride))
    return Expand::Rect;   // (rectangular frames have kernels of their own)
  if (on && sq && (b.hw_in < 40 || on >= 2)) {
    // (fp32 below fuse_dw_deep frames per launch -- round 5 -- the stride-1 blocks take its one-frame tiles with a four-stage ring)
    if (f32 && (pw_dw_deep(b.hw_in, frames, b.stride, ups, k_in) || frames >= (b.hw_in == 40 ? o.fuse_dw_min40 : whole)) &&
        pw_dw_supported(b.hw_in, k_in, b.cexp(), b.stride))
      return Expand::Square;
    if (!f32 && frames >= whole && pw_dw_bf16_supported(b.hw_in, k_in, b.cexp(), b.stride) && (!ups || pw_dw_bf16_takes_ups(b.hw_in, b.stride)))
      return Expand::Square;
  }
  return !f32 && ups ? Expand::None : Expand::Gemm;
}
// (neither the precision nor the frame count reaches the fused arm)
bool ir_is_fused(const CasyncOptions& o, const IR& b) { return expand_path(o, b, DT_F32, 0, false) == Expand::Fused; }
bool up_is_fused(const CasyncOptions& o, const IR& b0) {
  return o.fuse_ir && o.fuse_up && b0.hw_in >= o.fuse_min_hw && ir_fused_up_supported(b0.cin, b0.cout);
}
// How the first inverted residual of an Up stage takes its upsampled half.  ONE predicate for the plan (decode()) and for
// the workspace (max_unfused_expand()): apart, `fuse_up=0` sends up3.0 / up4.0 down the un-fused chain with E1 / E2 sized
// for up2.0.
enum class UpMode {
  CommuteUnfused,   // G = W1a.lo at the low resolution, then the un-fused chain (pw_dw / GEMM + depthwise) adds up(G)
  CommuteFused,     // G = W1a.lo, then ir_fused_kernel<.., UPS = 2>
  FusedLoad,        // ir_fused_kernel<.., UPS = 1>: bilinear taps while loading the A fragments
  Materialise       // upsample2x into the concat buffer, then the block as any other inverted residual
};
UpMode up_mode(const CasyncOptions& o, const IR& b0, int dtype, int batch = 0) {
  const bool f32 = dtype == DT_F32;
  if (up_is_fused(o, b0)) return f32 && o.ups_commute >= 2 ? UpMode::CommuteFused : UpMode::FusedLoad;
  // a block the plain fused kernel takes (fuse_up = 0, fuse_ir = 1) keeps it: upsample first, E never leaves LDS.  bf16 commutes
  // where its expand + depthwise kernel takes the block with the addend (`batch` frames per launch).
  if (!ir_is_fused(o, b0) && (f32 ? o.ups_commute != 0 : o.ups_commute_bf16 && expand_path(o, b0, DT_BF16, batch, true) == Expand::Square))
    return UpMode::CommuteUnfused;
  return UpMode::Materialise;
}
constexpr int kMinLaneBatch = 16;
// skip_early (decode()): small single-lane batches run the skip half of up1.0 / up2.0's expand conv beside the trunk
bool skip_early_batch(const CasyncOptions& o, int batch) {
  return o.skip_early > 0 && batch < o.skip_early && batch < kMinLaneBatch * 2;
}
// Largest expanded (2x) tensor an UN-fused inverted residual of the plan writes, per frame: the E1/E2
// slots are sized for it.  With the fused kernels on (default) that is up2.0's 40x40x512, not the
// 160x160x128 of up4.0 the fused kernel keeps in LDS (19.6 MB per frame less workspace).
int64_t max_unfused_expand(const CasyncOptions& o) {
  int64_t mx = 0;
  auto see = [&](const IR& b, bool fused) {
    if (!fused) mx = std::max<int64_t>(mx, (int64_t)b.hw_in * b.hw_in * b.cexp());
  };
  for (auto& st : kDown)
    for (auto& b : st) see(b, ir_is_fused(o, b));
  for (auto& b : kFuse) see(b, ir_is_fused(o, b));
  for (auto& st : kUp) {   // (dtype-independent: the fp32-only modes never un-fuse a block bf16 would fuse)
    see(st[0], up_is_fused(o, st[0]) || ir_is_fused(o, st[0]));
    see(st[1], ir_is_fused(o, st[1]));
  }
  return mx;
}

struct Arena {
  // per-frame float counts; pointers are filled by bind()
  struct Buf {
    const char* name;
    int64_t per_frame;
    char* p;
  };
  int esz = 4;
  enum Id {
    CAT4, CAT3, CAT2, CAT1, CATA, E1, E2, T0, U4, F, FM, U1, U2, U3, UG,
    A0, AC1, AC2, AC3, AC4, AC5, AC6, AE1, AE2,
    H, TX, OX0, OX1, OX2, OX3, KX, KXF, P1Q, AO, Q, KV, EP1, EP2, A0L, COUNT
  };
  Buf b[COUNT] = {
      {"cat4", 160 * 160 * 64, 0},  {"cat3", 80 * 80 * 128, 0},  {"cat2", 40 * 40 * 256, 0},
      {"cat1", 20 * 20 * 512, 0},   {"catA", 100 * 1024, 0},     {"E1", 160 * 160 * 128, 0},
      {"E2", 160 * 160 * 128, 0},   {"T0", 160 * 160 * 32, 0},   {"U4", 160 * 160 * 32, 0},
      {"F", 100 * 256, 0},          {"FM", 100 * 512, 0},        {"U1", 400 * 128, 0},
      {"U2", 1600 * 64, 0},         {"U3", 6400 * 32, 0},        {"UG", 6400 * 128, 0},   // W1a . lo of an Up block, low res
      {"A0", 1024 * 32, 0},
      {"AC1", 1024 * 64, 0},        {"AC2", 1024 * 128, 0},
      {"AC3", 256 * 256, 0},        {"AC4", 256 * 256, 0},       {"AC5", 100 * 512, 0},
      {"AC6", 100 * 512, 0},        {"AE1", 131072, 0},          {"AE2", 131072, 0},
      {"H", 100 * 1024, 0},         {"TX", 100 * 1024, 0},       {"OX0", 100 * 1024, 0},
      {"OX1", 100 * 1024, 0},       {"OX2", 100 * 1024, 0},      {"OX3", 100 * 1024, 0},
      {"KX", 100 * 1024, 0},        {"KXF", 100 * 1024, 0},      {"P1Q", 100 * 576, 0},
      {"AO", 100 * 512, 0},         {"Q", 100 * 64, 0},          {"KV", 100 * kBlocks * kKV, 0},
      // skip_early: W1b . skip + b of up1.0 (20x20 x 1024) and up2.0 (40x40 x 512), small batches only
      {"EP1", 400 * 1024, 0},       {"EP2", 1600 * 512, 0},
      // wenet, bf16 storage: the low half of the audio window, R(x - R(x)) (encode(): conv1's residual add); last, so that no other
      // buffer moves
      {"A0L", 0, 0}};
  // (the two skip_early buffers exist only for the batches that use them: 4.9 MB per frame)
  // wenet: the audio window is 256 x 16 x 32, conv1 / conv2 write 16x32 x 256 and expand to 16x32 x 512
  Arena(const CasyncOptions& o, int batch, int mode = CASYNC_AUDIO_HUBERT, int esz_ = 4) {
    b[E1].per_frame = b[E2].per_frame = max_unfused_expand(o);
    if (!skip_early_batch(o, batch)) b[EP1].per_frame = b[EP2].per_frame = 0;
    if (mode == CASYNC_AUDIO_WENET) {
      b[A0].per_frame = b[AC1].per_frame = 512 * 256;
      b[AE1].per_frame = b[AE2].per_frame = 512 * 512;
      if (esz_ == 2) b[A0L].per_frame = 512 * 256;
    }
  }
  static int64_t bytes(const CasyncOptions& o, int batch, int esz = 4, int mode = CASYNC_AUDIO_HUBERT) {
    Arena a(o, batch, mode, esz);
    int64_t tot = 0;
    for (auto& x : a.b) tot += (x.per_frame * batch + 63) / 64 * 64;
    return tot * (int64_t)esz;
  }
  void bind(void* base, int batch, int elem_size) {
    esz = elem_size;
    char* p = (char*)base;
    for (auto& x : b) {
      x.p = p;
      p += ((x.per_frame * batch + 63) / 64 * 64) * (int64_t)esz;
    }
  }
  // view of frames [b0, ...) of an arena bound for the whole batch (every buffer is frame-major)
  void slice(int b0) {
    for (auto& x : b) x.p += x.per_frame * (int64_t)b0 * esz;
  }
  Ptr operator[](Id i) const { return Ptr{b[i].p, esz}; }
  // elements per frame of the buffer that starts at `p` (-1: not the start of a buffer)
  int64_t per_frame_of(const Ptr& p) const {
    for (auto& x : b)
      if (x.p == p.p) return x.per_frame;
    return -1;
  }
};

}  // namespace

struct casync_engine {
  int device = 0;
  int dtype = DT_F32;        // activation storage type (DT_BF16: bf16 activations + bf16 GEMM weights)
  int mode = CASYNC_AUDIO_HUBERT;   // audio encoder (fixed at creation): selects the packed layout, the arena and encode()'s branch
  PackedWeights pw;          // fp32: biases, scales, DW / fused-IR weights; the bf16 image (DT_BF16 only): the GEMM matrices
  // stream-K scratch of the GEMMs (gemm.hip): one private region per stream that can run a GEMM
  // (lane x {main, audio}), counters zeroed once here and left zeroed by every launch
  char* sk = nullptr;
  char* sk_ctx(int lane, int aux_stream) const { return sk ? sk + (size_t)(lane * 2 + aux_stream) * kStreamKBytes : nullptr; }
  // second stream per lane for the audio encoder, which is independent of the face encoder until
  // the fusion MLP (module/unet.py:315-321): forked/joined with events inside casync_forward
  // Lanes: the batch is cut into kMaxLanes contiguous sub-batches that run concurrently, lane 0
  // on the caller's stream, the others on engine-owned streams, so one lane's memory-bound
  // kernels and kernel tails overlap another lane's MFMA-bound GEMMs.  Every lane also forks
  // its audio encoder onto its own second stream.
  static constexpr int kMaxLanes = 4;
  hipStream_t lane_s[kMaxLanes] = {};   // [0] unused (caller's stream)
  hipStream_t aux[kMaxLanes] = {};
  hipEvent_t ev_fork[kMaxLanes] = {}, ev_join[kMaxLanes] = {}, ev_done[kMaxLanes] = {}, ev_mid[kMaxLanes] = {};
  hipEvent_t ev_start = nullptr, ev_start2 = nullptr;
  hipEvent_t ev_fwd = nullptr;   // recorded behind this handle's last forward when another handle's forward follows it (FwdGate)
  bool streams_ready = false;
  CasyncOptions opt;         // this handle's switches: process defaults at create, casync_set_option afterwards
  CasyncOptions eff;         // what the forward in progress runs under (run_forward: `opt` + the bf16 large-batch plan)
  const float* W(int64_t off) const { return pw.w + off; }   // off: a member of layout(mode)
  // GEMM weight matrix in the engine's storage type
  const void* WG(int64_t off) const { return dtype == DT_BF16 ? (const void*)(pw.w16 + off) : (const void*)(pw.w + off); }
};

namespace {

__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ in,
                                                          bf16_t* __restrict__ out, long long n) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i < n) st4(out + i, ld4(in + i));
}

}  // namespace

int launch_f32_to_bf16(const float* in, void* out, long long n, hipStream_t s) {
  CASYNC_REQUIRE(in && out && n > 0 && n % 4 == 0, "f32_to_bf16: %lld floats (a positive multiple of 4)", n);
  const long long blocks = (n / 4 + 255) / 256;
  CASYNC_REQUIRE(blocks < (1ll << 31), "f32_to_bf16: too many elements");
  return casync_launch(f32_to_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, static_cast<bf16_t*>(out), n);
}

namespace {

// Short name of a mangled kernel symbol, as tools/kernel_names.py short() writes it ("pw_gemm_kernel<__bf16, 128, 128, 2, 2>"),
// and a port of its decoder: the template arguments of this engine's kernels are float / __bf16 / int / bool literals, any
// other shape keeps the bare name.  (Not a general demangler: binutils' does not know DF16b, the mangling of __bf16.)
std::string kernel_short_name(const char* m) {
  const char* p = strncmp(m, "_ZN12_GLOBAL__N_1", 17) == 0 ? m + 17 : strncmp(m, "_Z", 2) == 0 ? m + 2 : nullptr;
  char* end = nullptr;
  const size_t n = p ? strtoul(p, &end, 10) : 0;
  if (!p || end == p || strlen(end) < n) return m;
  const std::string name(end, n);
  const char* r = end + n;
  if (*r != 'I') return name;
  std::string args;
  for (++r; *r && *r != 'E';) {
    if (!args.empty()) args += ", ";
    if (strncmp(r, "DF16b", 5) == 0) {
      args += "__bf16";
      r += 5;
    } else if (*r == 'f') {
      args += "float";
      ++r;
    } else if (r[0] == 'L' && (r[1] == 'i' || r[1] == 'b')) {
      const char* e = strchr(r, 'E');
      if (!e) return name;
      const std::string v(r + 2, e);
      args += r[1] == 'b' ? (v == "1" ? "true" : "false") : (v[0] == 'n' ? "-" + v.substr(1) : v);
      r = e + 1;
    } else {
      return name;
    }
  }
  return name + "<" + args + ">";
}

// ------------------------------------------------------------------ launch recorder
struct Runner {
  hipStream_t s;
  bool profile = false;
  std::vector<casync_kernel_time> rec;
  std::vector<hipEvent_t> ev;
  int status = CASYNC_OK;

  // f() issues one kernel launch (casync_launch): a profiled row is called prefix + suffix (put together only here, when
  // profiling) and names the kernel it launched
  template <class F>
  void run(const char* prefix, const char* suffix, double flops, double bytes, F&& f) {
    if (status != CASYNC_OK) return;
    if (!profile) {
      status = f();
      return;
    }
    const std::string name = std::string(prefix) + suffix;
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    (void)hipEventRecord(a, s);
    casync_launch_note = CasyncLaunchNote();
    status = f();
    (void)hipEventRecord(b, s);
    ev.push_back(a);
    ev.push_back(b);
    if (status == CASYNC_OK && casync_launch_note.count != 1) {
      casync_set_error("profile: %s issued %u kernel launches, not one", name.c_str(), casync_launch_note.count);
      status = CASYNC_ERR_STATE;
    }
    casync_kernel_time t;
    memset(&t, 0, sizeof(t));
    strncpy(t.name, name.c_str(), sizeof(t.name) - 1);
    if (status == CASYNC_OK) {
      const char* mangled = hipKernelNameRefByPtr(casync_launch_note.kernel, s);
      strncpy(t.kernel, mangled ? kernel_short_name(mangled).c_str() : "?", sizeof(t.kernel) - 1);
    }
    t.flops = flops;
    t.bytes = bytes;
    rec.push_back(t);
  }
  void finish() {
    if (!profile) return;
    // An event pair around a launch also times the command processor's own work between two timestamps (~3-4 us on
    // MI355X), which is not kernel time: rocprofv3's begin/end of the same launches were 10 % shorter than the raw
    // pairs.  Calibrate it on this stream -- the median of 16 pairs with NOTHING between them -- and
    // take it off every figure, so that the HIP-event averages and the rocprofv3 averages of profiles/ agree.
    constexpr int NCAL = 16;
    hipEvent_t cal[2 * NCAL];
    for (int i = 0; i < 2 * NCAL; ++i) {
      (void)hipEventCreate(&cal[i]);
      (void)hipEventRecord(cal[i], s);
    }
    (void)hipStreamSynchronize(s);
    float gaps[NCAL];
    for (int i = 0; i < NCAL; ++i) {
      gaps[i] = 0.f;
      (void)hipEventElapsedTime(&gaps[i], cal[2 * i], cal[2 * i + 1]);
    }
    for (int i = 0; i < 2 * NCAL; ++i) (void)hipEventDestroy(cal[i]);
    std::sort(gaps, gaps + NCAL);
    const float overhead = gaps[NCAL / 2];
    for (size_t i = 0; i < rec.size(); ++i) {
      (void)hipEventElapsedTime(&rec[i].ms, ev[2 * i], ev[2 * i + 1]);
      rec[i].ms_raw = rec[i].ms;
      rec[i].ms = rec[i].ms > overhead ? rec[i].ms - overhead : 0.f;
      (void)hipEventDestroy(ev[2 * i]);
      (void)hipEventDestroy(ev[2 * i + 1]);
    }
  }
};

struct Plan {
  const casync_engine& e;
  Arena ar;
  Runner& r;
  int B;
  hipStream_t aux = nullptr;          // engine's second stream (null = no overlap)
  int lane = 0;                       // selects the stream-K scratch of this lane's streams
  // Stream-K GEMM remainders only when the batch runs as ONE lane: it cuts small-batch latency
  // (B=1 -23 %, B=4 -14 %, B=8 -6 %) and gains 2.6 % at B=64 single-lane, but with two lanes the
  // other lane's kernels already fill a launch's idle CUs and the split only adds traffic
  // (measured -1.1 % fp32 B=64, -1.9 % bf16 B=512).
  bool stream_k = false;
  bool concurrent = false;            // another lane runs beside this one
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_fork2 = nullptr, ev_skip = nullptr;   // skip_early: fork after the encoder, join in front of up1.0's depthwise
  bool skip_early = false;            // set by run_forward for the trunk and the decoder of a forward alike
  // audio source: either the NCHW windows tensor (`audio`) or, when win_feat is set, the whole
  // HuBERT feature array + per-frame indices, gathered on the device (infer_api.py:99-145)
  const float* win_feat = nullptr;
  int win_steps = 0;
  const int* win_idx = nullptr;
  const CasyncOptions& o = e.eff;     // the options of the forward in progress (run_forward)

  const UNetLayout& L = layout(e.mode);   // the offsets W() / WG() take
  using A = Arena;
  int dt() const { return e.dtype; }
  const float* bias(int64_t off) const { return off == kNoWeight ? nullptr : e.W(off); }
  // the stream-K scratch of the stream the next launch goes to, where this plan splits K
  void bind_stream_k(GemmEpilogue& ep) const {
    if (char* ctx = stream_k ? e.sk_ctx(lane, aux && r.s == aux ? 1 : 0) : nullptr) {
      ep.sk_ws = reinterpret_cast<float*>(ctx);
      ep.sk_cnt = reinterpret_cast<unsigned*>(ctx + kStreamKFloats * 4);
    }
  }

  // Send what follows to the second stream, behind what this stream holds so far -> false, status set, where that failed ...
  bool fork_to_aux(hipEvent_t ev, const char* which) {
    if (hipEventRecord(ev, r.s) != hipSuccess || hipStreamWaitEvent(aux, ev, 0) != hipSuccess) {
      casync_set_error("forward: fork onto the %s stream failed", which);
      r.status = CASYNC_ERR_HIP;
      return false;
    }
    r.s = aux;
    return true;
  }
  // ... and come back to `main_s`: `ev` marks the end of the second stream's work for whoever joins it
  void back_from_aux(hipEvent_t ev, hipStream_t main_s) {
    if (r.status == CASYNC_OK && hipEventRecord(ev, aux) != hipSuccess) r.status = CASYNC_ERR_HIP;
    r.s = main_s;
  }

  // GEMM wrapper with work accounting (algorithmic bytes: A + C once, W once).  w, b: offsets of the weight matrix and of
  // the bias (kNoWeight: none)
  void gemm(const char* prefix, const char* suffix, const void* a, int lda, int64_t w, int64_t b, void* c, int ldc, long long m,
            int n, int k, GemmEpilogue epi, double alg_flops = 0) {
    epi.bias = bias(b);
    const double es = dtype_size(dt());
    double bytes = es * ((double)m * k + (double)m * n + (double)n * k);
    if (epi.pre_res) bytes += es * m * n;
    if (epi.post_res) bytes += es * m * n;
    if (epi.acc_out) bytes += 2 * es * m * n;
    bind_stream_k(epi);
    epi.concurrent = concurrent ? 1 : 0;
    epi.stamps = g_gemm_stamps;
    r.run(prefix, suffix, alg_flops > 0 ? alg_flops : 2.0 * m * n * k, bytes,
          [&] { return launch_pw_gemm(a, lda, e.WG(w), c, ldc, (int)m, n, k, epi, r.s, dt()); });
  }

  // Dense 3x3 conv + bias + activation (audio conv3 / conv5: LReLU in AudioConvHubert, module/unet.py:161-168; ReLU and
  // conv3's stride (1, 2) in AudioConvWenet, :119-133) as an implicit GEMM: the ring kernel gathers the taps itself (no
  // im2col buffer).
  void conv3x3(const char* tag, Ptr in, int64_t wt, int64_t b, Ptr out, int h, int w, int cin, int cout, int stride_h, int stride_w,
               int pad, int act) {
    const int ho = (h + 2 * pad - 3) / stride_h + 1, wo = (w + 2 * pad - 3) / stride_w + 1;
    const long long m = (long long)B * ho * wo;
    GemmEpilogue ep;
    ep.act = act;
    ep.bias = bias(b);
    ep.concurrent = concurrent ? 1 : 0;
    bind_stream_k(ep);
    // fp32: position-major rows and the tap walk of conv_skip (gemm.hip): the table was built by casync_create_mode, and the
    // FLOPs booked are the executed ones -- the share of (tile, tap) pairs the launcher walks.  The bf16 engine keeps frame-major
    // rows (its convs are bound by data movement: measured 0.4 % slower at B = 512 with the rows regrouped, profiles/padwork_ab.txt).
    const bool by_position = dt() == DT_F32;
    if (by_position) ep.conv_tab = conv3x3_positions(h, w, stride_h, stride_w, pad);
    long long kt_full = 1, kt_run = 1;
    const int plan_st = !by_position ? CASYNC_OK : ep.conv_tab ? conv3x3_plan(B, h, w, cin, cout, stride_h, stride_w, pad, ep.sk_ws != nullptr, concurrent, dt(), &kt_full, &kt_run)
                                    : CASYNC_ERR_HIP;
    const double es = dtype_size(dt());
    r.run(tag, "", 2.0 * m * cout * 9 * cin * ((double)kt_run / (double)kt_full),
          es * ((double)B * h * w * cin + (double)m * cout + 9.0 * cin * cout), [&] {
      if (plan_st) return plan_st;
      return launch_conv3x3_gemm(in, e.WG(wt), out, cout, B, h, w, cin, cout, stride_h, stride_w, pad, ep, r.s, dt());
    });
  }

  // One inverted-residual block.  in: [B*hw_in^2, cin] (ld_in); out: [B*hw_out^2, cout] (ld_out).
  // `ups` (an Up block's first inverted residual with ups_commute): `in` is only the SKIP half of the concatenated
  // input (k_in = cin / 2 channels, expand matrix pw1b), and ups = W1a . lo at the low resolution, whose bilinear x2
  // upsample the expand conv adds before its activation.
  void ir(const IR& b, Ptr in, int ld_in, Ptr out, int ld_out, Ptr e1, Ptr e2,
          const GemmEpilogue* extra = nullptr, Ptr ups = Ptr{}) {
    const UNetLayout::IRW& w = L.ir[b.id];
    const char* p = b.prefix;
    const long long m_in = (long long)B * b.hw_in * b.wd(), m_out = (long long)B * b.hw_out() * b.wd_out();
    const int k_in = ups.p ? b.cin / 2 : b.cin;
    const int64_t w1 = ups.p ? w.pw1b_w : w.pw1_w;
    const Expand path = expand_path(o, b, dt(), B, ups.p != nullptr, extra != nullptr);
    if (path == Expand::Fused) {
      const double flops = 2.0 * (m_in * (double)b.cin * b.cexp() + 9.0 * m_out * b.cexp() +
                                  (double)m_out * b.cexp() * b.cout);
      r.run(p, ".fused", flops, dtype_size(dt()) * (m_in * (double)b.cin + (double)m_out * b.cout), [&] {
        return launch_ir_fused(in, ld_in, e.WG(w.pw1_w), e.W(w.pw1_b), e.W(w.dw_w), e.W(w.dw_b), e.WG(w.pw2_w), e.W(w.pw2_b), out,
                               ld_out, B, b.hw_in, b.hw_in, b.cin, b.cout, b.stride, b.res, r.s, dt());
      });
      return;
    }
    // the un-fused chain parks the expanded tensor in e1 / e2: they must have been sized for this block (the arena asks
    // expand_path() as this function does; this catches the day it does not)
    if (ar.per_frame_of(e2) < (int64_t)b.hw_in * b.wd() * b.cexp()) {
      casync_set_error("plan: %s un-fused needs %lld expanded elements per frame, the workspace slot holds %lld", b.prefix,
                       (long long)b.hw_in * b.wd() * b.cexp(), (long long)ar.per_frame_of(e2));
      r.status = CASYNC_ERR_STATE;
      return;
    }
    switch (path) {
      case Expand::Rect:
      case Expand::Square:
        // (flops: what this launch executes -- with `ups` the upsampled half was a GEMM at the low resolution)
        r.run(p, ".pw1dw", 2.0 * (m_in * (double)k_in * b.cexp() + 9.0 * m_out * b.cexp()),
              dtype_size(dt()) * (m_in * (double)k_in + (double)b.cexp() * k_in + (double)m_out * b.cexp()), [&] {
          const bool f32 = dt() == DT_F32;
          if (path == Expand::Rect)
            return (f32 ? launch_pw_dw_rect : launch_pw_dw_bf16_rect)(in, ld_in, e.WG(w1), e.W(w.pw1_b), e.W(w.dw_w), e.W(w.dw_b), e2,
                                                                      b.cexp(), B, b.hw_in, b.wd(), k_in, b.cexp(), r.s);
          return (f32 ? launch_pw_dw : launch_pw_dw_bf16)(in, ld_in, e.WG(w1), e.W(w.pw1_b), e.W(w.dw_w), e.W(w.dw_b), e2, b.cexp(), B,
                                                          b.hw_in, b.stride, k_in, b.cexp(), r.s, ups.p, b.cexp());
        });
        break;
      case Expand::None:
        casync_set_error("plan: %s was planned with the commuted upsample but the bf16 expand + depthwise kernel does not take it", b.prefix);
        r.status = CASYNC_ERR_STATE;
        return;
      default: {
        GemmEpilogue ep1;
        ep1.act = 1;
        if (ups.p) {
          ep1.ups_src = ups;
          ep1.ups_ld = b.cexp();
          ep1.ups_h = ep1.ups_w = b.hw_in;
        }
        gemm(p, ".pw1", in, ld_in, w1, w.pw1_b, e1, b.cexp(), m_in, b.cexp(), k_in, ep1);
        r.run(p, ".dw", 2.0 * 9 * m_out * b.cexp(), dtype_size(dt()) * (double)(m_in + m_out) * b.cexp(), [&] {
          return launch_dw3x3(e1, e.W(w.dw_w), e.W(w.dw_b), e2, B, b.hw_in, b.wd(), b.cexp(), b.stride, r.s, dt());
        });
      }
    }
    GemmEpilogue ep2;
    if (extra) ep2 = *extra;
    ep2.act = 1;
    if (b.res) {
      ep2.post_res = in;
      ep2.ld_post = ld_in;
    }
    gemm(p, ".pw2", e2, b.cexp(), w.pw2_w, w.pw2_b, out, ld_out, m_out, b.cout, b.cexp(), ep2);
  }

  // att.kv beside the face encoder (kv_early: 1 = in single-lane runs, where the launch chain is the bound; 2 = always;
  // with two lanes the other lane already fills the chip and the extra stream only competes: -0.5 % at B=64)
  bool kv_in_encode = false;          // set by run_forward for all three phases of a forward alike
  void kv_projection() {
    gemm("att.kv", "", ar[Arena::CATA] + 512, 1024, L.kv_w, L.kv_b, ar[Arena::KV], kBlocks * kKV, (long long)B * 100, kBlocks * kKV, 512,
         GemmEpilogue());
  }

  // Phase 1 of Model.forward: audio encoder || face encoder down to x5 (module/unet.py:315-321).
  void encode(const float* x, const float* audio) {
    Ptr E1 = ar[A::E1], E2 = ar[A::E2], T0 = ar[A::T0];
    // The audio encoder and the face encoder are independent until the fusion MLP; with a
    // second stream they run concurrently and the many small 10x10 / 16x16 audio launches fill
    // CUs the face encoder leaves idle.  Profiling mode keeps everything on one stream.
    const bool overlap = aux && !r.profile;
    hipStream_t main_s = r.s;
    if (overlap && !fork_to_aux(ev_fork, "audio")) return;
    // ---------------- audio encoder (module/unet.py:177-194; AudioConvWenet :135-144)
    Ptr AE1 = ar[A::AE1], AE2 = ar[A::AE2];
    const bool wenet = e.mode == CASYNC_AUDIO_WENET;
    if (wenet) {
      // [B,256,16,32] -> NHWC 16x32 x 256; two residual blocks at 16x32; conv3 (1,2)-strided to 16x16 + ReLU; conv4; conv5
      // + ReLU to 10x10; conv6; conv7 straight into the audio half of cat([x5, a]) (no bn7 / relu7)
      r.run("audio.nchw_to_nhwc", "", 0, (4.0 + dtype_size(dt())) * B * 131072,
            [&] { return launch_nchw_to_nhwc(audio, ar[A::A0], B, 256, 512, r.s, dt()); });
      if (dt() == DT_BF16) {
        // conv1 is a residual block on the network's fp32 input, and the reference keeps that sum in fp32 under bf16 autocast.  The
        // bf16 window A0 feeds the expand conv; the residual add takes the window to 16 mantissa bits, A0 + A0L with A0L =
        // R(x - R(x)): the project GEMM adds A0 behind its activation (post_res), then the running-sum output adds A0L to the fp32
        // value and rounds ONCE into AC1.  (The GEMM's own C output, rounded before A0L, lands in the dead expand slot AE1.)
        r.run("audio.nchw_to_nhwc_lo", "", 0, (4.0 + dtype_size(dt())) * B * 131072,
              [&] { return launch_nchw_to_nhwc(audio, ar[A::A0L], B, 256, 512, r.s, dt(), 1); });
        GemmEpilogue lo;
        lo.acc_in = (const void*)ar[A::A0L];
        lo.acc_out = (void*)ar[A::AC1];
        lo.ld_acc = 256;
        ir(kAudioW[0], ar[A::A0], 256, AE1, 256, AE1, AE2, &lo);
      } else {
        ir(kAudioW[0], ar[A::A0], 256, ar[A::AC1], 256, AE1, AE2);
      }
      ir(kAudioW[1], ar[A::AC1], 256, ar[A::AC2], 256, AE1, AE2);
      conv3x3("audio.conv3", ar[A::AC2], L.conv3_w, L.conv3_b, ar[A::AC3], 16, 32, 256, 256, 1, 2, 1, 2);
    } else {
      if (win_feat)
        r.run("audio.window_gather", "", 0, (4.0 + dtype_size(dt())) * B * 32768,
              [&] { return launch_audio_window_gather(win_feat, win_steps, win_idx, ar[A::A0], B, r.s, dt()); });
      else
        r.run("audio.nchw_to_nhwc", "", 0, (4.0 + dtype_size(dt())) * B * 32768,
              [&] { return launch_nchw_to_nhwc(audio, ar[A::A0], B, 32, 1024, r.s, dt()); });
      ir(kAudio[0], ar[A::A0], 32, ar[A::AC1], 64, AE1, AE2);
      ir(kAudio[1], ar[A::AC1], 64, ar[A::AC2], 128, AE1, AE2);
      conv3x3("audio.conv3", ar[A::AC2], L.conv3_w, L.conv3_b, ar[A::AC3], 32, 32, 128, 256, 2, 2, 1, 1);
    }
    // from the 16x16 x 256 map on the two encoders are one: conv4, conv5 (ReLU in AudioConvWenet, LReLU in AudioConvHubert),
    // conv6, conv7; HuBERT fuses relu7(bn7(x + conv(x))) behind conv7's residual add
    ir(kAudio[2], ar[A::AC3], 256, ar[A::AC4], 256, AE1, AE2);
    conv3x3("audio.conv5", ar[A::AC4], L.conv5_w, L.conv5_b, ar[A::AC5], 16, 16, 256, 512, 2, 2, 3, wenet ? 2 : 1);
    ir(kAudio[3], ar[A::AC5], 512, ar[A::AC6], 512, AE1, AE2);
    GemmEpilogue bn7;
    if (!wenet) {
      bn7.aff_s = e.W(L.bn7_s);
      bn7.aff_t = e.W(L.bn7_t);
    }
    ir(kAudio[4], ar[A::AC6], 512, ar[A::CATA] + 512, 1024, AE1, AE2, wenet ? nullptr : &bn7);
    // K and V projections of the audio features for all four attention blocks in one GEMM (module/unet.py:202-203,
    // 210, 214).  They depend on the audio branch alone, so they run HERE, on the audio stream beside the face encoder,
    // instead of between the fusion MLP and the first attention block (one launch less on the serial chain: at B=8,
    // the reference's own batch, 24 us of 1.26 ms).
    if (kv_in_encode) kv_projection();
    if (overlap) back_from_aux(ev_join, main_s);
    // ---------------- face encoder (module/unet.py:315-319)
    r.run("inc", "", 2.0 * B * 25600 * (72 + 108 + 384),
          (double)B * 25600 * (6 * 4 + 32 * dtype_size(dt())), [&] {
      return launch_inc(x, e.W(L.inc), ar[A::CAT4] + 32, 64, B, r.s, dt());
    });
    struct Skip { Ptr p; int ld; };
    const Skip sk[5] = {{ar[A::CAT4] + 32, 64},   {ar[A::CAT3] + 64, 128}, {ar[A::CAT2] + 128, 256},
                        {ar[A::CAT1] + 256, 512}, {ar[A::CATA], 1024}};
    for (int i = 0; i < 4; ++i) {
      ir(kDown[i][0], sk[i].p, sk[i].ld, T0, kDown[i][0].cout, E1, E2);
      ir(kDown[i][1], T0, kDown[i][1].cin, sk[i + 1].p, sk[i + 1].ld, E1, E2);
    }
    if (overlap && r.status == CASYNC_OK && hipStreamWaitEvent(main_s, ev_join, 0) != hipSuccess) {
      casync_set_error("forward: join of the audio stream failed");
      r.status = CASYNC_ERR_HIP;
    }
  }

  // Phase 2: the 10x10 trunk -- fusion MLP, four attention blocks, fuse_conv (module/unet.py:323-337).
  // All of it is [B*100, C] GEMMs (+ the attention core and four small depthwise convs).
  void trunk() {
    Ptr E1 = ar[A::E1], E2 = ar[A::E2], T0 = ar[A::T0];
    // ---------------- skip_early: W1b . skip + b of up1.0 / up2.0 depend on the encoder alone.  At small batch the
    // forward is one launch chain, so they leave it: they run on the second stream beside the
    // fusion MLP and the attention blocks (forked behind the MLP instead: B=8 1.169 against 1.165 ms), and the decoder's depthwise kernel adds up(W1a . lo) while it stages its slab
    // (dw3x3_ups_lds_kernel) -- at B=8 27 + 9 us become 12 us on the chain at up1.0 and 44 become 22 at up2.0, for ~20 us that
    // the two GEMMs cost the kernels they run beside: 1.182 -> 1.165 ms, B=1 0.760 -> 0.751 ms.
    if (skip_early) {
      const bool fork = aux && !r.profile;
      hipStream_t main_s = r.s;
      if (fork && !fork_to_aux(ev_fork2, "second")) return;
      for (int i = 0; i < 2; ++i) {
        const IR& b0 = kUp[i][0];
        const int c = b0.cin / 2;   // the skip half of the concatenated input
        gemm(b0.prefix, ".pw1b", ar[i ? A::CAT2 : A::CAT1] + c, 2 * c, L.ir[b0.id].pw1b_w, L.ir[b0.id].pw1_b, ar[i ? A::EP2 : A::EP1], b0.cexp(),
             (long long)B * b0.hw_in * b0.hw_in, b0.cexp(), c, GemmEpilogue());
      }
      if (fork) back_from_aux(ev_skip, main_s);
    }
    // ---------------- fusion (module/unet.py:323-326): tx = bn_tx(cat + mlp(cat))
    const long long M10 = (long long)B * 100;
    Ptr CATA = ar[A::CATA];
    {
      GemmEpilogue ep;
      ep.act = 1;
      gemm("mlp.fc1", "", CATA, 1024, L.fc1_w, L.fc1_b, ar[A::H], 1024, M10, 1024, 1024, ep);
      GemmEpilogue ep2;
      ep2.pre_res = CATA;
      ep2.ld_pre = 1024;
      ep2.pre_scale = e.W(L.fc2_rs);
      gemm("mlp.fc2", "", ar[A::H], 1024, L.fc2_w, L.fc2_b, ar[A::TX], 1024, M10, 1024, 1024, ep2);
    }
    if (!kv_in_encode) kv_projection();
    // ---------------- attention blocks (module/unet.py:331-336)
    Ptr ox[4] = {ar[A::OX0], ar[A::OX1], ar[A::OX2], ar[A::OX3]};
    for (int i = 0; i < kBlocks; ++i) {
      const Ptr prev = i ? ox[i - 1] : ar[A::TX];
      const UNetLayout::Att& w = L.att[i];
      const char* p = kAttName[i];
      // ox = p_1(x) lands in columns 0..511 of P1Q (ld 576); q = query_conv(ox) in columns 512..575:
      // either as 64 extra output columns of the same GEMM (weights composed on the host, default) or
      // by the reference's own second GEMM on ox
      Ptr P1 = ar[A::P1Q], Qp = ar[A::P1Q] + 512;
      int ldq = 576;
      if (o.fuse_q) {
        gemm(p, ".p1q", prev, 1024, w.p1q_w, w.p1q_b, P1, 576, M10, 576, 1024, GemmEpilogue(), 2.0 * M10 * (1024.0 * 512 + 512.0 * 64));
      } else {
        gemm(p, ".p1", prev, 1024, w.p1_w, w.p1_b, P1, 576, M10, 512, 1024, GemmEpilogue());
        gemm(p, ".q", P1, 576, w.q_w, w.q_b, ar[A::Q], 64, M10, 64, 512, GemmEpilogue());
        Qp = ar[A::Q];
        ldq = 64;
      }
      Ptr kv = ar[A::KV] + i * kKV;
      r.run(p, ".attn", 2.0 * M10 * 100 * (64 + 512),
            dtype_size(dt()) * (double)M10 * (64 + kKV + 1024), [&] {
        return launch_cross_attention(Qp, ldq, kv, kBlocks * kKV, kv + 64, kBlocks * kKV, P1, 576,
                                      e.W(w.gamma), ar[A::AO], 512, B, r.s, dt());
      });
      GemmEpilogue ep;  // lrelu(bn(b_1(ox) + tx)); kx += ox; last block also lrelu(bn_kx(kx))
      ep.pre_res = ar[A::TX];
      ep.ld_pre = 1024;
      ep.pre_scale = e.W(w.b1_rs);
      ep.act = 1;
      ep.acc_in = i == 0 ? (const void*)ar[A::TX] : (const void*)ar[A::KX];
      ep.acc_out = i == kBlocks - 1 ? (void*)ar[A::KXF] : (void*)ar[A::KX];
      ep.ld_acc = 1024;
      if (i == kBlocks - 1) {
        ep.aff_s = e.W(L.bn_kx_s);
        ep.aff_t = e.W(L.bn_kx_t);
        ep.aff_on_acc = 1;
      }
      gemm(p, ".b1", ar[A::AO], 512, w.b1_w, w.b1_b, ox[i], 1024, M10, 1024, 512, ep);
    }
    // ---------------- fuse_conv (module/unet.py:337)
    ir(kFuse[0], ar[A::KXF], 1024, T0, 512, E1, E2);
    ir(kFuse[1], T0, 512, ar[A::FM], 512, E1, E2);
    ir(kFuse[2], ar[A::FM], 512, T0, 256, E1, E2);
    ir(kFuse[3], T0, 256, ar[A::F], 256, E1, E2);
  }

  // Phase 3: decoder + head (module/unet.py:338-344).
  void decode(float* out) {
    Ptr E1 = ar[A::E1], E2 = ar[A::E2], T0 = ar[A::T0];
    // ---------------- decoder (module/unet.py:338-341)
    Ptr cat[4] = {ar[A::CAT1], ar[A::CAT2], ar[A::CAT3], ar[A::CAT4]};
    Ptr uo[4] = {ar[A::U1], ar[A::U2], ar[A::U3], ar[A::U4]};
    for (int i = 0; i < 4; ++i) {
      const IR& b0 = kUp[i][0];
      const Ptr lo = i ? uo[i - 1] : ar[A::F];
      const int hw = b0.hw_in / 2, c = b0.cin / 2, cc = b0.cin;   // the low resolution, its channels (= the skip's), the concat width
      const double m = (double)B * b0.hw_in * b0.hw_in;           // rows of the stage
      const UNetLayout::IRW& w = L.ir[b0.id];
      const char* p = b0.prefix;
      const UpMode mode = up_mode(o, b0, dt(), B);
      // upsample and 1x1 conv commute: the upsampled half of the expand conv runs on the LOW-resolution tensor
      // (a quarter of the pixels: 37.5 % of this GEMM's multiply-adds never happen), the consumer adds its bilinear
      // x2 upsample before the activation.  Every launch books the flops it executes.
      if (mode == UpMode::CommuteUnfused || mode == UpMode::CommuteFused)
        gemm(p, ".pw1a", lo, c, w.pw1a_w, kNoWeight, ar[A::UG], b0.cexp(), (long long)B * hw * hw, b0.cexp(), c, GemmEpilogue());
      if (mode == UpMode::CommuteUnfused) {
        if (skip_early && i < 2) {
          // the skip half is already there (trunk()): depthwise over LReLU(pre + up(G)), then the project GEMM
          if (i == 0 && aux && !r.profile && hipStreamWaitEvent(r.s, ev_skip, 0) != hipSuccess) {
            casync_set_error("forward: join of the second stream failed");
            r.status = CASYNC_ERR_HIP;
            return;
          }
          const float* pre = (const float*)ar[i == 0 ? A::EP1 : A::EP2].p;
          r.run(p, ".dwups", 2.0 * 9 * m * b0.cexp(), 4.0 * (m * b0.cexp() * 2 + m / 4 * b0.cexp()), [&] {
            return launch_dw3x3_ups(pre, (const float*)ar[A::UG].p, b0.cexp(), e.W(w.dw_w), e.W(w.dw_b), (float*)E2.p, B, 2 * hw, 2 * hw,
                                    b0.cexp(), r.s);
          });
          GemmEpilogue ep2;
          ep2.act = 1;
          gemm(p, ".pw2", E2, b0.cexp(), w.pw2_w, w.pw2_b, T0, b0.cout, (long long)m, b0.cout, b0.cexp(), ep2);
        } else {
          ir(b0, cat[i] + c, cc, T0, b0.cout, E1, E2, nullptr, ar[A::UG]);
        }
      } else if (mode == UpMode::CommuteFused) {
        // the same commutation inside the fused kernel: the fused block runs its expand over the skip half only and adds
        // up(G) chunk by chunk from LDS
        r.run(p, ".upfused", 2.0 * m * (c * b0.cexp() + 9.0 * b0.cexp() + b0.cexp() * b0.cout),
              4.0 * (m / 4 * b0.cexp() + m * c + m * b0.cout), [&] {
                return launch_ir_fused_upg((const float*)ar[A::UG].p, b0.cexp(), (const float*)(cat[i] + c).p, cc, e.W(w.pw1b_w),
                                           e.W(w.pw1_b), e.W(w.dw_w), e.W(w.dw_b), e.W(w.pw2_w), e.W(w.pw2_b), (float*)T0.p, b0.cout, B,
                                           2 * hw, 2 * hw, b0.cin, b0.cout, r.s);
              });
      } else if (mode == UpMode::FusedLoad) {
        // bilinear x2 folded into the fused block's input load: up(x) is never materialised
        r.run(p, ".upfused", 2.0 * m * (b0.cin * b0.cexp() + 9.0 * b0.cexp() + b0.cexp() * b0.cout),
              dtype_size(dt()) * (m / 4 * c + m * c + m * b0.cout), [&] {
                return launch_ir_fused_up(lo, c, c, cat[i], cc, e.WG(w.pw1_w), e.W(w.pw1_b), e.W(w.dw_w), e.W(w.dw_b), e.WG(w.pw2_w),
                                          e.W(w.pw2_b), T0, b0.cout, B, 2 * hw, 2 * hw, b0.cin, b0.cout, r.s, dt());
              });
      } else {
        r.run(kUpName[i], ".bilinear", 0, dtype_size(dt()) * (double)B * hw * hw * c * 5, [&] {
          return launch_upsample2x(lo, cat[i], cc, B, hw, hw, c, r.s, dt());
        });
        ir(b0, cat[i], cc, T0, b0.cout, E1, E2);
      }
      ir(kUp[i][1], T0, kUp[i][1].cin, uo[i], kUp[i][1].cout, E1, E2);
    }
    // ---------------- head (module/unet.py:342-344)
    r.run("outc", "", 2.0 * B * 25600 * 96, (double)B * 25600 * (32 * dtype_size(dt()) + 12), [&] {
      return launch_outc(ar[A::U4], 32, e.W(L.outc_w), e.W(L.outc_b), out, B, r.s, dt());
    });
  }
};

int check_forward_args(casync_handle h, const float* x, const float* a, float* out, int batch,
                       void* ws, int64_t ws_bytes) {
  CASYNC_REQUIRE(h, "null handle");
  CASYNC_REQUIRE(x && a && out && ws, "forward: null pointer");
  CASYNC_REQUIRE(batch > 0 && batch <= 8192, "forward: batch %d out of range [1, 8192]", batch);
  if (!h->pw.w) {
    casync_set_error("forward: weights not loaded");
    return CASYNC_ERR_STATE;
  }
  if (ws_bytes < Arena::bytes(h->opt, batch, dtype_size(h->dtype), h->mode)) {
    casync_set_error("forward: workspace %lld B < required %lld B", (long long)ws_bytes,
                     (long long)Arena::bytes(h->opt, batch, dtype_size(h->dtype), h->mode));
    return CASYNC_ERR_STATE;
  }
  CASYNC_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)out % 16) == 0 &&
                     ((uintptr_t)ws % 256) == 0,
                 "forward: pointers must be 16-B aligned (workspace 256-B)");
  return CASYNC_OK;
}

}  // namespace

// ====================================================================== C ABI
namespace {
// Forwards of DIFFERENT handles on one device do not overlap on the GPU (round 6).  Two models forwarding at the same time
// from two host threads -- an fp32 and a bf16 one -- produced sporadic wrong 2 x 16-pixel patches in the fp32 model's up3 / up4
// outputs (tools/experiments/two_models.py: up to 30 of 30 forwards; profiles/r6_two_models.txt).  Traced to packed fp32
// instructions at two sites (the fused Up block's G accumulation, ups_lerp()) returning wrong values while another wave of the
// SIMD executes bf16 matrix instructions; both sites are scalar now and the pair is clean with this gate switched off.  The
// gate stays as a second line -- the operand pattern the hardware trips on was not characterised: a forward starts behind
// the previous forward of any OTHER handle on the device: the gate is held while a forward is enqueued; a forward that finds another
// handle's forward in front of it records an event at the end of THAT forward's stream (everything of it is enqueued by then)
// and waits for it.  A process with one model never records or waits: one uncontended lock per forward (an event behind every
// forward cost 4 us per forward at B = 8).
struct FwdGate {
  std::mutex m;
  const void* last = nullptr;       // the handle (U-Net or HuBERT) whose forward was enqueued last on this device ...
  hipEvent_t* last_ev = nullptr;    // ... its event slot ...
  hipStream_t last_stream = nullptr;   // ... and the caller's stream it ended on (its lanes join there before it returns)
};
FwdGate& fwd_gate(int device) {
  static FwdGate gates[64];
  return gates[device < 0 || device >= 64 ? 0 : device];
}
struct StreamPool {
  std::mutex m;
  hipStream_t lane[casync_engine::kMaxLanes] = {};   // [0] unused (caller's stream)
  hipStream_t aux[casync_engine::kMaxLanes] = {};
};
StreamPool& stream_pool(int device) {
  static StreamPool pools[64];
  return pools[device < 0 || device >= 64 ? 0 : device];
}
}  // namespace

int casync_gate_enter(int device, const void* owner, hipEvent_t* ev, hipStream_t caller, std::unique_lock<std::mutex>* lock) {
  FwdGate& gate = fwd_gate(device);
  *lock = std::unique_lock<std::mutex>(gate.m);
  static const bool gate_off = getenv("CASYNC_NO_FWD_GATE") != nullptr;   // diagnosis only (tools/experiments/two_models.py)
  if (!gate_off && gate.last && gate.last != owner) {
    if (!*gate.last_ev) CASYNC_CHECK_HIP(hipEventCreateWithFlags(gate.last_ev, hipEventDisableTiming));
    if (hipEventRecord(*gate.last_ev, gate.last_stream) == hipSuccess) {
      CASYNC_CHECK_HIP(hipStreamWaitEvent(caller, *gate.last_ev, 0));
    } else {                          // (the other forward's stream is gone: its work is done or the device will tell)
      (void)hipGetLastError();
      CASYNC_CHECK_HIP(hipDeviceSynchronize());
    }
  }
  gate.last = owner;
  gate.last_ev = ev;
  gate.last_stream = caller;
  return CASYNC_OK;
}

void casync_gate_forget(int device, const void* owner, hipEvent_t* ev) {
  FwdGate& gate = fwd_gate(device);
  std::lock_guard<std::mutex> lock(gate.m);
  if (gate.last == owner) gate.last = nullptr, gate.last_ev = nullptr;
  if (*ev) { (void)hipEventSynchronize(*ev); (void)hipEventDestroy(*ev); *ev = nullptr; }
}

extern "C" {

int casync_abi_version(void) { return CASYNC_ABI_VERSION; }
int casync_packed_count(void) { return layout().packed.count(); }
const char* casync_packed_name(int i) { return layout().packed.name(i); }
int64_t casync_packed_offset(int i) { return layout().packed.offset(i); }
int64_t casync_packed_size(int i) { return layout().packed.size(i); }
int64_t casync_packed_total(void) { return layout().packed.total; }
int casync_packed_count_m(int mode) { return audio_mode_ok(mode) ? layout(mode).packed.count() : 0; }
const char* casync_packed_name_m(int mode, int i) { return audio_mode_ok(mode) ? layout(mode).packed.name(i) : nullptr; }
int64_t casync_packed_offset_m(int mode, int i) { return audio_mode_ok(mode) ? layout(mode).packed.offset(i) : -1; }
int64_t casync_packed_size_m(int mode, int i) { return audio_mode_ok(mode) ? layout(mode).packed.size(i) : -1; }
int64_t casync_packed_total_m(int mode) { return audio_mode_ok(mode) ? layout(mode).packed.total : -1; }
int64_t casync_workspace_bytes(int batch) { return casync_workspace_bytes_dt(batch, DT_F32); }
int64_t casync_workspace_bytes_dt(int batch, int dtype) {
  return batch > 0 && (dtype == DT_F32 || dtype == DT_BF16)
             ? Arena::bytes(casync_default_options(), batch, dtype_size(dtype)) : -1;
}
int64_t casync_workspace_bytes_h(casync_handle h, int batch) {
  return h && batch > 0 ? Arena::bytes(h->opt, batch, dtype_size(h->dtype), h->mode) : -1;
}

int casync_set_option(casync_handle h, const char* name, int value) {
  int* slot = nullptr;
  const int st = casync_option_ref(h ? h->opt : casync_default_options(), name, &slot);
  if (st != CASYNC_OK) return st;
  if (!strcmp(name, "gemm_cfg") && value >= 5) {
    casync_set_error("option gemm_cfg=%d: tile configurations are 0..4 (-1 = cost model)", value);
    return CASYNC_ERR_ARG;
  }
  *slot = value;
  return CASYNC_OK;
}
int casync_get_option(casync_handle h, const char* name, int* value) {
  CASYNC_REQUIRE(value, "get_option: null out");
  int* slot = nullptr;
  const int st = casync_option_ref(h ? h->opt : casync_default_options(), name, &slot);
  if (st == CASYNC_OK) *value = *slot;
  return st;
}

int casync_create(int device_id, casync_handle* out) { return casync_create_ex(device_id, DT_F32, out); }

int casync_create_ex(int device_id, int dtype, casync_handle* out) {
  return casync_create_mode(device_id, dtype, CASYNC_AUDIO_HUBERT, out);
}

int casync_create_mode(int device_id, int dtype, int audio_mode, casync_handle* out) {
  CASYNC_REQUIRE(out, "create: null out");
  CASYNC_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "create: dtype %d (0 = fp32, 1 = bf16)", dtype);
  CASYNC_REQUIRE(audio_mode_ok(audio_mode), "create: audio mode %d (0 = hubert, 1 = wenet)", audio_mode);
  if (int st = casync_require_gfx950("create", device_id)) return st;
  casync_engine* e = new casync_engine();
  e->device = device_id;
  e->dtype = dtype;
  e->mode = audio_mode;
  e->opt = casync_default_options();   // the environment was read once; this handle keeps its own copy
  {
    DeviceGuard guard(device_id);
    const size_t bytes = (size_t)casync_engine::kMaxLanes * 2 * kStreamKBytes;
    hipError_t err = guard.err;
    if (err == hipSuccess) err = hipMalloc((void**)&e->sk, bytes);
    if (err == hipSuccess) err = hipMemset(e->sk, 0, bytes);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) {
      casync_set_error("create: stream-K scratch (%zu bytes): %s", bytes, hipGetErrorString(err));
      if (e->sk) (void)hipFree(e->sk);
      delete e;
      return CASYNC_ERR_HIP;
    }
    // the position tables of audio conv3 / conv5 (Plan::conv3x3, fp32), so that no forward allocates or copies
    const bool wenet = audio_mode == CASYNC_AUDIO_WENET;
    if (dtype == DT_F32 && !((wenet ? conv3x3_positions(16, 32, 1, 2, 1) : conv3x3_positions(32, 32, 2, 2, 1)) && conv3x3_positions(16, 16, 2, 2, 3))) {
      (void)hipFree(e->sk);
      delete e;
      return CASYNC_ERR_HIP;
    }
  }
  *out = e;
  return CASYNC_OK;
}

void casync_destroy(casync_handle h) {
  if (!h) return;
  DeviceGuard guard(h->device);
  {
    casync_gate_forget(h->device, h, &h->ev_fwd);
  }
  if (h->streams_ready) {
    for (int l = 0; l < casync_engine::kMaxLanes; ++l) {
      if (h->lane_s[l]) (void)hipStreamSynchronize(h->lane_s[l]);   // (the streams belong to the process-wide pool: drained, not destroyed)
      if (h->aux[l]) (void)hipStreamSynchronize(h->aux[l]);
      if (h->ev_fork[l]) (void)hipEventDestroy(h->ev_fork[l]);
      if (h->ev_join[l]) (void)hipEventDestroy(h->ev_join[l]);
      if (h->ev_done[l]) (void)hipEventDestroy(h->ev_done[l]);
      if (h->ev_mid[l]) (void)hipEventDestroy(h->ev_mid[l]);
    }
    if (h->ev_start) (void)hipEventDestroy(h->ev_start);
    if (h->ev_start2) (void)hipEventDestroy(h->ev_start2);
  }
  h->pw.release();
  if (h->sk) (void)hipFree(h->sk);
  delete h;
}

int casync_load_weights_host(casync_handle h, const float* packed, int64_t n_floats) {
  CASYNC_REQUIRE(h, "load_weights: null");
  return h->pw.load_host("load_weights", h->device, packed, n_floats, layout(h->mode).packed.total, h->dtype == DT_BF16);
}

int casync_load_weights_device(casync_handle h, const float* packed_dev, int64_t n_floats) {
  CASYNC_REQUIRE(h, "load_weights_device: null");
  return h->pw.adopt_device("load_weights_device", h->device, packed_dev, n_floats, layout(h->mode).packed.total, h->dtype == DT_BF16);
}

// The engine's own streams are PROCESS-WIDE, one set per device, created as they are first needed (lane streams before
// audio streams), and every handle borrows them.  Round 6: with a set per handle a second model in the process ran 7 %
// slower than the first (bf16 B = 512: 45.7 k against 42.8 k frames/s, tools/experiments/bf16_after_fp32.py) -- the runtime
// multiplexes a process's streams onto a few hardware queues, so the second model's lanes landed on queues that already
// carried the first model's and serialised behind each other; `bench.py`'s bf16 leg inside the fp32 run read 42 k for the
// same reason.  Streams only order work: two handles that share them stay correct (every forward orders itself with its
// handle's own events), two forwards running at the same time share the queues -- as they did before.

static int ensure_streams(casync_handle h, int lanes, bool need_aux) {   // caller holds a DeviceGuard for h->device
  if (!h->streams_ready) {
    CASYNC_CHECK_HIP(hipEventCreateWithFlags(&h->ev_start, hipEventDisableTiming));
    CASYNC_CHECK_HIP(hipEventCreateWithFlags(&h->ev_start2, hipEventDisableTiming));
    for (int l = 0; l < casync_engine::kMaxLanes; ++l) {
      CASYNC_CHECK_HIP(hipEventCreateWithFlags(&h->ev_fork[l], hipEventDisableTiming));
      CASYNC_CHECK_HIP(hipEventCreateWithFlags(&h->ev_join[l], hipEventDisableTiming));
      CASYNC_CHECK_HIP(hipEventCreateWithFlags(&h->ev_done[l], hipEventDisableTiming));
      CASYNC_CHECK_HIP(hipEventCreateWithFlags(&h->ev_mid[l], hipEventDisableTiming));
    }
    h->streams_ready = true;
  }
  bool missing = false;
  for (int l = 0; l < lanes; ++l) missing |= (l && !h->lane_s[l]) || (need_aux && !h->aux[l]);
  if (!missing) return CASYNC_OK;
  StreamPool& pool = stream_pool(h->device);
  std::lock_guard<std::mutex> lock(pool.m);
  for (int l = 1; l < lanes; ++l) {
    if (!pool.lane[l]) CASYNC_CHECK_HIP(hipStreamCreateWithFlags(&pool.lane[l], hipStreamNonBlocking));
    h->lane_s[l] = pool.lane[l];
  }
  if (need_aux)
    for (int l = 0; l < lanes; ++l) {
      if (!pool.aux[l]) CASYNC_CHECK_HIP(hipStreamCreateWithFlags(&pool.aux[l], hipStreamNonBlocking));
      h->aux[l] = pool.aux[l];
    }
  return CASYNC_OK;
}

// Lanes: from 2 x 16 frames up the batch is cut into `lanes` contiguous sub-batches that run
// concurrently (lane 0 on the caller's stream), so one lane's memory-bound kernels and kernel tails
// overlap another lane's MFMA-bound GEMMs; below that one lane with stream-K GEMM remainders
// (tools/latency_sweep.py, one lane vs two: B=8 +19 %, B=24 +4 %, B=32 -3.5 %, B=96 -3.4 %).
// trunk_lanes = 1 ("hybrid"): the lanes join before the fusion MLP, the 10x10 trunk (all GEMMs with
// M = B*100 rows) runs once over the whole batch with stream-K remainders, and the lanes fork again
// for the decoder.

struct FwdArgs {
  const float* x;
  const float* a;        // NCHW windows (null when `feat` is set)
  const float* feat;     // whole HuBERT array + per-frame indices, gathered on the device
  int n_steps;
  const int* idx;
  float* out;
  int batch;
  void* ws;
};

// The launch sequence of one forward.  prof == null: enqueue on the caller's stream + engine streams,
// no host sync.  prof != null: the SAME launches (same lanes, sub-batches, kernels, grids) serialised
// on the caller's stream with an event pair around each; synchronises.
static int run_forward(casync_handle h, const FwdArgs& A, hipStream_t caller, std::vector<casync_kernel_time>* prof) {
  // the options this forward runs under: the handle's, plus -- bf16 engine, from `bf16_plan` frames -- the large-batch plan
  // measured in round 6 (profiles/r6_ab_bf16_plan.txt: B = 512 43.65 -> 45.94 k frames/s, B = 128 +0.8 %): three lanes, the
  // 128x128 GEMM tile on the two-stage ring, the audio encoder on its lane's own stream
  h->eff = h->opt;
  if (h->dtype == DT_BF16 && h->opt.bf16_plan > 0 && A.batch >= h->opt.bf16_plan) {
    h->eff.lanes = h->opt.lanes == 2 ? 3 : h->opt.lanes;     // (a caller who set another lane count keeps it)
    h->eff.gemm_ring128 = 1;
    h->eff.overlap = 0;
  }
  const CasyncOptions& o = h->eff;
  CasyncOptScope scope(&h->eff);
  DeviceGuard guard(h->device);
  CASYNC_CHECK_HIP(guard.err);
  const bool serial = prof != nullptr;
  std::unique_lock<std::mutex> gate_lock;          // held until this forward is enqueued
  if (int st = casync_gate_enter(h->device, h, &h->ev_fwd, caller, &gate_lock)) return st;
  const bool overlap = o.overlap != 0 && !serial;
  int lanes = o.lanes < 1 ? 1 : (o.lanes > casync_engine::kMaxLanes ? casync_engine::kMaxLanes : o.lanes);
  if (A.batch < kMinLaneBatch * lanes) lanes = 1;  // small batches are latency-bound: cutting them only adds launches
  const bool hybrid = lanes > 1 && o.trunk_lanes == 1;
  if (overlap || lanes > 1) {
    const int st = ensure_streams(h, lanes, overlap);
    if (st != CASYNC_OK) return st;
  }
  const int esz = dtype_size(h->dtype);
  bool forked = false;
  // On an error after work went to the engine's own streams, drain them before returning: the caller
  // will drop the workspace, and torch's allocator only knows about the caller's stream.
  auto fail = [&](int st) {
    if (forked)
      for (int l = 0; l < casync_engine::kMaxLanes; ++l) {
        if (h->lane_s[l]) (void)hipStreamSynchronize(h->lane_s[l]);
        if (h->aux[l]) (void)hipStreamSynchronize(h->aux[l]);
      }
    return st;
  };
#define FWD_HIP(expr)                                                                           \
  do {                                                                                          \
    hipError_t e__ = (expr);                                                                    \
    if (e__ != hipSuccess) {                                                                    \
      casync_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__));   \
      return fail(CASYNC_ERR_HIP);                                                              \
    }                                                                                           \
  } while (0)

  int b0s[casync_engine::kMaxLanes], bls[casync_engine::kMaxLanes];
  for (int l = 0, b0 = 0; l < lanes; ++l) {
    bls[l] = A.batch / lanes + (l < A.batch % lanes ? 1 : 0);
    if (lanes == 2 && o.lane_skew > 0 && o.lane_skew < A.batch / 2) bls[l] += l == 0 ? o.lane_skew : -o.lane_skew;
    b0s[l] = b0;
    b0 += bls[l];
  }
  auto lane_stream = [&](int l) { return serial || l == 0 ? caller : h->lane_s[l]; };
  // one phase of one lane (or of the whole batch: l = 0, b0 = 0, bl = batch)
  auto run_phase = [&](int phase, int l, int b0, int bl, bool stream_k, bool concurrent) -> int {
    Runner r;
    r.s = lane_stream(l);
    r.profile = serial;
    Plan p{*h, Arena(o, A.batch, h->mode, esz), r, bl};
    p.lane = l;
    p.kv_in_encode = o.kv_early >= 2 || (o.kv_early == 1 && lanes == 1);
    p.skip_early = lanes == 1 && h->dtype == DT_F32 && skip_early_batch(o, A.batch) &&
                   up_mode(o, kUp[0][0], DT_F32) == UpMode::CommuteUnfused && up_mode(o, kUp[1][0], DT_F32) == UpMode::CommuteUnfused;
    p.stream_k = stream_k;
    p.concurrent = concurrent;
    p.ar.bind(A.ws, A.batch, esz);
    p.ar.slice(b0);
    if (overlap) {
      p.aux = h->aux[l];
      p.ev_fork = h->ev_fork[l];
      p.ev_join = h->ev_join[l];
      p.ev_fork2 = h->ev_mid[l];     // (lane 0's ev_mid / ev_done are free in a single-lane forward)
      p.ev_skip = h->ev_done[l];
      forked = true;
    }
    if (A.feat) {
      p.win_feat = A.feat;
      p.win_steps = A.n_steps;
      p.win_idx = A.idx + b0;
    }
    if (phase == 0) p.encode(A.x + (size_t)b0 * 6 * 160 * 160, A.feat ? nullptr : A.a + (size_t)b0 * audio_frame_floats(h->mode));
    else if (phase == 1) p.trunk();
    else p.decode(A.out + (size_t)b0 * 3 * 160 * 160);
    r.finish();
    if (prof) prof->insert(prof->end(), r.rec.begin(), r.rec.end());
    return r.status;
  };

  if (lanes > 1 && !serial) {
    FWD_HIP(hipEventRecord(h->ev_start, caller));
    for (int l = 1; l < lanes; ++l) FWD_HIP(hipStreamWaitEvent(h->lane_s[l], h->ev_start, 0));
    forked = true;
  }
  const bool conc = lanes > 1;
  const bool lane_sk = !conc || o.lane_streamk != 0;
  for (int l = 0; l < lanes; ++l)
    if (int st = run_phase(0, l, b0s[l], bls[l], lane_sk, conc)) return fail(st);
  if (hybrid) {
    if (!serial)
      for (int l = 1; l < lanes; ++l) {
        FWD_HIP(hipEventRecord(h->ev_mid[l], h->lane_s[l]));
        FWD_HIP(hipStreamWaitEvent(caller, h->ev_mid[l], 0));
      }
    if (int st = run_phase(1, 0, 0, A.batch, true, false)) return fail(st);
    if (!serial) {
      FWD_HIP(hipEventRecord(h->ev_start2, caller));
      for (int l = 1; l < lanes; ++l) FWD_HIP(hipStreamWaitEvent(h->lane_s[l], h->ev_start2, 0));
    }
  } else {
    for (int l = 0; l < lanes; ++l)
      if (int st = run_phase(1, l, b0s[l], bls[l], lane_sk, conc)) return fail(st);
  }
  for (int l = 0; l < lanes; ++l)
    if (int st = run_phase(2, l, b0s[l], bls[l], lane_sk, conc)) return fail(st);
  if (lanes > 1 && !serial)
    for (int l = 1; l < lanes; ++l) {
      FWD_HIP(hipEventRecord(h->ev_done[l], h->lane_s[l]));
      FWD_HIP(hipStreamWaitEvent(caller, h->ev_done[l], 0));
    }
#undef FWD_HIP
  return CASYNC_OK;
}

int casync_forward(casync_handle h, const float* x, const float* a, float* out, int batch, void* ws,
                   int64_t ws_bytes, casync_stream stream) {
  int st = check_forward_args(h, x, a, out, batch, ws, ws_bytes);
  if (st != CASYNC_OK) return st;
  return run_forward(h, FwdArgs{x, a, nullptr, 0, nullptr, out, batch, ws}, (hipStream_t)stream, nullptr);
}

int casync_forward_windows(casync_handle h, const float* x, const float* features, int n_steps,
                           const int32_t* frame_idx, float* out, int batch, void* ws, int64_t ws_bytes,
                           casync_stream stream) {
  CASYNC_REQUIRE(!h || h->mode == CASYNC_AUDIO_HUBERT,
                 "forward_windows: the device window gather builds HuBERT windows; a wenet handle takes its [B,256,16,32] audio "
                 "through casync_forward");
  CASYNC_REQUIRE(features && frame_idx && n_steps > 0, "forward_windows: null features / indices");
  CASYNC_REQUIRE(((uintptr_t)features % 16) == 0, "forward_windows: features must be 16-B aligned");
  int st = check_forward_args(h, x, features, out, batch, ws, ws_bytes);
  if (st != CASYNC_OK) return st;
  return run_forward(h, FwdArgs{x, nullptr, features, n_steps, frame_idx, out, batch, ws}, (hipStream_t)stream, nullptr);
}

int casync_profile_forward(casync_handle h, const float* x, const float* a, float* out, int batch,
                           void* ws, int64_t ws_bytes, casync_stream stream, casync_kernel_time* res,
                           int cap) {
  int st = check_forward_args(h, x, a, out, batch, ws, ws_bytes);
  if (st != CASYNC_OK) return st;
  CASYNC_REQUIRE(res && cap > 0, "profile_forward: null result buffer");
  std::vector<casync_kernel_time> rec;
  st = run_forward(h, FwdArgs{x, a, nullptr, 0, nullptr, out, batch, ws}, (hipStream_t)stream, &rec);
  if (st != CASYNC_OK) return st;
  int n = 0;
  for (size_t i = 0; i < rec.size() && n < cap; ++i) res[n++] = rec[i];
  return n;
}

int64_t casync_tap(casync_handle h, const char* name, int batch, void* ws, void* dst, int64_t dst_floats,
                   casync_stream stream) {
  CASYNC_REQUIRE(h && name && ws && dst && batch > 0, "tap: bad args");
  Arena ar(h->opt, batch, h->mode, dtype_size(h->dtype));
  ar.bind(ws, batch, dtype_size(h->dtype));
  using A = Arena;
  struct T { const char* n; Ptr p; int ld, c, rows; };
  const bool wenet = h->mode == CASYNC_AUDIO_WENET;
  const T taps[] = {
      {"x1", ar[A::CAT4] + 32, 64, 32, 25600},  {"x2", ar[A::CAT3] + 64, 128, 64, 6400},
      {"x3", ar[A::CAT2] + 128, 256, 128, 1600}, {"x4", ar[A::CAT1] + 256, 512, 256, 400},
      {"x5", ar[A::CATA], 1024, 512, 100},      {"a", ar[A::CATA] + 512, 1024, 512, 100},
      {"tx", ar[A::TX], 1024, 1024, 100},       {"kx", ar[A::KXF], 1024, 1024, 100},
      {"att0", ar[A::OX0], 1024, 1024, 100},    {"att1", ar[A::OX1], 1024, 1024, 100},
      {"att2", ar[A::OX2], 1024, 1024, 100},    {"att3", ar[A::OX3], 1024, 1024, 100},
      {"fuse", ar[A::F], 256, 256, 100},        {"u1", ar[A::U1], 128, 128, 400},
      {"u2", ar[A::U2], 64, 64, 1600},          {"u3", ar[A::U3], 32, 32, 6400},
      {"u4", ar[A::U4], 32, 32, 25600},
      {"audio_conv1", ar[A::AC1], wenet ? 256 : 64, wenet ? 256 : 64, wenet ? 512 : 1024},
      {"audio_conv2", ar[A::AC2], wenet ? 256 : 128, wenet ? 256 : 128, wenet ? 512 : 1024},
      {"audio_conv3", ar[A::AC3], 256, 256, 256}, {"audio_conv4", ar[A::AC4], 256, 256, 256},
      {"audio_conv5", ar[A::AC5], 512, 512, 100}};
  for (const T& t : taps) {
    if (strcmp(t.n, name) != 0) continue;
    const int64_t per_frame = (int64_t)t.rows * t.c;
    CASYNC_REQUIRE(dst_floats >= per_frame * batch, "tap %s: dst holds %lld floats, need %lld", name,
                   (long long)dst_floats, (long long)(per_frame * batch));
    const size_t es = dtype_size(h->dtype);   // dst receives elements of the engine's storage type
    CASYNC_CHECK_HIP(hipMemcpy2DAsync(dst, (size_t)t.c * es, t.p.p, (size_t)t.ld * es, (size_t)t.c * es,
                                      (size_t)t.rows * batch, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return per_frame;
  }
  casync_set_error("tap: unknown name %s", name);
  return CASYNC_ERR_ARG;
}

// ---- single operators ------------------------------------------------------
int casync_debug_gemm_stamps(void* dev_words) {
  g_gemm_stamps = static_cast<unsigned long long*>(dev_words);
  return CASYNC_OK;
}
int casync_debug_launch_log(int on) {
  casync_launch_log.n = 0;
  casync_launch_log.overflow = false;
  casync_launch_log.on = on != 0;
  return CASYNC_OK;
}
int casync_debug_launched(char* buf, int cap) {
  CASYNC_REQUIRE(buf && cap > 0, "debug_launched: no buffer");
  CASYNC_REQUIRE(!casync_launch_log.overflow, "debug_launched: more than %d distinct kernels", CasyncLaunchLog::kCap);
  std::string all;
  for (int i = 0; i < casync_launch_log.n; ++i) {
    const char* mangled = hipKernelNameRefByPtr(casync_launch_log.kernel[i], nullptr);
    all += mangled ? kernel_short_name(mangled) : std::string("?");
    all += '\n';
  }
  CASYNC_REQUIRE((int)all.size() < cap, "debug_launched: %d bytes needed, buffer holds %d", (int)all.size() + 1, cap);
  memcpy(buf, all.c_str(), all.size() + 1);
  return casync_launch_log.n;
}
static thread_local int g_op_dtype = DT_F32;
int casync_op_set_dtype(int dtype) {
  CASYNC_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "op_set_dtype: %d", dtype);
  g_op_dtype = dtype;
  return CASYNC_OK;
}

int casync_op_pw_gemm(const void* a, int lda, const void* w, const float* bias, void* c, int ldc,
                      int m, int n, int k, int act, const void* pre_res, int ld_pre,
                      const float* pre_scale, const void* post_res, int ld_post, const float* aff_s,
                      const float* aff_t, casync_stream stream) {
  GemmEpilogue e;
  e.bias = bias;
  e.act = act;
  e.pre_res = pre_res;
  e.ld_pre = ld_pre;
  e.pre_scale = pre_scale;
  e.post_res = post_res;
  e.ld_post = ld_post;
  e.aff_s = aff_s;
  e.aff_t = aff_t;
  CASYNC_REQUIRE(!aff_s || aff_t, "pw_gemm: aff_s without aff_t");
  // stream-K scratch for the standalone operator: one region per device, created on first use
  // (callers of the op API run one GEMM at a time per device)
  static char* scratch[64] = {};
  static std::mutex scratch_mu;
  int dev = 0;
  CASYNC_CHECK_HIP(hipGetDevice(&dev));
  if (dev >= 0 && dev < 64) {
    std::lock_guard<std::mutex> lock(scratch_mu);
    if (!scratch[dev]) {
      CASYNC_CHECK_HIP(hipMalloc((void**)&scratch[dev], kStreamKBytes));
      CASYNC_CHECK_HIP(hipMemset(scratch[dev], 0, kStreamKBytes));
      CASYNC_CHECK_HIP(hipDeviceSynchronize());
    }
    e.sk_ws = reinterpret_cast<float*>(scratch[dev]);
    e.sk_cnt = reinterpret_cast<unsigned*>(scratch[dev] + kStreamKFloats * 4);
  }
  e.stamps = g_gemm_stamps;
  return launch_pw_gemm(a, lda, w, c, ldc, m, n, k, e, (hipStream_t)stream, g_op_dtype);
}
int casync_op_conv3x3(const void* in, const void* w, const float* bias, void* out, int batch, int h, int wdt,
                      int cin, int cout, int stride, int pad, int act, casync_stream stream) {
  return casync_op_conv3x3_ex(in, w, bias, out, batch, h, wdt, cin, cout, stride, stride, pad, act, stream);
}
int casync_op_conv3x3_ex(const void* in, const void* w, const float* bias, void* out, int batch, int h, int wdt,
                         int cin, int cout, int stride_h, int stride_w, int pad, int act, casync_stream stream) {
  GemmEpilogue e;
  e.bias = bias;
  e.act = act;
  if (g_op_dtype == DT_F32) {   // (fp32 only, as in the engine)
    e.conv_tab = conv3x3_positions(h, wdt, stride_h, stride_w, pad);   // cached per geometry: built on its first call
    if (!e.conv_tab) return CASYNC_ERR_ARG;
  }
  return launch_conv3x3_gemm(in, w, out, cout, batch, h, wdt, cin, cout, stride_h, stride_w, pad, e, (hipStream_t)stream,
                             g_op_dtype);
}
// What that launch walks at the process options, outside an engine (no stream-K scratch, no second lane): (tile, tap) pairs
// with all nine taps and with conv_skip.  Host only: needs no device.
int casync_conv3x3_plan(int batch, int h, int wdt, int cin, int cout, int stride_h, int stride_w, int pad, int64_t* ktile_groups_full,
                        int64_t* ktile_groups_run) {
  long long full = 0, run = 0;
  if (int st = conv3x3_plan(batch, h, wdt, cin, cout, stride_h, stride_w, pad, false, false, g_op_dtype, &full, &run)) return st;
  CASYNC_REQUIRE(ktile_groups_full && ktile_groups_run, "conv3x3_plan: null out");
  *ktile_groups_full = full;
  *ktile_groups_run = run;
  return CASYNC_OK;
}
int casync_op_dw3x3(const void* in, const float* w, const float* bias, void* out, int batch, int h,
                    int wdt, int c, int stride, casync_stream stream) {
  return launch_dw3x3(in, w, bias, out, batch, h, wdt, c, stride, (hipStream_t)stream, g_op_dtype);
}
int casync_op_dw3x3_ups(const float* pre, const float* g, int ldg, const float* w, const float* bias, float* out, int batch, int h,
                        int wdt, int c, casync_stream stream) {
  CASYNC_REQUIRE(g_op_dtype == DT_F32, "dw3x3_ups: fp32 only");
  return launch_dw3x3_ups(pre, g, ldg, w, bias, out, batch, h, wdt, c, (hipStream_t)stream);
}
int casync_op_pw_dw(const void* a, int lda, const void* w1, const float* b1, const float* wd, const float* bd, void* d, int ldd,
                    int frames, int hw, int stride, int cin, int cexp, const void* ups, int ld_ups, casync_stream stream) {
  if (g_op_dtype == DT_BF16) {
    return launch_pw_dw_bf16(a, lda, w1, b1, wd, bd, d, ldd, frames, hw, stride, cin, cexp, (hipStream_t)stream, ups, ld_ups);
  }
  return launch_pw_dw(a, lda, w1, b1, wd, bd, d, ldd, frames, hw, stride, cin, cexp, (hipStream_t)stream, ups, ld_ups);
}
int casync_op_pw_dw_rect(const void* a, int lda, const void* w1, const float* b1, const float* wd, const float* bd, void* d,
                         int ldd, int frames, int h, int w, int cin, int cexp, casync_stream stream) {
  if (g_op_dtype == DT_BF16)
    return launch_pw_dw_bf16_rect(a, lda, w1, b1, wd, bd, d, ldd, frames, h, w, cin, cexp, (hipStream_t)stream);
  return launch_pw_dw_rect(a, lda, w1, b1, wd, bd, d, ldd, frames, h, w, cin, cexp, (hipStream_t)stream);
}
int casync_op_pw_gemm_ups(const void* a, int lda, const void* w, const float* bias, void* c, int ldc, int m, int n, int k, int act,
                          const void* ups, int ld_ups, int h, int w_, casync_stream stream) {
  GemmEpilogue e;
  e.bias = bias;
  e.act = act;
  e.ups_src = ups;
  e.ups_ld = ld_ups;
  e.ups_h = h;
  e.ups_w = w_;
  return launch_pw_gemm(a, lda, w, c, ldc, m, n, k, e, (hipStream_t)stream, g_op_dtype);
}
int casync_op_ir_fused(const void* in, int ld_in, const void* w1, const float* b1, const float* wd,
                       const float* bd, const void* w2, const float* b2, void* out, int ld_out,
                       int batch, int h, int w, int cin, int cout, int stride, int res,
                       casync_stream stream) {
  return launch_ir_fused(in, ld_in, w1, b1, wd, bd, w2, b2, out, ld_out, batch, h, w, cin, cout, stride,
                         res, (hipStream_t)stream, g_op_dtype);
}
int casync_op_ir_fused_up(const void* lo, int ld_lo, int c_lo, const void* in, int ld_in, const void* w1,
                          const float* b1, const float* wd, const float* bd, const void* w2,
                          const float* b2, void* out, int ld_out, int batch, int h, int w, int cin,
                          int cout, casync_stream stream) {
  return launch_ir_fused_up(lo, ld_lo, c_lo, in, ld_in, w1, b1, wd, bd, w2, b2, out, ld_out, batch, h, w, cin,
                            cout, (hipStream_t)stream, g_op_dtype);
}
int casync_op_ir_fused_upg(const float* g, int ld_g, const float* in, int ld_in, const float* w1b, const float* b1,
                           const float* wd, const float* bd, const float* w2, const float* b2, float* out, int ld_out,
                           int batch, int h, int w, int cin, int cout, casync_stream stream) {
  return launch_ir_fused_upg(g, ld_g, in, ld_in, w1b, b1, wd, bd, w2, b2, out, ld_out, batch, h, w, cin, cout,
                             (hipStream_t)stream);
}
int casync_op_upsample2x(const void* in, void* out, int ldc, int batch, int h, int wdt, int c,
                         casync_stream stream) {
  return launch_upsample2x(in, out, ldc, batch, h, wdt, c, (hipStream_t)stream, g_op_dtype);
}
int casync_op_cross_attention(const void* q, int ldq, const void* k, int ldk, const void* v,
                              int ldv, const void* res, int ld_res, const float* gamma_dev,
                              void* out, int ld_out, int batch, casync_stream stream) {
  return launch_cross_attention(q, ldq, k, ldk, v, ldv, res, ld_res, gamma_dev, out, ld_out, batch,
                                (hipStream_t)stream, g_op_dtype);
}
int casync_op_nchw_to_nhwc(const float* in, void* out, int batch, int c, int hw, casync_stream stream) {
  return launch_nchw_to_nhwc(in, out, batch, c, hw, (hipStream_t)stream, g_op_dtype);
}
int casync_op_inc(const float* x_nchw, const float* packed_inc, void* out, int ldc, int batch,
                  casync_stream stream) {
  return launch_inc(x_nchw, packed_inc, out, ldc, batch, (hipStream_t)stream, g_op_dtype);
}
int casync_op_audio_windows(const float* features_dev, int n_steps, const int32_t* frame_idx_dev, void* windows_dev,
                            int batch, int nhwc, casync_stream stream) {
  if (nhwc) return launch_audio_window_gather(features_dev, n_steps, frame_idx_dev, windows_dev, batch, (hipStream_t)stream,
                                              g_op_dtype);
  return launch_audio_windows_nchw(features_dev, n_steps, frame_idx_dev, (float*)windows_dev, batch, (hipStream_t)stream);
}
int casync_op_crop_to_input(const uint8_t* crops168_dev, float* x_dev, int batch, casync_stream stream) {
  return launch_crop_to_input(crops168_dev, x_dev, batch, (hipStream_t)stream);
}
int casync_op_pred_to_u8(const float* pred_dev, uint8_t* out_dev, int batch, casync_stream stream) {
  return launch_pred_to_u8(pred_dev, out_dev, batch, (hipStream_t)stream);
}
int casync_op_outc(const void* in, int ld_in, const float* w, const float* b, float* out_nchw,
                   int batch, casync_stream stream) {
  return launch_outc(in, ld_in, w, b, out_nchw, batch, (hipStream_t)stream, g_op_dtype);
}

}  // extern "C"
