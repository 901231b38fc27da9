// The trainer's batch from a clip resident on the device: what MyDataset.__getitem__ / process_img of the reference
// (dataset/dataset.py:73-134) compute per sample with two cv2.imread, two cv2.resize and numpy, as ONE kernel over the stored
// frames [N,H,W,3] u8.
//
//   crop168  = cv2.resize(frame[y0:y0+h, x0:x0+w], (168, 168))     INTER_LINEAR (resize_u8.h; the region may be non-square)
//   real     = crop168[4:164, 4:164]
//   masked   = real with the filled rectangle (x, y, w, h) = (5, 5, 150, 145) black: x in [5, 154], y in [5, 149]
//   real_ex  = the same crop of the reference frame, with its own box
//   img_concat[b] = cat(real_ex, masked) [6,160,160], img_real[b] = real [3,160,160]: CHW, float(u8) / 255.0f (fp32 division)
//
// A record is 12 int32: { t, y0, x0, h, w, r, ry0, rx0, rh, rw, 0, 0 }, both boxes already cut to the frame.  Records arrive in
// HOST memory, are all checked before the first launch and travel as kernel arguments, RECORDS_PER_LAUNCH to a launch (the
// idiom of clip_ops.hip): neither an upload nor a synchronisation, no workspace.
//
// A sample writes 9 x 160 x 160 floats (922 KB) and reads two regions (0.4 - 1.3 MB each on 1080p frames) as byte gathers through
// the caches.  The stores are laid out for the memory system: a lane owns four consecutive floats of a plane, so a wave writes 1 KB
// of each of the nine planes in one piece, with 16-byte stores where both outputs are 16-byte aligned (a plane is 25600 floats, a
// lane's offset a multiple of 4) and four 4-byte stores otherwise.  The regions are read straight from the stored frames: no
// `regions` buffer, no crops168 in memory.  Every output element has one writer.  Frame byte offsets are 64-bit: the base of frame
// 346 of a 1080p clip is past 2^31.  No LDS, no atomics, no scratch.  Measured: 82 us for 64 samples of
// 390 - 650 pixel regions, 0.7 TB/s of stores and about 2 TB/s with the region bytes: the gathers, not the stores, are the bound.
//
// Floating point that must round like the host's (numpy, scalar C++): contraction is switched off in this file.
#pragma clang fp contract(off)
#include "../../include/casync_train.h"
#include "common.h"
#include "resize_u8.h"

namespace {

constexpr int RECORDS_PER_LAUNCH = 64;
constexpr int REC_WORDS = 12;             // t, y0, x0, h, w, r, ry0, rx0, rh, rw, 0, 0
constexpr int OUT = 160, CROP = 168, INSET = 4, PLANE = OUT * OUT;
constexpr int THREADS = 256, PX_PER_LANE = 4;
constexpr int GROUPS = PLANE / (THREADS * PX_PER_LANE);      // 25 workgroups a sample
static_assert(GROUPS * THREADS * PX_PER_LANE == PLANE && OUT % PX_PER_LANE == 0, "a lane's four pixels lie in one row");

struct TrainBlock { int r[RECORDS_PER_LAUNCH][REC_WORDS]; };

template <bool VEC>
__device__ __forceinline__ void store4(float* p, f32x4 v) {
  if (VEC) {
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
    p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
  }
}

// grid (GROUPS, records of this launch); `first`: the sample the launch's record 0 writes
template <bool VEC>
__global__ __launch_bounds__(THREADS) void train_batch_kernel(const unsigned char* __restrict__ frames, int H, int W, TrainBlock blk,
                                                              int first, float* __restrict__ img_concat, float* __restrict__ img_real) {
  const int* g = blk.r[blockIdx.y];
  const int p = (blockIdx.x * THREADS + threadIdx.x) * PX_PER_LANE;     // first of four pixels of one row of the 160 x 160 planes
  const int py = p / OUT, px = p - py * OUT;
  const size_t row_bytes = (size_t)W * 3, frame_bytes = (size_t)H * row_bytes;
  const int h = g[3], w = g[4], rh = g[8], rw = g[9];
  const unsigned char* tgt = frames + (size_t)g[0] * frame_bytes + (size_t)g[1] * row_bytes + (size_t)g[2] * 3;
  const unsigned char* ref = frames + (size_t)g[5] * frame_bytes + (size_t)g[6] * row_bytes + (size_t)g[7] * 3;
  auto fetch_t = [&](int y, int x, int c) -> int { return tgt[(size_t)y * row_bytes + x * 3 + c]; };
  auto fetch_r = [&](int y, int x, int c) -> int { return ref[(size_t)y * row_bytes + x * 3 + c]; };
  const size_t b = (size_t)first + blockIdx.y;
  float* cat = img_concat + b * 6 * PLANE + p;
  float* real = img_real + b * 3 * PLANE + p;
  const bool row_masked = py >= 5 && py < 150;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f32x4 ex, re, ma;
#pragma unroll
    for (int k = 0; k < PX_PER_LANE; ++k) {
      const int x = px + k;
      ex[k] = __fdiv_rn((float)resize_u8_at(fetch_r, rh, rw, CROP, CROP, py + INSET, x + INSET, c), 255.0f);
      re[k] = __fdiv_rn((float)resize_u8_at(fetch_t, h, w, CROP, CROP, py + INSET, x + INSET, c), 255.0f);
      ma[k] = row_masked && x >= 5 && x < 155 ? 0.f : re[k];
    }
    store4<VEC>(cat + c * PLANE, ex);
    store4<VEC>(cat + (3 + c) * PLANE, ma);
    store4<VEC>(real + c * PLANE, re);
  }
}

bool box_ok(const int32_t* b, int H, int W) {      // { y0, x0, h, w } inside the frame
  return b[0] >= 0 && b[1] >= 0 && (long long)b[0] + b[2] <= H && (long long)b[1] + b[3] <= W;
}

// rec[first .. first + n) -> one kernel-argument block, checked
int fill_block(const int32_t* rec, int first, int n, int n_frames, int H, int W, TrainBlock& blk) {
  for (int i = 0; i < n; ++i) {
    const int32_t* g = rec + (size_t)(first + i) * REC_WORDS;
    for (int side = 0; side < 2; ++side) {
      const int32_t* s = g + 5 * side;
      const char* who = side ? "reference" : "target";
      CASYNC_REQUIRE(s[0] >= 0 && s[0] < n_frames, "train_batch: record %d names %s frame %d of %d", first + i, who, s[0], n_frames);
      CASYNC_REQUIRE(s[3] >= 1 && s[4] >= 1, "train_batch: record %d has a %s box of %d x %d (h x w)", first + i, who, s[3], s[4]);
      CASYNC_REQUIRE(box_ok(s + 1, H, W), "train_batch: record %d: %s box %d x %d at (%d, %d) (h x w at y, x) is not inside the %d x %d frame",
                     first + i, who, s[3], s[4], s[1], s[2], H, W);
    }
    for (int k = 0; k < REC_WORDS; ++k) blk.r[i][k] = g[k];
  }
  for (int i = n; i < RECORDS_PER_LAUNCH; ++i)
    for (int k = 0; k < REC_WORDS; ++k) blk.r[i][k] = 0;
  return CASYNC_OK;
}

}  // namespace

extern "C" {

int casync_op_train_batch(const uint8_t* frames, int n_frames, int H, int W, const int32_t* rec, int batch, float* img_concat,
                          float* img_real, casync_stream stream) {
  CASYNC_REQUIRE(frames && rec && img_concat && img_real, "train_batch: null pointer");
  CASYNC_REQUIRE(H >= 1 && W >= 1, "train_batch: frames of %d x %d (h x w)", H, W);
  CASYNC_REQUIRE(batch >= 0, "train_batch: batch %d", batch);
  TrainBlock blk;
  for (int first = 0; first < batch; first += RECORDS_PER_LAUNCH) {      // every record is checked before the first launch
    const int n = batch - first < RECORDS_PER_LAUNCH ? batch - first : RECORDS_PER_LAUNCH;
    if (int st = fill_block(rec, first, n, n_frames, H, W, blk)) return st;
  }
  const bool vec = (((uintptr_t)img_concat | (uintptr_t)img_real) & 15u) == 0;
  for (int first = 0; first < batch; first += RECORDS_PER_LAUNCH) {
    const int n = batch - first < RECORDS_PER_LAUNCH ? batch - first : RECORDS_PER_LAUNCH;
    fill_block(rec, first, n, n_frames, H, W, blk);
    if (int st = casync_launch(vec ? train_batch_kernel<true> : train_batch_kernel<false>, dim3(GROUPS, n), dim3(THREADS), 0,
                               (hipStream_t)stream, frames, H, W, blk, first, img_concat, img_real))
      return st;
  }
  return CASYNC_OK;
}

}  // extern "C"
