// A clip resident on the device, for the frame loop: the two byte moves between the stored frames [N,H,W,3] u8 and the packed
// `regions` layout that casync_frame_prepare / casync_frame_paste_back read and write.
//
//   gather:   regions[offset .. offset + h w 3) = frames[frame, y0:y0+h, x0:x0+w]          the img[ymin:ymax, xmin:xmax] of infer_api.py:234
//   compose:  out[b] = frames[frame], with the box replaced by out_regions[offset ..) where valid     infer_api.py:201, 346
//
// A record is 8 int32: { frame, y0, x0, h, w, valid, region byte offset, 0 }.  Records arrive in HOST memory, are all checked
// before the first launch and travel as kernel arguments, RECORDS_PER_LAUNCH to a launch (the idiom of face_ops.hip): neither
// an upload nor a synchronisation.
//
// Both kernels are row copies: one wave per row of a record, a row being one span of bytes (gather; compose outside the box)
// or three (compose inside a valid box: frame | out_regions | frame).  Every output byte belongs to exactly one span and a
// span has one source, so a byte has ONE writer: nothing is copied first and pasted over.  Within a span the access width is
// the largest power of two up to 16 bytes that divides (source - destination); the bytes before the destination's first
// aligned address and behind its last whole vector go one by one.  A vector therefore never crosses a span's end, and every
// access is aligned on both sides.  All byte offsets are 64-bit: the base of frame 346 of a 1080p clip is past 2^31.
// No LDS, no atomics, no scratch.
#include "common.h"

namespace {

constexpr int RECORDS_PER_LAUNCH = 64;
constexpr int REC_WORDS = 8;              // frame, y0, x0, h, w, valid, region byte offset, 0
constexpr int WAVES = 4;                  // per workgroup: one row each at a time
constexpr int ROWS_PER_WAVE = 4;          // rows a wave walks when the grid covers the tallest record

struct ClipBlock { int r[RECORDS_PER_LAUNCH][REC_WORDS]; };

template <class T>
__device__ __forceinline__ void copy_vectors(unsigned char* d, const unsigned char* s, unsigned n_vec, int lane) {
  T* dv = reinterpret_cast<T*>(d);
  const T* sv = reinterpret_cast<const T*>(s);
  for (unsigned i = lane; i < n_vec; i += 64) dv[i] = sv[i];
}

// n bytes s -> d by the 64 lanes of one wave (d, s, n are the same on every lane).
__device__ __forceinline__ void copy_span(unsigned char* d, const unsigned char* s, unsigned n, int lane) {
  if (n == 0) return;
  const unsigned apart = ((unsigned)(uintptr_t)s - (unsigned)(uintptr_t)d) | 16u;
  const unsigned width = apart & (0u - apart);                      // 1, 2, 4, 8 or 16: both sides aligned together
  unsigned head = (0u - (unsigned)(uintptr_t)d) & (width - 1u);     // bytes before d's first aligned address (< 16)
  if (head > n) head = n;
  const unsigned n_vec = (n - head) / width;
  const unsigned done = head + n_vec * width, tail = n - done;      // tail < width <= 16
  if (lane < (int)head) d[lane] = s[lane];
  if (lane >= 16 && lane - 16 < (int)tail) d[done + lane - 16] = s[done + lane - 16];
  switch (width) {
    case 16: copy_vectors<uint4>(d + head, s + head, n_vec, lane); break;
    case 8: copy_vectors<uint2>(d + head, s + head, n_vec, lane); break;
    case 4: copy_vectors<unsigned>(d + head, s + head, n_vec, lane); break;
    case 2: copy_vectors<unsigned short>(d + head, s + head, n_vec, lane); break;
    default: copy_vectors<unsigned char>(d + head, s + head, n_vec, lane); break;
  }
}

// grid (row groups, records of this launch)
__global__ __launch_bounds__(64 * WAVES) void clip_gather_kernel(const unsigned char* __restrict__ frames, int H, int W, ClipBlock blk,
                                                                 unsigned char* __restrict__ regions) {
  const int* g = blk.r[blockIdx.y];
  const int y0 = g[1], x0 = g[2], h = g[3], w = g[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row_bytes = (size_t)W * 3;
  const unsigned char* src = frames + (size_t)g[0] * H * row_bytes + (size_t)y0 * row_bytes + (size_t)x0 * 3;
  unsigned char* dst = regions + (size_t)g[6];
  const unsigned n = (unsigned)w * 3u;
  for (int r = blockIdx.x * WAVES + wave; r < h; r += gridDim.x * WAVES) copy_span(dst + (size_t)r * n, src + (size_t)r * row_bytes, n, lane);
}

// grid (row groups, records of this launch); out points at the first frame of this launch
__global__ __launch_bounds__(64 * WAVES) void clip_compose_kernel(const unsigned char* __restrict__ frames, int H, int W, ClipBlock blk,
                                                                  const unsigned char* __restrict__ out_regions,
                                                                  unsigned char* __restrict__ out) {
  const int* g = blk.r[blockIdx.y];
  const bool valid = g[5] != 0;
  const int y0 = g[1], x0 = g[2], h = g[3], w = g[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row_bytes = (size_t)W * 3, frame_bytes = (size_t)H * row_bytes;
  const unsigned char* src = frames + (size_t)g[0] * frame_bytes;
  unsigned char* dst = out + (size_t)blockIdx.y * frame_bytes;
  const unsigned char* box = valid ? out_regions + (size_t)g[6] : nullptr;
  const unsigned left = (unsigned)x0 * 3u, mid = (unsigned)w * 3u;
  for (int y = blockIdx.x * WAVES + wave; y < H; y += gridDim.x * WAVES) {
    const unsigned char* s = src + (size_t)y * row_bytes;
    unsigned char* d = dst + (size_t)y * row_bytes;
    if (valid && y >= y0 && y < y0 + h) {                           // the box's bytes come from out_regions alone
      copy_span(d, s, left, lane);
      copy_span(d + left, box + (size_t)(y - y0) * mid, mid, lane);
      copy_span(d + left + mid, s + left + mid, (unsigned)row_bytes - left - mid, lane);
    } else {
      copy_span(d, s, (unsigned)row_bytes, lane);
    }
  }
}

unsigned row_groups(int rows) {
  const int per_group = WAVES * ROWS_PER_WAVE;
  return (unsigned)((rows + per_group - 1) / per_group);
}

// rec[first .. first + n) -> one kernel-argument block, checked.  check_box: every record (gather) or the valid ones (compose);
// have_regions: a valid record has somewhere to read from.  *tallest: the most rows a record of the block copies.
int fill_block(const int32_t* rec, int first, int n, int n_frames, int H, int W, int64_t regions_bytes, bool every_box, bool have_regions,
               const char* who, ClipBlock& blk, int* tallest) {
  *tallest = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t* g = rec + (size_t)(first + i) * REC_WORDS;
    const bool valid = g[5] != 0;
    CASYNC_REQUIRE(g[0] >= 0 && g[0] < n_frames, "%s: record %d names frame %d of %d", who, first + i, g[0], n_frames);
    CASYNC_REQUIRE(have_regions || !valid, "%s: record %d is valid and out_regions is null", who, first + i);
    if (every_box || valid) {
      CASYNC_REQUIRE(g[3] >= 1 && g[4] >= 1, "%s: record %d has a box of %d x %d (h x w)", who, first + i, g[3], g[4]);
      CASYNC_REQUIRE(g[1] >= 0 && g[2] >= 0 && (long long)g[1] + g[3] <= H && (long long)g[2] + g[4] <= W,
                     "%s: record %d: box %d x %d at (%d, %d) (h x w at y, x) is not inside the %d x %d frame", who, first + i, g[3], g[4], g[1],
                     g[2], H, W);
      CASYNC_REQUIRE(g[6] >= 0 && (long long)g[6] + (long long)g[3] * g[4] * 3 <= (long long)regions_bytes,
                     "%s: record %d: %lld bytes at offset %d do not fit regions of %lld bytes", who, first + i, (long long)g[3] * g[4] * 3, g[6],
                     (long long)regions_bytes);
      if (g[3] > *tallest) *tallest = g[3];
    }
    for (int k = 0; k < REC_WORDS; ++k) blk.r[i][k] = g[k];
  }
  for (int i = n; i < RECORDS_PER_LAUNCH; ++i)
    for (int k = 0; k < REC_WORDS; ++k) blk.r[i][k] = 0;
  return CASYNC_OK;
}

}  // namespace

extern "C" {

int casync_op_clip_gather(const uint8_t* frames, int n_frames, int H, int W, const int32_t* rec, int batch, uint8_t* regions,
                          int64_t regions_bytes, casync_stream stream) {
  CASYNC_REQUIRE(frames && rec && regions, "clip_gather: null pointer");
  CASYNC_REQUIRE(H >= 1 && W >= 1, "clip_gather: frames of %d x %d (h x w)", H, W);
  CASYNC_REQUIRE(batch >= 0, "clip_gather: batch %d", batch);
  ClipBlock blk;
  int tallest;
  for (int first = 0; first < batch; first += RECORDS_PER_LAUNCH) {      // every record is checked before the first launch
    const int n = batch - first < RECORDS_PER_LAUNCH ? batch - first : RECORDS_PER_LAUNCH;
    if (int st = fill_block(rec, first, n, n_frames, H, W, regions_bytes, true, true, "clip_gather", blk, &tallest)) return st;
  }
  for (int first = 0; first < batch; first += RECORDS_PER_LAUNCH) {
    const int n = batch - first < RECORDS_PER_LAUNCH ? batch - first : RECORDS_PER_LAUNCH;
    fill_block(rec, first, n, n_frames, H, W, regions_bytes, true, true, "clip_gather", blk, &tallest);
    if (int st = casync_launch(clip_gather_kernel, dim3(row_groups(tallest), n), dim3(64 * WAVES), 0, (hipStream_t)stream, frames, H, W, blk,
                               regions))
      return st;
  }
  return CASYNC_OK;
}

int casync_op_clip_compose(const uint8_t* frames, int n_frames, int H, int W, const int32_t* rec, int batch, const uint8_t* out_regions,
                           int64_t regions_bytes, uint8_t* out, casync_stream stream) {
  CASYNC_REQUIRE(frames && rec && out, "clip_compose: null pointer");
  CASYNC_REQUIRE(H >= 1 && W >= 1, "clip_compose: frames of %d x %d (h x w)", H, W);
  CASYNC_REQUIRE(batch >= 0, "clip_compose: batch %d", batch);
  ClipBlock blk;
  int tallest;
  for (int first = 0; first < batch; first += RECORDS_PER_LAUNCH) {
    const int n = batch - first < RECORDS_PER_LAUNCH ? batch - first : RECORDS_PER_LAUNCH;
    if (int st = fill_block(rec, first, n, n_frames, H, W, regions_bytes, false, out_regions != nullptr, "clip_compose", blk, &tallest)) return st;
  }
  for (int first = 0; first < batch; first += RECORDS_PER_LAUNCH) {
    const int n = batch - first < RECORDS_PER_LAUNCH ? batch - first : RECORDS_PER_LAUNCH;
    fill_block(rec, first, n, n_frames, H, W, regions_bytes, false, out_regions != nullptr, "clip_compose", blk, &tallest);
    if (int st = casync_launch(clip_compose_kernel, dim3(row_groups(H), n), dim3(64 * WAVES), 0, (hipStream_t)stream, frames, H, W, blk,
                               out_regions, out + (size_t)first * H * W * 3))
      return st;
  }
  return CASYNC_OK;
}

}  // extern "C"
