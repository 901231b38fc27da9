// The pixel and row work between the two face networks, on the device: frames -> S3FD input, dense det -> candidate rows,
// frames + boxes -> PFLD crops, PFLD output -> int32 landmarks.
//
//   resize:      [B,sh,sw,3] u8 --cv2.resize(INTER_LINEAR)--> [B,dh,dw,3]     S3FD.detect_faces, tools/s3fd/main.py:34
//   crops192:    the padded 1.05 x square of every box --cv2.resize--> 192 x 192 x 3      lip_detector.py:46-80
//   candidates:  det[b][det[b,:,0] > thresh] in prior order                               box_utils.py:150-156
//   finalize:    int32((y + mean_face) * (w, h) + (x1, y1))                               lip_detector.py:106-114
//
// The resize is OpenCV 4.x's 8-bit INTER_LINEAR path (resize.cpp: float position tables made in double, 11-bit coefficients
// by cvRound, the 22-bit vertical pass) with its two special cases, equal sizes and the exact 2x decimation that cv::resize
// hands to INTER_AREA.  oracle/frame_ops_oracle.py::resize_linear_u8 is the same restatement on the CPU and the -m gpu tests
// demand bit equality with it; parity with the real cv2 is as unpinned here as for the frame loop.
//
// Per-crop geometry arrives as kernel arguments, a block of CROPS_PER_LAUNCH records per launch: the entry points read it
// from host memory, check it before any device call, and need neither an upload nor a synchronisation.
//
// Floating point here has to round like numpy on the host: no contraction, and the roundings that matter are spelled out.
#pragma clang fp contract(off)
#include "common.h"

namespace {

constexpr int COEF_ONE = 2048;            // INTER_RESIZE_COEF_SCALE: 11 fractional bits
constexpr int FACE = 192;                 // PFLD's input side
constexpr int CROPS_PER_LAUNCH = 64;
constexpr int GEOM_WORDS = 5;             // frame, x1, y1, w, h

struct CropBlock { int g[CROPS_PER_LAUNCH][GEOM_WORDS]; };

// One axis of the bilinear table for destination index d: the two source indices and their fixed-point weights.
struct AxisTap { int i0, i1, c0, c1; };

// position in the source, as cv::resize computes it: double arithmetic, one rounding to float
__device__ __forceinline__ float src_position(int d, double scale) {
  return (float)__dsub_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), 0.5);
}
__device__ __forceinline__ int fixed_weight(float c) { return __float2int_rn(__fmul_rn(c, (float)COEF_ONE)); }   // cvRound: half to even

// Columns: a position left of the first or at / right of the last source column collapses onto that column with weight 1.
__device__ __forceinline__ AxisTap tap_columns(int d, int n, double scale) {
  const float pos = src_position(d, scale);
  int i = (int)floorf(pos);
  float frac = __fsub_rn(pos, (float)i);
  if (i < 0) { i = 0; frac = 0.f; }
  if (i >= n - 1) { i = n - 1; frac = 0.f; }
  return AxisTap{i, i + 1 < n ? i + 1 : n - 1, fixed_weight(__fsub_rn(1.f, frac)), fixed_weight(frac)};
}
// Rows: the indices are clipped into the image, the weights stay what the position gave.
__device__ __forceinline__ AxisTap tap_rows(int d, int n, double scale) {
  const float pos = src_position(d, scale);
  const int i = (int)floorf(pos);
  const float frac = __fsub_rn(pos, (float)i);
  const int lo = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
  const int hi = i + 1 < 0 ? 0 : (i + 1 > n - 1 ? n - 1 : i + 1);
  return AxisTap{lo, hi, fixed_weight(__fsub_rn(1.f, frac)), fixed_weight(frac)};
}

enum ResizeMode { MODE_COPY = 0, MODE_AREA2 = 1, MODE_LINEAR = 2 };
__host__ __device__ __forceinline__ int resize_mode(int sh, int sw, int dh, int dw) {
  if (sh == dh && sw == dw) return MODE_COPY;
  if (sw == 2 * dw && sh == 2 * dh) return MODE_AREA2;
  return MODE_LINEAR;
}

// The three channels of destination pixel (dy, dx).  px(y, x, out[3]) reads one source pixel.
template <class Px>
__device__ __forceinline__ void resize_pixel(Px px, int mode, int sh, int sw, double scale_y, double scale_x, int dy, int dx, int out[3]) {
  if (mode == MODE_COPY) {
    px(dy, dx, out);
    return;
  }
  int p00[3], p01[3], p10[3], p11[3];
  if (mode == MODE_AREA2) {
    px(2 * dy, 2 * dx, p00); px(2 * dy, 2 * dx + 1, p01); px(2 * dy + 1, 2 * dx, p10); px(2 * dy + 1, 2 * dx + 1, p11);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (p00[c] + p01[c] + p10[c] + p11[c] + 2) >> 2;
    return;
  }
  const AxisTap tx = tap_columns(dx, sw, scale_x), ty = tap_rows(dy, sh, scale_y);
  px(ty.i0, tx.i0, p00); px(ty.i0, tx.i1, p01); px(ty.i1, tx.i0, p10); px(ty.i1, tx.i1, p11);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int top = p00[c] * tx.c0 + p01[c] * tx.c1;          // horizontal pass: int, not shifted
    const int bot = p10[c] * tx.c0 + p11[c] * tx.c1;
    const int v = (((ty.c0 * (top >> 4)) >> 16) + ((ty.c1 * (bot >> 4)) >> 16) + 2) >> 2;
    out[c] = v < 0 ? 0 : (v > 255 ? 255 : v);
  }
}

// ---------------------------------------------------------------- frames -> frames of another size
// One lane per destination pixel: at the detector's scale 4 a destination row touches two of every four source rows and
// two of every four columns, so the taps are gathered straight from global memory (three consecutive bytes each).
__global__ __launch_bounds__(256) void face_resize_kernel(const unsigned char* __restrict__ src, int sh, int sw,
                                                          unsigned char* __restrict__ dst, int dh, int dw, double scale_x,
                                                          double scale_y, int mode) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= dh * dw) return;
  const int dy = p / dw, dx = p - dy * dw;
  const unsigned char* frame = src + (size_t)blockIdx.y * sh * sw * 3;
  auto px = [&](int y, int x, int v[3]) {
    const unsigned char* q = frame + ((size_t)y * sw + x) * 3;
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
  };
  int out[3];
  resize_pixel(px, mode, sh, sw, scale_y, scale_x, dy, dx, out);
  unsigned char* o = dst + ((size_t)blockIdx.y * dh * dw + p) * 3;
  o[0] = (unsigned char)out[0]; o[1] = (unsigned char)out[1]; o[2] = (unsigned char)out[2];
}

// ---------------------------------------------------------------- frames + crop records -> 192 x 192 crops
// The h x w crop is a window on its frame that may hang over any border (zeros there): it exists only as this fetch.
__global__ __launch_bounds__(256) void face_crops192_kernel(const unsigned char* __restrict__ frames, int H, int W, CropBlock blk,
                                                            unsigned char* __restrict__ crops) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= FACE * FACE) return;
  const int* g = blk.g[blockIdx.y];
  const int x1 = g[1], y1 = g[2], w = g[3], h = g[4];
  const unsigned char* frame = frames + (size_t)g[0] * H * W * 3;
  auto px = [&](int y, int x, int v[3]) {
    const int fy = y1 + y, fx = x1 + x;
    if (fy >= 0 && fy < H && fx >= 0 && fx < W) {
      const unsigned char* q = frame + ((size_t)fy * W + fx) * 3;
      v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
    } else {
      v[0] = v[1] = v[2] = 0;
    }
  };
  const int dy = p / FACE, dx = p - dy * FACE;
  // cv2.resize(crop, (192, 192)): scale = 1 / (dst / src), both in double
  const double scale_x = 1.0 / ((double)FACE / (double)w), scale_y = 1.0 / ((double)FACE / (double)h);
  int out[3];
  resize_pixel(px, resize_mode(h, w, FACE, FACE), h, w, scale_y, scale_x, dy, dx, out);
  unsigned char* o = crops + ((size_t)blockIdx.y * FACE * FACE + p) * 3;
  o[0] = (unsigned char)out[0]; o[1] = (unsigned char)out[1]; o[2] = (unsigned char)out[2];
}

// ---------------------------------------------------------------- dense det -> rows above the threshold, in prior order
// One 256-lane workgroup per frame walks the priors 256 at a time.  Within a step a lane's slot is the number of passing
// priors before it: the lanes below it in its wave (ballot), the waves below it (four counts in LDS), the steps before
// (a running base every lane keeps).  No atomics, so the order is the priors'.
__global__ __launch_bounds__(256) void face_candidates_kernel(const float* __restrict__ det, int P, float thresh, int cap,
                                                              int* __restrict__ counts, float* __restrict__ rows) {
  __shared__ int wave_total[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* d = det + (size_t)blockIdx.x * P * 5;
  float* out = rows + (size_t)blockIdx.x * cap * 5;
  int base = 0;
  for (int start = 0, it = 0; start < P; start += 256, ++it) {
    const int p = start + threadIdx.x;
    const bool pass = p < P && d[(size_t)p * 5] > thresh;          // a NaN score fails, as in numpy
    const unsigned long long votes = __ballot(pass);
    const int before = __popcll(votes & ((1ull << lane) - 1ull));
    int* tot = wave_total[it & 1];                                  // two sets: one barrier per step is enough
    if (lane == 0) tot[wave] = __popcll(votes);
    __syncthreads();
    int slot = base + before;
    for (int k = 0; k < wave; ++k) slot += tot[k];
    if (pass && slot < cap) {
      const float* r = d + (size_t)p * 5;
      float* o = out + (size_t)slot * 5;
      o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3]; o[4] = r[4];
    }
    base += tot[0] + tot[1] + tot[2] + tot[3];
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = base;
}

// ---------------------------------------------------------------- PFLD output -> int32 landmarks
__global__ __launch_bounds__(128) void face_finalize_kernel(const float* __restrict__ y, const float* __restrict__ mean_face,
                                                            CropBlock blk, int* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= 110) return;
  const int* g = blk.g[blockIdx.x];
  const float* row = y + (size_t)blockIdx.x * 220;
  // (row + mean) * (w, h) + (x1, y1): float32, every operation rounded on its own; astype(int32) truncates
  const float px = __fadd_rn(__fmul_rn(__fadd_rn(row[2 * k], mean_face[2 * k]), (float)g[3]), (float)g[1]);
  const float py = __fadd_rn(__fmul_rn(__fadd_rn(row[2 * k + 1], mean_face[2 * k + 1]), (float)g[4]), (float)g[2]);
  int* o = out + ((size_t)blockIdx.x * 110 + k) * 2;
  o[0] = (int)px;
  o[1] = (int)py;
}

constexpr int MAX_SIDE = 32767;           // image and crop sides: the products below stay inside int / size_t
constexpr int MAX_OFFSET = 1 << 24;       // |x1|, |y1| of a crop

// geom[first .. first + n) -> one kernel-argument block, checked; n_frames < 0: no frame index to check (finalize)
int fill_block(const int32_t* geom, int first, int n, int n_frames, const char* who, CropBlock& blk) {
  for (int i = 0; i < n; ++i) {
    const int32_t* g = geom + (size_t)(first + i) * GEOM_WORDS;
    CASYNC_REQUIRE(g[3] >= 1 && g[4] >= 1 && g[3] <= MAX_SIDE && g[4] <= MAX_SIDE, "%s: crop %d is %d x %d (w x h), sides are 1..%d", who,
                   first + i, g[3], g[4], MAX_SIDE);
    CASYNC_REQUIRE(g[1] >= -MAX_OFFSET && g[1] <= MAX_OFFSET && g[2] >= -MAX_OFFSET && g[2] <= MAX_OFFSET,
                   "%s: crop %d starts at (%d, %d), beyond +-%d", who, first + i, g[1], g[2], MAX_OFFSET);
    CASYNC_REQUIRE(n_frames < 0 || (g[0] >= 0 && g[0] < n_frames), "%s: crop %d names frame %d of %d", who, first + i, g[0], n_frames);
    for (int k = 0; k < GEOM_WORDS; ++k) blk.g[i][k] = g[k];
  }
  for (int i = n; i < CROPS_PER_LAUNCH; ++i)
    for (int k = 0; k < GEOM_WORDS; ++k) blk.g[i][k] = 0;
  return CASYNC_OK;
}

}  // namespace

extern "C" {

int casync_op_resize_linear_u8(const uint8_t* src, int batch, int sh, int sw, uint8_t* dst, int dh, int dw, double scale_x,
                               double scale_y, casync_stream stream) {
  CASYNC_REQUIRE(src && dst, "resize_linear_u8: null pointer");
  CASYNC_REQUIRE(batch >= 1 && batch <= 65535, "resize_linear_u8: batch %d (1..65535)", batch);
  CASYNC_REQUIRE(sh >= 1 && sw >= 1 && dh >= 1 && dw >= 1 && sh <= MAX_SIDE && sw <= MAX_SIDE && dh <= MAX_SIDE && dw <= MAX_SIDE,
                 "resize_linear_u8: %d x %d -> %d x %d (h x w), sides are 1..%d", sh, sw, dh, dw, MAX_SIDE);
  // a destination index must land within int range of the source: (d + 0.5) * scale stays below 2^31
  CASYNC_REQUIRE(scale_x > 0.0 && scale_y > 0.0 && scale_x <= 32768.0 && scale_y <= 32768.0,
                 "resize_linear_u8: scale (%g, %g), expected source / destination in (0, 32768]", scale_x, scale_y);
  return casync_launch(face_resize_kernel, dim3((unsigned)(((long long)dh * dw + 255) / 256), batch), dim3(256), 0, (hipStream_t)stream, src,
                       sh, sw, dst, dh, dw, scale_x, scale_y, resize_mode(sh, sw, dh, dw));
}

int casync_op_face_crops192(const uint8_t* frames, int n_frames, int H, int W, const int32_t* geom, int n_crops, uint8_t* crops192,
                            casync_stream stream) {
  CASYNC_REQUIRE(frames && geom && crops192, "face_crops192: null pointer");
  CASYNC_REQUIRE(n_frames >= 1 && H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "face_crops192: %d frames of %d x %d (h x w)",
                 n_frames, H, W);
  CASYNC_REQUIRE(n_crops >= 1 && n_crops <= (1 << 20), "face_crops192: %d crops (1..%d)", n_crops, 1 << 20);
  CropBlock blk;
  for (int first = 0; first < n_crops; first += CROPS_PER_LAUNCH) {      // every record is checked before the first launch
    const int n = n_crops - first < CROPS_PER_LAUNCH ? n_crops - first : CROPS_PER_LAUNCH;
    if (int st = fill_block(geom, first, n, n_frames, "face_crops192", blk)) return st;
  }
  for (int first = 0; first < n_crops; first += CROPS_PER_LAUNCH) {
    const int n = n_crops - first < CROPS_PER_LAUNCH ? n_crops - first : CROPS_PER_LAUNCH;
    fill_block(geom, first, n, n_frames, "face_crops192", blk);
    if (int st = casync_launch(face_crops192_kernel, dim3((FACE * FACE + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, frames, H, W, blk,
                               crops192 + (size_t)first * FACE * FACE * 3))
      return st;
  }
  return CASYNC_OK;
}

int casync_op_s3fd_candidates(const float* det, int batch, int P, float thresh, int cap, int32_t* counts, float* rows,
                              casync_stream stream) {
  CASYNC_REQUIRE(det && counts && rows, "s3fd_candidates: null pointer");
  CASYNC_REQUIRE(batch >= 1 && batch <= 65535 && P >= 1 && P <= (1 << 26), "s3fd_candidates: batch %d, %d priors", batch, P);
  CASYNC_REQUIRE(cap >= 1 && cap <= P, "s3fd_candidates: cap %d (1..%d priors)", cap, P);
  return casync_launch(face_candidates_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, det, P, thresh, cap, counts, rows);
}

int casync_op_landmarks_finalize(const float* y, const float* mean_face, const int32_t* geom, int n, int32_t* out,
                                 casync_stream stream) {
  CASYNC_REQUIRE(y && mean_face && geom && out, "landmarks_finalize: null pointer");
  CASYNC_REQUIRE(n >= 1 && n <= (1 << 20), "landmarks_finalize: %d rows (1..%d)", n, 1 << 20);
  CropBlock blk;
  for (int first = 0; first < n; first += CROPS_PER_LAUNCH) {
    const int m = n - first < CROPS_PER_LAUNCH ? n - first : CROPS_PER_LAUNCH;
    if (int st = fill_block(geom, first, m, -1, "landmarks_finalize", blk)) return st;
  }
  for (int first = 0; first < n; first += CROPS_PER_LAUNCH) {
    const int m = n - first < CROPS_PER_LAUNCH ? n - first : CROPS_PER_LAUNCH;
    fill_block(geom, first, m, -1, "landmarks_finalize", blk);
    if (int st = casync_launch(face_finalize_kernel, dim3(m), dim3(128), 0, (hipStream_t)stream, y + (size_t)first * 220, mean_face, blk,
                               out + (size_t)first * 220))
      return st;
  }
  return CASYNC_OK;
}

}  // extern "C"
