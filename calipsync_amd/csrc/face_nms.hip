// S3FD's two non-maximum suppressions on the device: the candidate rows of casync_op_s3fd_candidates -> the face rows that
// S3FD.detect_faces returns, so that only the faces themselves come back to the host.
//
//   stage 1:  Detect.forward's nms in float32, IoU 0.3, 750 kept                            box_utils.py:62-173
//   stage 2:  the "> conf_th" walk, float32 scaling to pixels, float64 rows, nms_(rows, 0.1)   main.py:45-58, box_utils.py:7-38
//
// calipsync_amd/facedet.py restates both in numpy (nms_f32 / detect_output, detect_faces_rows / nms_); every operation in them
// is one IEEE add, subtract, multiply, divide, max, min or compare in a stated type, and the -m gpu tests demand bit equality
// with them (tests/test_face_nms_gpu.py).
//
// One 256-lane workgroup per frame, everything in static LDS, no atomics.  A pass is a rank-by-counting sort (stable by
// construction: among equal scores the higher row index is visited first, which is what the stable ascending argsort popped
// from its end gives) followed by the greedy walk over the sorted rows.  A lane owns the rows at sorted positions lane + 256 r
// and keeps them in registers; after a row is kept every lane tests its own surviving rows against it, the waves publish
// their survivors as 64-bit ballots, and after ONE barrier every lane finds the next survivor itself from those words (two
// sets of words, alternating, so a fast wave never overwrites what a slow one still reads).
//
// n <= MAX_ROWS (1024) by construction: the entry refuses a larger cap and a frame with counts[b] > cap is not touched.  Every
// loop below is bounded by that clamp, never by a value read from device memory alone.  Specified for finite boxes and
// non-NaN scores (what the detector emits above CONF_THRESH); any other bits stay inside the buffers and give unspecified rows.
//
// Floating point here has to round like numpy on the host: no contraction, and the roundings that matter are spelled out.
#pragma clang fp contract(off)
#include "common.h"

namespace {

constexpr int MAX_ROWS = 1024;            // cap of the candidate rows per frame
constexpr int TOP_K = 750;                // Detect.top_k: rows of Detect.forward's output per class
// (Detect.nms_top_k = 5000 cuts the sorted rows to the 5000 best before the walk: it can never bite at cap <= 1024.)
constexpr int ROUNDS1 = MAX_ROWS / 256;   // sorted positions a lane owns in stage 1
constexpr int ROUNDS2 = (TOP_K + 255) / 256;   // ... and in stage 2 (at most TOP_K - 1 rows reach it)
constexpr int WORDS = MAX_ROWS / 64;

__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float div_rn(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float max_of(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ float min_of(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double sub_rn(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double div_rn(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ double add_rn(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double max_of(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ double min_of(double a, double b) { return fmin(a, b); }

// The sorted rows of a pass: float32 in LDS for both (stage 2's pixels are float32 products, widened exactly when read).
struct Sorted {
  float x1[MAX_ROWS], y1[MAX_ROWS], x2[MAX_ROWS], y2[MAX_ROWS], score[MAX_ROWS];
};

template <typename T> struct Box { T x1, y1, x2, y2, area; };

template <typename T> __device__ __forceinline__ Box<T> box_at(const Sorted& s, int p) {
  Box<T> b{(T)s.x1[p], (T)s.y1[p], (T)s.x2[p], (T)s.y2[p], (T)0};
  b.area = mul_rn(sub_rn(b.x2, b.x1), sub_rn(b.y2, b.y1));
  return b;
}

// row j outlives the kept row i: the overlap ratio, written in the positive form so that a NaN (0 / 0) drops the row
template <typename T> __device__ __forceinline__ bool outlives(const Box<T>& j, const Box<T>& i, T thresh) {
  const T w = max_of(sub_rn(min_of(j.x2, i.x2), max_of(j.x1, i.x1)), (T)0);
  const T h = max_of(sub_rn(min_of(j.y2, i.y2), max_of(j.y1, i.y1)), (T)0);
  const T inter = mul_rn(w, h);
  const T uni = sizeof(T) == 4 ? add_rn(sub_rn(j.area, inter), i.area)      // nms: (area[idx] - inter) + area[i]
                               : sub_rn(add_rn(i.area, j.area), inter);      // nms_: (areas[i] + areas[order[1:]]) - inter
  return div_rn(inter, uni) <= thresh;
}

// position of row j in visiting order: the rows with a higher score, and those with the same score and a higher index
__device__ __forceinline__ int visit_rank(const float* score, int n, int j, float sj) {
  int rank = 0;
#pragma unroll 4
  for (int k = 0; k < n; ++k) {
    const float sk = score[k];
    rank += (sk > sj || (sk == sj && k > j)) ? 1 : 0;
  }
  return rank;
}

// The greedy walk over n sorted rows (n >= 1): keep the first survivor, drop what overlaps it, up to `limit` kept rows.
// -> the number kept; keep[0 .. kept) are their sorted positions, ascending.  Ends behind a barrier.
template <typename T, int ROUNDS>
__device__ __forceinline__ int greedy_walk(const Sorted& s, int n, int limit, T thresh, unsigned long long (*words)[WORDS], int* keep) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Box<T> mine[ROUNDS];
  bool alive[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int p = r * 256 + threadIdx.x;
    alive[r] = p < n;
    mine[r] = box_at<T>(s, alive[r] ? p : 0);
  }
  int cur = 0, kept = 0;
  for (int it = 0; it < limit && cur < n; ++it) {          // cur grows by at least one per trip: at most n <= MAX_ROWS trips
    if (threadIdx.x == 0) keep[kept] = cur;
    ++kept;
    const Box<T> top = box_at<T>(s, cur);
    unsigned long long* w = words[it & 1];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const int p = r * 256 + threadIdx.x;
      bool a = alive[r] && p > cur;
      if (a) a = outlives(mine[r], top, thresh);
      alive[r] = a;
      const unsigned long long votes = __ballot(a);
      if (lane == 0) w[r * 4 + wave] = votes;
    }
    __syncthreads();
    const unsigned long long word = lane < ROUNDS * 4 ? w[lane] : 0ull;
    const unsigned long long filled = __ballot(word != 0ull);
    if (!filled) {
      cur = n;
    } else {
      const int first = __ffsll((long long)filled) - 1;
      cur = first * 64 + __ffsll((long long)__shfl(word, first)) - 1;
    }
  }
  return kept;
}

__global__ __launch_bounds__(256) void face_nms_kernel(const float* __restrict__ rows, const int* __restrict__ counts, int cap, float fw,
                                                       float fh, float conf_th, int* __restrict__ status, double* __restrict__ faces,
                                                       float* __restrict__ detect_out, int* __restrict__ detect_n) {
  __shared__ Sorted sorted;                                  // 20 KB
  __shared__ float score_in[MAX_ROWS];                       // scores in arrival order: what the ranks are counted over
  __shared__ int keep[TOP_K];
  __shared__ unsigned long long words[2][WORDS];
  __shared__ int first_fail[ROUNDS2 * 4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int n = counts[b];
  if (n > cap) {                                             // the host falls back to this frame's dense rows
    if (threadIdx.x == 0) status[b] = -1;
    return;
  }
  n = n < 0 ? 0 : (n > MAX_ROWS ? MAX_ROWS : n);
  if (n == 0) {
    if (threadIdx.x == 0) {
      status[b] = 0;
      if (detect_n) detect_n[b] = 0;
    }
    return;
  }

  // ---- stage 1: float32, IoU <= 0.3, TOP_K kept
  const float* in = rows + (size_t)b * cap * 5;
  float mine[ROUNDS1][5];
#pragma unroll
  for (int r = 0; r < ROUNDS1; ++r) {
    const int j = r * 256 + threadIdx.x;
    if (j < n) {
#pragma unroll
      for (int c = 0; c < 5; ++c) mine[r][c] = in[(size_t)j * 5 + c];
      score_in[j] = mine[r][0];
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < ROUNDS1; ++r) {
    const int j = r * 256 + threadIdx.x;
    if (j < n) {
      const int p = visit_rank(score_in, n, j, mine[r][0]);
      sorted.score[p] = mine[r][0];
      sorted.x1[p] = mine[r][1]; sorted.y1[p] = mine[r][2]; sorted.x2[p] = mine[r][3]; sorted.y2[p] = mine[r][4];
    }
  }
  __syncthreads();
  const int kept = greedy_walk<float, ROUNDS1>(sorted, n, TOP_K, 0.3f, words, keep);
  if (detect_out) {
    float* o = detect_out + (size_t)b * TOP_K * 5;
    for (int k = threadIdx.x; k < kept; k += 256) {
      const int p = keep[k];
      o[k * 5] = sorted.score[p];
      o[k * 5 + 1] = sorted.x1[p]; o[k * 5 + 2] = sorted.y1[p]; o[k * 5 + 3] = sorted.x2[p]; o[k * 5 + 4] = sorted.y2[p];
    }
    if (threadIdx.x == 0) detect_n[b] = kept;
  }

  // ---- stage 2: the rows of Detect.forward's [750,5] output (zeros behind the kept ones) while their score > conf_th
  float px[ROUNDS2][5];
#pragma unroll
  for (int r = 0; r < ROUNDS2; ++r) {
    const int k = r * 256 + threadIdx.x;
    const int p = k < kept ? keep[k] : 0;
    px[r][0] = k < kept ? sorted.score[p] : 0.f;
    px[r][1] = mul_rn(sorted.x1[p], fw); px[r][2] = mul_rn(sorted.y1[p], fh);     // pt = box * (W, H, W, H) in float32
    px[r][3] = mul_rn(sorted.x2[p], fw); px[r][4] = mul_rn(sorted.y2[p], fh);
    const unsigned long long fails = __ballot(k < TOP_K && !(px[r][0] > conf_th));
    if (lane == 0) first_fail[r * 4 + wave] = fails ? r * 256 + wave * 64 + __ffsll((long long)fails) - 1 : TOP_K;
  }
  __syncthreads();                                           // (also: every lane is done with sorted and keep)
  int m = TOP_K;
#pragma unroll
  for (int i = ROUNDS2 * 4 - 1; i >= 0; --i) m = first_fail[i] < TOP_K ? first_fail[i] : m;
  if (m >= TOP_K) {                                          // all 750 pass: the reference walks off the array (IndexError)
    if (threadIdx.x == 0) status[b] = -2;
    return;
  }
  if (m == 0) {
    if (threadIdx.x == 0) status[b] = 0;
    return;
  }
  // (m <= kept: behind the kept rows the score is 0, which passes only a negative conf_th, and then nothing behind fails)
#pragma unroll
  for (int r = 0; r < ROUNDS2; ++r) {
    const int k = r * 256 + threadIdx.x;
    if (k < m) score_in[k] = px[r][0];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < ROUNDS2; ++r) {
    const int k = r * 256 + threadIdx.x;
    if (k < m) {
      const int p = visit_rank(score_in, m, k, px[r][0]);
      sorted.score[p] = px[r][0];
      sorted.x1[p] = px[r][1]; sorted.y1[p] = px[r][2]; sorted.x2[p] = px[r][3]; sorted.y2[p] = px[r][4];
    }
  }
  __syncthreads();
  const int n_faces = greedy_walk<double, ROUNDS2>(sorted, m, m, 0.1, words, keep);
  double* o = faces + (size_t)b * TOP_K * 5;
  for (int k = threadIdx.x; k < n_faces; k += 256) {         // bboxes[nms_(bboxes, 0.1)]: (x1, y1, x2, y2, score)
    const int p = keep[k];
    o[k * 5] = (double)sorted.x1[p]; o[k * 5 + 1] = (double)sorted.y1[p]; o[k * 5 + 2] = (double)sorted.x2[p];
    o[k * 5 + 3] = (double)sorted.y2[p]; o[k * 5 + 4] = (double)sorted.score[p];
  }
  if (threadIdx.x == 0) status[b] = n_faces;
}

}  // namespace

extern "C" {

int casync_op_s3fd_nms(const float* rows, const int32_t* counts, int batch, int cap, int width, int height, float conf_th,
                       int32_t* status, double* faces, float* detect_out, int32_t* detect_n, casync_stream stream) {
  CASYNC_REQUIRE(rows && counts && status && faces, "s3fd_nms: null pointer");
  CASYNC_REQUIRE((detect_out == nullptr) == (detect_n == nullptr), "s3fd_nms: detect_out and detect_n go together (both or neither)");
  CASYNC_REQUIRE(batch >= 1 && batch <= 65535, "s3fd_nms: batch %d (1..65535)", batch);
  CASYNC_REQUIRE(cap >= 1 && cap <= MAX_ROWS, "s3fd_nms: cap %d (1..%d rows per frame)", cap, MAX_ROWS);
  CASYNC_REQUIRE(width >= 1 && height >= 1, "s3fd_nms: frame of %d x %d (w x h)", width, height);
  return casync_launch(face_nms_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, rows, counts, cap, (float)width, (float)height,
                       conf_th, status, faces, detect_out, detect_n);
}

}  // extern "C"
