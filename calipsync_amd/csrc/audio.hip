// The audio front end of the HuBERT leg: the PCM bytes of a WAV file -> the mono 16 kHz waveform and its Wav2Vec2 normalisation.
//
//   decode:     u8 (v - 128) / 128, i16 v / 2^15, i24 v / 2^23, i32 v / 2^31 (little endian), each an fp32 value
//   downmix:    mono 0 ("mean"): the channels summed in channel order in fp32, divided once by C; mono 1 ("first"): channel 0
//   resample:   y[k] = sum_i x[i] h[k down + half - i up], half = (n_taps - 1) / 2, zeros outside both arrays: a polyphase FIR
//               whose taps are an ARGUMENT (calipsync_amd/audio.py resample_taps designs scipy.signal.resample_poly's)
//   normalise:  out = (x - mean) (var + 1e-7)^-1/2 over the whole utterance, the moments summed in float64
//
// wav_resample_kernel<WIDTH>: one workgroup makes OUT_PER_WG consecutive outputs.  The input frames they reach are one span of
// the file; it is decoded and downmixed straight from the PCM bytes into an fp32 tile in LDS (16-byte loads over the part of
// the span where a frame never straddles a vector, single bytes elsewhere), then each thread sums the taps of its outputs in
// ascending i with one fp32 fma chain.  The taps stay in global memory: a bank is 2 half + 1 floats, 320,021 of them at
// 16001 Hz.  Every k down, i up and byte offset is 64-bit: k * 441 passes 2^31 after five minutes of 44.1 kHz audio.
// wav_convert_kernel<WIDTH>: the same decode into global memory, for input that is already at 16 kHz (up == down).
// wav_moments_kernel / wav_moments_final_kernel: float64 sum and sum of squares, per block over a fixed span in a fixed order,
// then one block over the partials: no atomics, so the bits repeat from call to call.  wav_normalize_kernel applies them.
// No scratch, no inline assembly, no atomics.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int OUT_PER_WG = 512;           // outputs of one workgroup of the resample kernel
constexpr int TILE_IN = 8192;             // fp32 input frames a workgroup can stage (32 KB of LDS)
constexpr int CONVERT_PER_WG = 4096;      // frames of one workgroup of the convert kernel
constexpr int MOMENT_BLOCKS = 512;        // at most this many partial sums
constexpr int MOMENT_MIN_SPAN = 4096;     // samples a moments block sums at least
constexpr int MAX_CHANNELS = 16;
constexpr int WS_HEAD = 4;                // doubles ahead of the partials: mean, var, {float mean, float rstd}, 0

template <int WIDTH> __device__ __forceinline__ float pcm_scale();
template <> __device__ __forceinline__ float pcm_scale<1>() { return 1.f / 128.f; }
template <> __device__ __forceinline__ float pcm_scale<2>() { return 1.f / 32768.f; }
template <> __device__ __forceinline__ float pcm_scale<3>() { return 1.f / 8388608.f; }
template <> __device__ __forceinline__ float pcm_scale<4>() { return 1.f / 2147483648.f; }

// one sample from its bytes (any alignment)
template <int WIDTH> __device__ __forceinline__ float pcm_value(const unsigned char* p) {
  int v;
  if (WIDTH == 1) v = (int)p[0] - 128;
  else if (WIDTH == 2) v = (int)(short)((unsigned)p[0] | ((unsigned)p[1] << 8));
  else if (WIDTH == 3) v = (int)(((unsigned)p[0] << 8) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 24)) >> 8;
  else v = (int)((unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24));
  return (float)v * pcm_scale<WIDTH>();     // int -> fp32 rounds to nearest even (i32 only), the power of two is exact
}

// sample S of a 16-byte vector of WIDTH 1, 2 or 4 (S is a constant after unrolling: no indexed registers)
template <int WIDTH, int S> __device__ __forceinline__ float vec_value(const uint4& q) {
  constexpr int BYTE = S * WIDTH, WORD = BYTE / 4, SHIFT = (BYTE % 4) * 8;
  const unsigned w = WORD == 0 ? q.x : WORD == 1 ? q.y : WORD == 2 ? q.z : q.w;
  int v;
  if (WIDTH == 1) v = (int)((w >> SHIFT) & 0xffu) - 128;
  else if (WIDTH == 2) v = (int)(short)((w >> SHIFT) & 0xffffu);
  else v = (int)w;
  return (float)v * pcm_scale<WIDTH>();
}

template <int WIDTH, int S> struct VecFrames {
  // the frames of one vector: samples S .. 16 / WIDTH - 1, `acc` the channels of the open frame so far
  static __device__ __forceinline__ void run(const uint4& q, int channels, int lg, int mono, float acc, float* dst) {
    const float v = vec_value<WIDTH, S>(q);
    const int c = S & (channels - 1);
    acc = c == 0 ? v : acc + v;
    if (mono) {
      if (c == 0) dst[S >> lg] = v;
    } else if (c == channels - 1) {
      dst[S >> lg] = acc / (float)channels;
    }
    VecFrames<WIDTH, S + 1>::run(q, channels, lg, mono, acc, dst);
  }
};
template <int WIDTH> struct VecFrames<WIDTH, 16 / WIDTH> {
  static __device__ __forceinline__ void run(const uint4&, int, int, int, float, float*) {}
};

// frame `f` of the file from single bytes
template <int WIDTH> __device__ __forceinline__ float frame_value(const unsigned char* pcm, long long f, int channels, int mono) {
  const unsigned char* p = pcm + f * (long long)(channels * WIDTH);
  float acc = pcm_value<WIDTH>(p);
  if (mono || channels == 1) return acc;
  for (int c = 1; c < channels; ++c) acc += pcm_value<WIDTH>(p + c * WIDTH);
  return acc / (float)channels;
}

// frames [f0, f0 + count) of the file, decoded and downmixed -> dst[0 .. count), by the THREADS threads of a workgroup.
// Vectors cover only whole frames inside the span, so nothing outside the span's bytes is read.
template <int WIDTH> __device__ __forceinline__ void decode_span(const unsigned char* __restrict__ pcm, long long f0, int count, int channels,
                                                                 int mono, float* dst) {
  const int fs = channels * WIDTH;                                   // bytes of a frame
  const unsigned char* base = pcm + f0 * (long long)fs;
  int head = count, n_vec = 0, lg = 0;
  if (WIDTH != 3 && (fs & (fs - 1)) == 0 && fs <= 16 && ((uintptr_t)pcm & (uintptr_t)(fs - 1)) == 0) {
    while ((1 << lg) < channels) ++lg;
    const int head_bytes = (int)((0 - (uintptr_t)base) & 15u);      // a multiple of fs: base is fs-aligned
    head = head_bytes / fs < count ? head_bytes / fs : count;
    n_vec = (int)(((long long)(count - head) * fs) / 16);
  }
  const int per_vec = WIDTH == 3 ? 1 : 16 / fs;                      // frames of a vector (unused when n_vec == 0)
  const int body = n_vec * per_vec;
  if constexpr (WIDTH != 3) {
    const uint4* v = reinterpret_cast<const uint4*>(base + (long long)head * fs);
    for (int j = threadIdx.x; j < n_vec; j += THREADS) {
      const uint4 q = v[j];
      VecFrames<WIDTH, 0>::run(q, channels, lg, mono, 0.f, dst + head + j * per_vec);
    }
  }
  for (int j = threadIdx.x; j < count - body; j += THREADS) {        // ahead of the first vector and behind the last
    const int f = j < head ? j : j + body;
    dst[f] = frame_value<WIDTH>(pcm, f0 + f, channels, mono);
  }
}

__device__ __forceinline__ long long first_input(long long centre, long long half, long long up) {
  const long long lo = centre - half;                                // i up >= centre - half
  return lo <= 0 ? 0 : (lo + up - 1) / up;
}

template <int WIDTH>
__global__ __launch_bounds__(THREADS) void wav_resample_kernel(const unsigned char* __restrict__ pcm, int channels, long long frames, int mono,
                                                               long long up, long long down, const float* __restrict__ taps, long long half,
                                                               float* __restrict__ out, long long n_out) {
  __shared__ float tile[TILE_IN];
  const long long k0 = (long long)blockIdx.x * OUT_PER_WG;
  const long long k_last = (k0 + OUT_PER_WG < n_out ? k0 + OUT_PER_WG : n_out) - 1;
  const long long i0 = first_input(k0 * down, half, up);
  long long i_end = (k_last * down + half) / up;                     // the last frame any output of this workgroup reaches
  if (i_end > frames - 1) i_end = frames - 1;
  long long count = i_end - i0 + 1;                                  // <= TILE_IN: checked on the host
  if (count > TILE_IN) count = TILE_IN;
  if (count > 0) decode_span<WIDTH>(pcm, i0, (int)count, channels, mono, tile);
  __syncthreads();
  for (int o = threadIdx.x; o < OUT_PER_WG; o += THREADS) {
    const long long k = k0 + o;
    if (k > k_last) break;
    const long long centre = k * down;
    const long long lo = first_input(centre, half, up);
    long long hi = (centre + half) / up;
    if (hi > i0 + count - 1) hi = i0 + count - 1;
    const float* x = tile + (lo - i0);
    const float* h = taps + (centre + half - lo * up);               // 0 <= index <= 2 half, stepping down by `up`
    const int n = (int)(hi - lo + 1);
    float acc = 0.f;
    for (int j = 0; j < n; ++j) acc = fmaf(x[j], h[-(long long)j * up], acc);
    out[k] = acc;
  }
}

template <int WIDTH>
__global__ __launch_bounds__(THREADS) void wav_convert_kernel(const unsigned char* __restrict__ pcm, int channels, long long frames, int mono,
                                                              float* __restrict__ out) {
  const long long f0 = (long long)blockIdx.x * CONVERT_PER_WG;
  const long long left = frames - f0;
  const int count = left < CONVERT_PER_WG ? (int)left : CONVERT_PER_WG;
  if (count > 0) decode_span<WIDTH>(pcm, f0, count, channels, mono, out + f0);
}

// sum over the THREADS values of a workgroup in a fixed tree -> thread 0
__device__ __forceinline__ double block_sum(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}

// block b: samples [b span, (b + 1) span) -> partial[2 b] = sum, partial[2 b + 1] = sum of squares
__global__ __launch_bounds__(THREADS) void wav_moments_kernel(const float* __restrict__ x, long long n, long long span, double* __restrict__ partial) {
  __shared__ double lds[THREADS];
  const long long a = (long long)blockIdx.x * span;
  const long long b = a + span < n ? a + span : n;
  double s = 0.0, q = 0.0;
  for (long long i = a + threadIdx.x; i < b; i += THREADS) {
    const double v = (double)x[i];
    s += v;
    q += v * v;
  }
  s = block_sum(s, lds);
  q = block_sum(q, lds);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = s;
    partial[2 * blockIdx.x + 1] = q;
  }
}

// one block: head[0] = mean, head[1] = population variance, head[2] = {(float)mean, (float)(var + 1e-7)^-1/2}
__global__ __launch_bounds__(THREADS) void wav_moments_final_kernel(const double* __restrict__ partial, int blocks, long long n, double* __restrict__ head) {
  __shared__ double lds[THREADS];
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < blocks; i += THREADS) {
    s += partial[2 * i];
    q += partial[2 * i + 1];
  }
  s = block_sum(s, lds);
  q = block_sum(q, lds);
  if (threadIdx.x == 0) {
    const double mean = s / (double)n;
    double var = q / (double)n - mean * mean;
    if (var < 0.0) var = 0.0;
    head[0] = mean;
    head[1] = var;
    float* f = reinterpret_cast<float*>(head + 2);
    f[0] = (float)mean;
    f[1] = (float)(1.0 / sqrt(var + 1e-7));
    head[3] = 0.0;
  }
}

// vec: x and out are 16-byte aligned, four samples to a thread; the last n % 4 one by one.  out may be x (neither is __restrict__):
// a thread reads what it writes and nothing else
__global__ __launch_bounds__(THREADS) void wav_normalize_kernel(const float* x, long long n, const double* __restrict__ head, int vec, float* out) {
  const float* f = reinterpret_cast<const float*>(head + 2);
  const float mean = f[0], rstd = f[1];
  const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (vec) {
    const long long n4 = n / 4;
    if (t < n4) {
      f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * t);
      v[0] = (v[0] - mean) * rstd;
      v[1] = (v[1] - mean) * rstd;
      v[2] = (v[2] - mean) * rstd;
      v[3] = (v[3] - mean) * rstd;
      *reinterpret_cast<f32x4*>(out + 4 * t) = v;
    } else if (t < n4 + (n & 3)) {
      const long long i = 4 * n4 + (t - n4);
      out[i] = (x[i] - mean) * rstd;
    }
  } else if (t < n) {
    out[t] = (x[t] - mean) * rstd;
  }
}

int moment_blocks(long long n, long long* span) {
  long long s = (n + MOMENT_BLOCKS - 1) / MOMENT_BLOCKS;
  if (s < MOMENT_MIN_SPAN) s = MOMENT_MIN_SPAN;
  *span = s;
  return (int)((n + s - 1) / s);
}

template <int WIDTH>
int launch_front(const uint8_t* pcm, int channels, long long frames, int mono, long long up, long long down, const float* taps, long long half,
                 float* out, long long n_out, hipStream_t s) {
  if (up == down) {
    const unsigned grid = (unsigned)((frames + CONVERT_PER_WG - 1) / CONVERT_PER_WG);
    return casync_launch(wav_convert_kernel<WIDTH>, dim3(grid), dim3(THREADS), 0, s, pcm, channels, frames, mono, out);
  }
  const unsigned grid = (unsigned)((n_out + OUT_PER_WG - 1) / OUT_PER_WG);
  return casync_launch(wav_resample_kernel<WIDTH>, dim3(grid), dim3(THREADS), 0, s, pcm, channels, frames, mono, up, down, taps, half, out, n_out);
}

}  // namespace

extern "C" {

int64_t casync_audio_out_samples(int64_t n, int rate) {
  if (n < 0 || rate < 1) return -1;
  long long a = rate, b = 16000;
  while (b) {
    const long long t = a % b;
    a = b;
    b = t;
  }
  const long long up = 16000 / a, down = rate / a;
  if (n > (INT64_MAX - down) / up) return -1;
  return (n * up + down - 1) / down;
}

int64_t casync_op_audio_workspace_bytes(int64_t n_out) {
  if (n_out < 1) return -1;
  return (int64_t)sizeof(double) * (WS_HEAD + 2 * MOMENT_BLOCKS);
}

int casync_op_audio_resample(const uint8_t* pcm, int width, int channels, int64_t frames, int mono, int up, int down, const float* taps_dev,
                             int64_t n_taps, float* out, int64_t n_out, casync_stream stream) {
  CASYNC_REQUIRE(pcm && out, "audio_resample: null pointer");
  CASYNC_REQUIRE(width >= 1 && width <= 4, "audio_resample: samples of %d bytes (1..4)", width);
  CASYNC_REQUIRE(channels >= 1 && channels <= MAX_CHANNELS, "audio_resample: %d channels (1..%d)", channels, MAX_CHANNELS);
  CASYNC_REQUIRE(mono == 0 || mono == 1, "audio_resample: mono %d (0: mean, 1: first)", mono);
  CASYNC_REQUIRE(up >= 1 && down >= 1, "audio_resample: up %d, down %d", up, down);
  CASYNC_REQUIRE(frames >= 1 && frames <= (int64_t)1 << 40, "audio_resample: %lld frames", (long long)frames);
  CASYNC_REQUIRE(((uintptr_t)out & 3u) == 0, "audio_resample: out is not 4-byte aligned");
  const long long want = ((long long)frames * up + down - 1) / down;
  CASYNC_REQUIRE(n_out == want, "audio_resample: n_out %lld, %lld frames by %d / %d give %lld", (long long)n_out, (long long)frames, up, down, want);
  CASYNC_REQUIRE((want + OUT_PER_WG - 1) / OUT_PER_WG <= 0x7fffffffLL && (frames + CONVERT_PER_WG - 1) / CONVERT_PER_WG <= 0x7fffffffLL,
                 "audio_resample: %lld frames are more than one launch takes", (long long)frames);
  long long half = 0;
  if (up != down) {
    CASYNC_REQUIRE(taps_dev && ((uintptr_t)taps_dev & 3u) == 0, "audio_resample: taps null or not 4-byte aligned");
    CASYNC_REQUIRE(n_taps >= 1 && (n_taps & 1) == 1 && n_taps <= (int64_t)1 << 30, "audio_resample: %lld taps (odd, at least 1)", (long long)n_taps);
    half = (n_taps - 1) / 2;
    const long long reach = ((long long)(OUT_PER_WG - 1) * down + 2 * half) / up + 2;   // frames under the outputs of one workgroup
    CASYNC_REQUIRE(reach <= TILE_IN, "audio_resample: %d / %d with %lld taps reaches %lld frames per %d outputs (at most %d)", up, down,
                   (long long)n_taps, reach, OUT_PER_WG, TILE_IN);
  }
  hipStream_t s = (hipStream_t)stream;
  switch (width) {
    case 1: return launch_front<1>(pcm, channels, frames, mono, up, down, taps_dev, half, out, n_out, s);
    case 2: return launch_front<2>(pcm, channels, frames, mono, up, down, taps_dev, half, out, n_out, s);
    case 3: return launch_front<3>(pcm, channels, frames, mono, up, down, taps_dev, half, out, n_out, s);
    default: return launch_front<4>(pcm, channels, frames, mono, up, down, taps_dev, half, out, n_out, s);
  }
}

int casync_op_audio_normalize(const float* x, int64_t n, void* workspace, float* out, casync_stream stream) {
  CASYNC_REQUIRE(x && workspace && out, "audio_normalize: null pointer");
  CASYNC_REQUIRE(n >= 1 && n <= (int64_t)1 << 36, "audio_normalize: %lld samples", (long long)n);
  CASYNC_REQUIRE(((uintptr_t)x & 3u) == 0 && ((uintptr_t)out & 3u) == 0, "audio_normalize: x or out is not 4-byte aligned");
  CASYNC_REQUIRE(((uintptr_t)workspace & 7u) == 0, "audio_normalize: workspace is not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  double* head = static_cast<double*>(workspace);
  double* partial = head + WS_HEAD;
  long long span;
  const int blocks = moment_blocks(n, &span);
  if (int st = casync_launch(wav_moments_kernel, dim3(blocks), dim3(THREADS), 0, s, x, (long long)n, span, partial)) return st;
  if (int st = casync_launch(wav_moments_final_kernel, dim3(1), dim3(THREADS), 0, s, (const double*)partial, blocks, (long long)n, head)) return st;
  const int vec = (((uintptr_t)x | (uintptr_t)out) & 15u) == 0;
  const long long threads = vec ? n / 4 + (n & 3) : n;
  const unsigned grid = (unsigned)((threads + THREADS - 1) / THREADS);
  return casync_launch(wav_normalize_kernel, dim3(grid), dim3(THREADS), 0, s, x, (long long)n, (const double*)head, vec, out);
}

}  // extern "C"
