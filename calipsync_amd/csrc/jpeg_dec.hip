// Baseline JPEG files -> uint8 BGR frames [B,H,W,3] on the device, byte for byte what libjpeg's default integer path decodes
// (islow inverse DCT, fancy chroma upsampling, 16-bit fixed-point colour; calipsync_amd/jpeg.py decode_jpeg_host is the numpy
// twin).  The encoders are csrc/jpeg_enc.hip and csrc/jpeg_enc420.hip; this file shares no code with them;
// what it shares with its wider sibling csrc/jpeg_dec_mjpeg.hip is csrc/jpeg_dec_common.h.
//
// A Huffman stream has no index: where a code starts is known only to a decoder that read everything before it.  Files without
// restart markers are the normal input, so the scan of every restart segment is cut into subsequences of chunk_bits bits of the
// stuffed stream, and the state a serial decoder would have at every cut (bit position, block slot of the MCU, zigzag index) is
// found by a fixed-point iteration (a decoder that starts in a wrong state usually falls into step with the right one):
//
//   jpegdec_sync_kernel    one workgroup per frame, the frame's Huffman tables in LDS.  The first subsequence of a segment starts
//                          in the known state, every other from the guess (its first bit, slot 0, zigzag 0).  A round decodes
//                          every subsequence whose entry state changed, one lane each, and hands its exit state to the next
//                          subsequence of the segment; the rounds end when no entry state changes.  Subsequence k of a segment
//                          is right after at most k rounds, so the loop ends on every input with the serial decoder's states.  A
//                          subsequence that meets an invalid code hands on the next guess, so that a wrong guess which runs into
//                          one spoils nothing behind it.  Then a segmented prefix sum over the subsequences (blocks finished, DC
//                          differences per component; what follows the first invalid code of a segment counts for nothing) gives
//                          each its first block and its DC predictors, and the frame its status.
//   jpegdec_write_kernel   one lane per subsequence again, from the verified state: the coefficients go into a zeroed int16
//                          [block][64] scratch in natural order, DC as values.
//   jpegdec_idct_kernel    one lane per block: dequantisation, the two passes of jidctint in registers, +128, clamp, eight 8-byte
//                          stores into the component's sample plane.
//   jpegdec_color_kernel   one lane per four pixels of a row: chroma upsampled from the real downsampled plane with libjpeg's
//                          triangle filter (edge rows and columns repeated), YCbCr -> BGR, 4-byte stores where the row allows.
//
// Bounds: no stream content forms an address or bounds a loop.  Bit reads past a segment's end return zeros; the tables and the
// segment list lie in device memory and every value read from them is clamped or masked before use; the zigzag index is checked
// before every coefficient store; a segment writes at most the blocks the frame geometry gives it; every symbol consumes at least
// one bit, so a subsequence's loop is bounded by its bits.  The output is a pure function of the input: no global atomics, and
// every round of the iteration is separated from the next by workgroup barriers.
#include "jpeg_dec_common.h"

namespace {

// The samplings of this decoder: sub 0 is 4:4:4 (an MCU of three blocks on 8 x 8 pixels), anything else 4:2:0 (six on 16 x 16)
struct Baseline {
  __host__ __device__ static inline Geo geometry(int H, int W, int sub, int ri) {
    Geo g;
    const int s = sub ? 16 : 8;
    g.bpm = sub ? 6 : 3;
    g.mrows = (H + s - 1) / s;
    g.mcols = (W + s - 1) / s;
    g.n_mcu = g.mrows * g.mcols;
    g.ri = ri > 0 && ri < g.n_mcu ? ri : g.n_mcu;
    return g;
  }
  __device__ static __forceinline__ int comp(int bpm, int s) { return bpm == 3 ? s : (s < 4 ? 0 : s - 3); }
};
__host__ __device__ inline Geo geometry(int H, int W, int sub, int ri) { return Baseline::geometry(H, W, sub, ri); }

__global__ __launch_bounds__(SYNC_THREADS) void jpegdec_sync_kernel(const unsigned char* __restrict__ data, DecRecs recs, int frame0, int H, int W,
                                                                    int chunk_bits, SubState* subs_all, int* __restrict__ status) {
  sync_body<Baseline>(data, recs, frame0, H, W, chunk_bits, subs_all, status);
}

__global__ __launch_bounds__(256) void jpegdec_write_kernel(const unsigned char* __restrict__ data, DecRecs recs, int frame0, int H, int W, int chunk_bits,
                                                            const SubState* __restrict__ subs_all, short* __restrict__ coef_all, long long coef_stride) {
  write_body<Baseline>(data, recs, frame0, H, W, chunk_bits, subs_all, coef_all, coef_stride);
}

// The sample planes of a frame: 4:4:4 three planes of 8 mrows x 8 mcols; 4:2:0 Y of 16 mrows x 16 mcols, then Cb and Cr of half that each way
struct Planes { long long off[3]; int pw[3]; };
__device__ __forceinline__ Planes planes_of(const Geo& g) {
  Planes p;
  if (g.bpm == 3) {
    const long long sz = 64ll * g.n_mcu;
    p.off[0] = 0, p.off[1] = sz, p.off[2] = 2 * sz;
    p.pw[0] = p.pw[1] = p.pw[2] = 8 * g.mcols;
  } else {
    const long long sz = 256ll * g.n_mcu;
    p.off[0] = 0, p.off[1] = sz, p.off[2] = sz + sz / 4;
    p.pw[0] = 16 * g.mcols, p.pw[1] = p.pw[2] = 8 * g.mcols;
  }
  return p;
}

// grid (ceil(blocks of the largest frame / 64), frames of this launch), 64 threads.
__global__ __launch_bounds__(64) void jpegdec_idct_kernel(const unsigned char* __restrict__ data, DecRecs recs, int frame0, int H, int W,
                                                          const short* __restrict__ coef_all, long long coef_stride, unsigned char* __restrict__ planes_all,
                                                          long long plane_stride) {
  __shared__ unsigned short q_s[192];
  const DecRec rec = recs.r[blockIdx.y];
  if (rec.pre_status) return;
  const Geo geo = geometry(H, W, rec.sub, rec.ri);
  const int blocks = geo.n_mcu * geo.bpm;
  if ((int)(blockIdx.x * 64u) >= blocks) return;                // uniform
  {
    const unsigned short* q = reinterpret_cast<const unsigned short*>(data + rec.tab_off);
    for (int i = threadIdx.x; i < 192; i += 64) q_s[i] = q[i];
  }
  __syncthreads();
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= blocks) return;
  const int mcu = b / geo.bpm, slot = b - mcu * geo.bpm;
  const int my = mcu / geo.mcols, mx = mcu - my * geo.mcols;
  const int c = geo.bpm == 3 ? slot : (slot < 4 ? 0 : slot - 3);
  int by = my, bx = mx;
  if (geo.bpm == 6 && slot < 4) {
    by = 2 * my + (slot >> 1);
    bx = 2 * mx + (slot & 1);
  }
  const uint4* src = reinterpret_cast<const uint4*>(coef_all + (long long)(frame0 + blockIdx.y) * coef_stride + (long long)b * 64);
  const Planes pl = planes_of(geo);
  idct_block(src, q_s + 64 * c, planes_all + (long long)(frame0 + blockIdx.y) * plane_stride + pl.off[c] + ((long long)by * 8) * pl.pw[c] + bx * 8, pl.pw[c]);
}

// grid (ceil(H ceil(W / 4) / 256), frames of this launch), 256 threads: four pixels of a row each.
__global__ __launch_bounds__(256) void jpegdec_color_kernel(DecRecs recs, int frame0, int H, int W, const unsigned char* __restrict__ planes_all,
                                                            long long plane_stride, unsigned char* __restrict__ out) {
  const DecRec rec = recs.r[blockIdx.y];
  if (rec.pre_status) return;
  const int groups = (W + 3) >> 2;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)H * groups) return;
  const int y = (int)(t / groups), x0 = (int)(t - (long long)y * groups) * 4;
  const Geo geo = geometry(H, W, rec.sub, rec.ri);
  const Planes pl = planes_of(geo);
  const unsigned char* base = planes_all + (long long)(frame0 + blockIdx.y) * plane_stride;
  const unsigned yy = *reinterpret_cast<const unsigned*>(base + pl.off[0] + (long long)y * pl.pw[0] + x0);
  int cb[4], cr[4];
  if (geo.bpm == 3) {
    const unsigned b4 = *reinterpret_cast<const unsigned*>(base + pl.off[1] + (long long)y * pl.pw[1] + x0);
    const unsigned r4 = *reinterpret_cast<const unsigned*>(base + pl.off[2] + (long long)y * pl.pw[2] + x0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      cb[i] = (int)((b4 >> (8 * i)) & 0xFFu);
      cr[i] = (int)((r4 >> (8 * i)) & 0xFFu);
    }
  } else {                                                      // h2v2 fancy upsampling from the real ceil(H/2) x ceil(W/2) plane
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    const int near = y >> 1, far = clampi((y & 1) ? near + 1 : near - 1, 0, ch - 1);
    const int c0 = x0 >> 1;
#pragma unroll
    for (int comp = 1; comp < 3; ++comp) {
      const unsigned char* pn = base + pl.off[comp] + (long long)near * pl.pw[comp];
      const unsigned char* pf = base + pl.off[comp] + (long long)far * pl.pw[comp];
      int s[4];                                                 // 3 near + far at chroma columns c0 - 1 .. c0 + 2, the edge columns repeated
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cx = clampi(c0 - 1 + i, 0, cw - 1);
        s[i] = 3 * (int)pn[cx] + (int)pf[cx];
      }
      int* dst = comp == 1 ? cb : cr;
      dst[0] = (3 * s[1] + s[0] + 8) >> 4;
      dst[1] = (3 * s[1] + s[2] + 7) >> 4;
      dst[2] = (3 * s[2] + s[1] + 8) >> 4;
      dst[3] = (3 * s[2] + s[3] + 7) >> 4;
    }
  }
  store_bgr4(yy, cb, cr, out + ((long long)(frame0 + blockIdx.y) * H + y) * W * 3 + (long long)x0 * 3, x0, W);
}

// blocks and plane bytes of a frame, the larger of the samplings `subsampling` admits (0: either, 2: 4:2:0 only)
void frame_caps(int H, int W, int subsampling, long long* blocks, long long* plane_bytes) {
  const Geo g2 = geometry(H, W, 2, 0), g0 = geometry(H, W, 0, 0);
  long long b = 6ll * g2.n_mcu, p = 384ll * g2.n_mcu;
  if (subsampling == 0) {
    if (3ll * g0.n_mcu > b) b = 3ll * g0.n_mcu;
    if (192ll * g0.n_mcu > p) p = 192ll * g0.n_mcu;
  }
  *blocks = b;
  *plane_bytes = align_up(p);
}

int check_args(const char* who, int batch, int H, int W, int subsampling, long long total_sub) {
  CASYNC_REQUIRE(H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "%s: a frame of %d x %d (h x w) is outside 1..65535", who, H, W);
  CASYNC_REQUIRE(batch >= 0 && batch <= 32768, "%s: batch %d", who, batch);
  CASYNC_REQUIRE(subsampling == 0 || subsampling == 2, "%s: subsampling %d is neither 0 (any) nor 2 (4:2:0 only)", who, subsampling);
  CASYNC_REQUIRE(total_sub >= 0 && total_sub <= (1ll << 28), "%s: %lld subsequences", who, total_sub);
  return CASYNC_OK;
}

}  // namespace

extern "C" {

int64_t casync_op_jpegdec_workspace_bytes(int batch, int H, int W, int subsampling, int64_t total_subsequences) {
  if (int st = check_args("jpegdec_workspace_bytes", batch, H, W, subsampling, total_subsequences)) return st;
  long long blocks, plane_bytes;
  frame_caps(H, W, subsampling, &blocks, &plane_bytes);
  return align_up(total_subsequences * (long long)sizeof(SubState)) + (long long)batch * (blocks * 128 + plane_bytes);
}

int casync_op_jpegdec_decode(const uint8_t* data, int64_t data_bytes, const int32_t* rec, int batch, int H, int W, int subsampling, int chunk_bits,
                             uint8_t* scratch, int64_t scratch_bytes, uint8_t* out, int32_t* status, casync_stream stream) {
  if (int st = check_args("jpegdec_decode", batch, H, W, subsampling, 0)) return st;
  CASYNC_REQUIRE(chunk_bits >= 32 && chunk_bits % 32 == 0 && chunk_bits <= (1 << 30), "jpegdec_decode: chunk_bits %d is not a multiple of 32 in 32..2^30",
                 chunk_bits);
  if (batch == 0) return CASYNC_OK;
  CASYNC_REQUIRE(data && rec && scratch && out && status, "jpegdec_decode: null pointer");
  CASYNC_REQUIRE(((uintptr_t)data & 3) == 0 && ((uintptr_t)scratch & 15) == 0 && ((uintptr_t)status & 3) == 0,
                 "jpegdec_decode: data and status must be 4-byte aligned, scratch 16-byte aligned");
  CASYNC_REQUIRE(data_bytes >= 0 && data_bytes < (1ll << 31), "jpegdec_decode: data of %lld bytes", (long long)data_bytes);
  long long total_sub = 0;
  for (int f = 0; f < batch; ++f) {
    const int32_t* r = rec + (size_t)f * REC_WORDS;
    const int scan_off = r[0], scan_len = r[1], sub = r[2], ri = r[3], nseg = r[4], seg_off = r[5], tab_off = r[6], nsub = r[7], sub_base = r[8], pre = r[9];
    CASYNC_REQUIRE(pre >= 0 && pre <= 3, "jpegdec_decode: record %d: status %d", f, pre);
    CASYNC_REQUIRE(sub == 0 || (sub == 2), "jpegdec_decode: record %d: sampling %d", f, sub);
    // (a record with a status gets no work and no kernel reads its sampling word: plan_decode leaves it 0 for a file outside the subset)
    CASYNC_REQUIRE(subsampling == 0 || sub == 2 || pre, "jpegdec_decode: record %d is 4:4:4 in a call sized for 4:2:0", f);
    CASYNC_REQUIRE(sub_base == total_sub, "jpegdec_decode: record %d: its subsequences start at %d, not %lld", f, sub_base, total_sub);
    if (pre) {
      CASYNC_REQUIRE(nsub == 0, "jpegdec_decode: record %d: a frame with a status has no subsequences", f);
      continue;
    }
    const Geo g = geometry(H, W, sub, ri);
    CASYNC_REQUIRE(ri >= 0 && ri <= 65535, "jpegdec_decode: record %d: restart interval %d", f, ri);
    CASYNC_REQUIRE(scan_off >= 0 && scan_len >= 0 && scan_len < (1 << 27) && (long long)scan_off + scan_len <= data_bytes,
                   "jpegdec_decode: record %d: scan [%d, +%d) outside the data", f, scan_off, scan_len);
    CASYNC_REQUIRE(nseg == (g.n_mcu + g.ri - 1) / g.ri, "jpegdec_decode: record %d: %d segments, the geometry has %d", f, nseg, (g.n_mcu + g.ri - 1) / g.ri);
    CASYNC_REQUIRE(seg_off >= 0 && seg_off % 4 == 0 && (long long)seg_off + 4ll * (3ll * nseg + 1) <= data_bytes,
                   "jpegdec_decode: record %d: segment list outside the data", f);
    CASYNC_REQUIRE(tab_off >= 0 && tab_off % 4 == 0 && (long long)tab_off + TAB_BYTES <= data_bytes, "jpegdec_decode: record %d: tables outside the data", f);
    CASYNC_REQUIRE(nsub >= nseg && (long long)nsub <= (long long)scan_len * 8 / chunk_bits + nseg, "jpegdec_decode: record %d: %d subsequences", f, nsub);
    CASYNC_REQUIRE(nsub <= MAX_SUBSEQUENCES, "jpegdec_decode: record %d: %d subsequences, at most %d a frame (a longer chunk_bits, or the host)", f, nsub,
                   MAX_SUBSEQUENCES);
    total_sub += nsub;
  }
  long long blocks, plane_bytes;
  frame_caps(H, W, subsampling, &blocks, &plane_bytes);
  const long long subs_bytes = align_up(total_sub * (long long)sizeof(SubState)), coef_bytes = (long long)batch * blocks * 128;
  const long long need = subs_bytes + coef_bytes + (long long)batch * plane_bytes;
  CASYNC_REQUIRE(scratch_bytes >= need, "jpegdec_decode: scratch of %lld bytes, casync_op_jpegdec_workspace_bytes says %lld", (long long)scratch_bytes, need);
  SubState* subs = reinterpret_cast<SubState*>(scratch);
  short* coef = reinterpret_cast<short*>(scratch + subs_bytes);
  unsigned char* planes = scratch + subs_bytes + coef_bytes;
  hipStream_t s = (hipStream_t)stream;
  CASYNC_CHECK_HIP(hipMemsetAsync(coef, 0, (size_t)coef_bytes, s));
  const long long groups = (long long)H * ((W + 3) / 4);
  for (int f0 = 0; f0 < batch; f0 += FRAMES_PER_LAUNCH) {
    const int n = batch - f0 < FRAMES_PER_LAUNCH ? batch - f0 : FRAMES_PER_LAUNCH;
    DecRecs recs = {};
    int launch_sub = 0, launch_blocks = 0;
    bool any = false;
    for (int i = 0; i < n; ++i) {
      const int32_t* r = rec + (size_t)(f0 + i) * REC_WORDS;
      recs.r[i] = DecRec{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], 0, 0};
      if (r[9]) continue;
      any = true;
      const Geo g = geometry(H, W, r[2], r[3]);
      if (r[7] > launch_sub) launch_sub = r[7];
      if (g.n_mcu * g.bpm > launch_blocks) launch_blocks = g.n_mcu * g.bpm;
    }
    if (int st = casync_launch(jpegdec_sync_kernel, dim3(n), dim3(SYNC_THREADS), 0, s, (const unsigned char*)data, recs, f0, H, W, chunk_bits, subs,
                               (int*)status))
      return st;
    if (!any) continue;
    if (int st = casync_launch(jpegdec_write_kernel, dim3((launch_sub + 255) / 256, n), dim3(256), 0, s, (const unsigned char*)data, recs, f0, H, W,
                               chunk_bits, (const SubState*)subs, coef, blocks * 64))
      return st;
    if (int st = casync_launch(jpegdec_idct_kernel, dim3((launch_blocks + 63) / 64, n), dim3(64), 0, s, (const unsigned char*)data, recs, f0, H, W,
                               (const short*)coef, blocks * 64, planes, plane_bytes))
      return st;
    if (int st = casync_launch(jpegdec_color_kernel, dim3((unsigned)((groups + 255) / 256), n), dim3(256), 0, s, recs, f0, H, W,
                               (const unsigned char*)planes, plane_bytes, (unsigned char*)out))
      return st;
  }
  return CASYNC_OK;
}

}  // extern "C"
