// Motion-JPEG frames -> uint8 BGR frames [B,H,W,3] on the device: the wider sibling of csrc/jpeg_dec.hip,
// byte for byte what libjpeg's default integer path decodes.  Beside 4:4:4 and 4:2:0 it reads what capture cards, webcams and
// `ffmpeg -c:v mjpeg` write: 2x1 / 1x1 / 1x1 sampling (4:2:2) and one-component files (grayscale), and one batch may mix the four.
// A file without its Huffman tables (the MJPG convention) needs nothing here: the host puts the Annex K tables into the file's
// table block (calipsync_amd/jpeg.py parse_jpeg, subset="mjpeg").  calipsync_amd/jpeg.py decode_jpeg_host(subset="mjpeg") is the
// numpy twin.
//
// The four stages are those of jpeg_dec.hip and their bodies are csrc/jpeg_dec_common.h; what is new is the geometry of an MCU and
// the component of each of its block slots, taken from the record's sampling word:
//
//   word  sampling  MCU (w x h)  slots            Y blocks of an MCU         chroma planes
//   0     4:4:4     8 x 8        Y Cb Cr          1                          full size
//   1     4:2:2     16 x 8       Y Y Cb Cr        2, side by side            ceil(W/2) columns: h2v1 fancy upsampling
//   2     4:2:0     16 x 16      Y Y Y Y Cb Cr    2 x 2                      ceil(H/2) x ceil(W/2): h2v2 fancy upsampling
//   3     gray      8 x 8        Y                1 (a scan of single blocks) none: Y is written to B, G and R
//
//   mjpegdec_sync_kernel    the entropy plan, one workgroup per frame (sync_body)
//   mjpegdec_write_kernel   the coefficient write, one lane per subsequence (write_body)
//   mjpegdec_idct_kernel    one lane per block: its place in its component's sample plane from the table above, then idct_block
//   mjpegdec_color_kernel   one lane per four pixels of a row: h2v1 is libjpeg's triangle filter along the row only, on the real
//                           ceil(W/2) columns, out[2i] = (3 c[i] + c[i-1] + 1) >> 2 and out[2i+1] = (3 c[i] + c[i+1] + 2) >> 2, the
//                           first and the last column copied (which is what a repeated edge column gives under this rounding);
//                           h2v2 as in jpeg_dec.hip; gray takes Cb = Cr = 128, under which the colour arithmetic returns Y.
//
// Bounds: the rules at the top of jpeg_dec.hip, unchanged.  No stream content forms an address or bounds a loop; reads past a
// segment's end return zeros; every table value is clamped or masked before use; the sampling word comes from the host's record,
// is checked to be 0..3 before anything is launched and masked where it is used; no global atomics.
#include "jpeg_dec_common.h"

namespace {

constexpr int SAMPLINGS = 4;
constexpr int GRAY = 3;

struct Mjpeg {
  // Y blocks of an MCU across and down
  __host__ __device__ static inline int hs(int sub) { return sub == 1 || sub == 2 ? 2 : 1; }
  __host__ __device__ static inline int vs(int sub) { return sub == 2 ? 2 : 1; }
  __host__ __device__ static inline Geo geometry(int H, int W, int sub, int ri) {
    Geo g;
    sub &= 3;
    const int mw = 8 * hs(sub), mh = 8 * vs(sub);
    g.bpm = sub == GRAY ? 1 : hs(sub) * vs(sub) + 2;
    g.mrows = (H + mh - 1) / mh;
    g.mcols = (W + mw - 1) / mw;
    g.n_mcu = g.mrows * g.mcols;
    g.ri = ri > 0 && ri < g.n_mcu ? ri : g.n_mcu;
    return g;
  }
  // the component of slot s of an MCU of bpm blocks: the Y blocks first, then Cb and Cr
  __device__ static __forceinline__ int comp(int bpm, int s) {
    const int ny = bpm > 2 ? bpm - 2 : 1;
    return s < ny ? 0 : clampi(s - ny + 1, 1, 2);
  }
};

// The sample planes of a frame: Y of (8 vs mrows) x (8 hs mcols), then (but for gray) Cb and Cr of (8 mrows) x (8 mcols) each
struct Planes { long long off[3]; int pw[3]; };
__device__ __forceinline__ Planes planes_of(const Geo& g, int sub) {
  Planes p;
  const int h = Mjpeg::hs(sub), v = Mjpeg::vs(sub);
  p.off[0] = 0;
  p.off[1] = 64ll * h * v * g.n_mcu;
  p.off[2] = p.off[1] + 64ll * g.n_mcu;
  p.pw[0] = 8 * h * g.mcols;
  p.pw[1] = p.pw[2] = 8 * g.mcols;
  return p;
}

// grid (frames of this launch), SYNC_THREADS.  subs: every frame's subsequences, frame f's from rec.sub_base on.
__global__ __launch_bounds__(SYNC_THREADS) void mjpegdec_sync_kernel(const unsigned char* __restrict__ data, DecRecs recs, int frame0, int H, int W,
                                                                     int chunk_bits, SubState* subs_all, int* __restrict__ status) {
  sync_body<Mjpeg>(data, recs, frame0, H, W, chunk_bits, subs_all, status);
}

// grid (ceil(subsequences of the largest frame / 256), frames of this launch), 256 threads.  coef: [frame][blocks][64] int16, zeroed.
__global__ __launch_bounds__(256) void mjpegdec_write_kernel(const unsigned char* __restrict__ data, DecRecs recs, int frame0, int H, int W, int chunk_bits,
                                                             const SubState* __restrict__ subs_all, short* __restrict__ coef_all, long long coef_stride) {
  write_body<Mjpeg>(data, recs, frame0, H, W, chunk_bits, subs_all, coef_all, coef_stride);
}

// grid (ceil(blocks of the largest frame / 64), frames of this launch), 64 threads.
__global__ __launch_bounds__(64) void mjpegdec_idct_kernel(const unsigned char* __restrict__ data, DecRecs recs, int frame0, int H, int W,
                                                           const short* __restrict__ coef_all, long long coef_stride, unsigned char* __restrict__ planes_all,
                                                           long long plane_stride) {
  __shared__ unsigned short q_s[192];
  const DecRec rec = recs.r[blockIdx.y];
  if (rec.pre_status) return;
  const int sub = rec.sub & 3;
  const Geo geo = Mjpeg::geometry(H, W, sub, rec.ri);
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
  const int c = Mjpeg::comp(geo.bpm, slot);
  int by = my, bx = mx;
  if (c == 0) {                                                  // Y block `slot` of its MCU: hs across, vs down
    const int h = Mjpeg::hs(sub);
    by = Mjpeg::vs(sub) * my + (h == 2 ? slot >> 1 : 0);
    bx = h * mx + (h == 2 ? slot & 1 : 0);
  }
  const uint4* src = reinterpret_cast<const uint4*>(coef_all + (long long)(frame0 + blockIdx.y) * coef_stride + (long long)b * 64);
  const Planes pl = planes_of(geo, sub);
  idct_block(src, q_s + 64 * c, planes_all + (long long)(frame0 + blockIdx.y) * plane_stride + pl.off[c] + ((long long)by * 8) * pl.pw[c] + bx * 8, pl.pw[c]);
}

// grid (ceil(H ceil(W / 4) / 256), frames of this launch), 256 threads: four pixels of a row each.
__global__ __launch_bounds__(256) void mjpegdec_color_kernel(DecRecs recs, int frame0, int H, int W, const unsigned char* __restrict__ planes_all,
                                                             long long plane_stride, unsigned char* __restrict__ out) {
  const DecRec rec = recs.r[blockIdx.y];
  if (rec.pre_status) return;
  const int groups = (W + 3) >> 2;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)H * groups) return;
  const int y = (int)(t / groups), x0 = (int)(t - (long long)y * groups) * 4;
  const int sub = rec.sub & 3;                                   // uniform over the workgroups of a frame
  const Geo geo = Mjpeg::geometry(H, W, sub, rec.ri);
  const Planes pl = planes_of(geo, sub);
  const unsigned char* base = planes_all + (long long)(frame0 + blockIdx.y) * plane_stride;
  const unsigned yy = *reinterpret_cast<const unsigned*>(base + pl.off[0] + (long long)y * pl.pw[0] + x0);
  int cb[4], cr[4];
  if (sub == GRAY) {
#pragma unroll
    for (int i = 0; i < 4; ++i) cb[i] = cr[i] = 128;
  } else if (sub == 0) {
    const unsigned b4 = *reinterpret_cast<const unsigned*>(base + pl.off[1] + (long long)y * pl.pw[1] + x0);
    const unsigned r4 = *reinterpret_cast<const unsigned*>(base + pl.off[2] + (long long)y * pl.pw[2] + x0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      cb[i] = (int)((b4 >> (8 * i)) & 0xFFu);
      cr[i] = (int)((r4 >> (8 * i)) & 0xFFu);
    }
  } else {
    const int cw = (W + 1) >> 1, c0 = x0 >> 1;
    const bool v2 = sub == 2;                                   // h2v2: 3 near + far of the real ceil(H/2) rows; h2v1: the row itself
    const int ch = (H + 1) >> 1;
    const int near = v2 ? y >> 1 : y, far = v2 ? clampi((y & 1) ? near + 1 : near - 1, 0, ch - 1) : near;
#pragma unroll
    for (int comp = 1; comp < 3; ++comp) {
      const unsigned char* pn = base + pl.off[comp] + (long long)near * pl.pw[comp];
      const unsigned char* pf = base + pl.off[comp] + (long long)far * pl.pw[comp];
      int s[4];                                                 // chroma columns c0 - 1 .. c0 + 2, the edge columns repeated
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cx = clampi(c0 - 1 + i, 0, cw - 1);
        s[i] = v2 ? 3 * (int)pn[cx] + (int)pf[cx] : (int)pn[cx];
      }
      int* dst = comp == 1 ? cb : cr;
      if (v2) {
        dst[0] = (3 * s[1] + s[0] + 8) >> 4;
        dst[1] = (3 * s[1] + s[2] + 7) >> 4;
        dst[2] = (3 * s[2] + s[1] + 8) >> 4;
        dst[3] = (3 * s[2] + s[3] + 7) >> 4;
      } else {
        dst[0] = (3 * s[1] + s[0] + 1) >> 2;
        dst[1] = (3 * s[1] + s[2] + 2) >> 2;
        dst[2] = (3 * s[2] + s[1] + 1) >> 2;
        dst[3] = (3 * s[2] + s[3] + 2) >> 2;
      }
    }
  }
  store_bgr4(yy, cb, cr, out + ((long long)(frame0 + blockIdx.y) * H + y) * W * 3 + (long long)x0 * 3, x0, W);
}

// blocks and plane bytes of a frame: the largest over the four samplings, so that one scratch serves a mixed batch
void frame_caps(int H, int W, long long* blocks, long long* plane_bytes) {
  long long b = 0, p = 0;
  for (int sub = 0; sub < SAMPLINGS; ++sub) {
    const Geo g = Mjpeg::geometry(H, W, sub, 0);
    const long long nb = (long long)g.n_mcu * g.bpm;
    b = nb > b ? nb : b;
    p = 64 * nb > p ? 64 * nb : p;
  }
  *blocks = b;
  *plane_bytes = align_up(p);
}

int check_args(const char* who, int batch, int H, int W, long long total_sub) {
  CASYNC_REQUIRE(H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "%s: a frame of %d x %d (h x w) is outside 1..65535", who, H, W);
  CASYNC_REQUIRE(batch >= 0 && batch <= 32768, "%s: batch %d", who, batch);
  CASYNC_REQUIRE(total_sub >= 0 && total_sub <= (1ll << 28), "%s: %lld subsequences", who, total_sub);
  return CASYNC_OK;
}

}  // namespace

extern "C" {

int64_t casync_op_mjpegdec_workspace_bytes(int batch, int H, int W, int64_t total_subsequences) {
  if (int st = check_args("mjpegdec_workspace_bytes", batch, H, W, total_subsequences)) return st;
  long long blocks, plane_bytes;
  frame_caps(H, W, &blocks, &plane_bytes);
  return align_up(total_subsequences * (long long)sizeof(SubState)) + (long long)batch * (blocks * 128 + plane_bytes);
}

int casync_op_mjpegdec_decode(const uint8_t* data, int64_t data_bytes, const int32_t* rec, int batch, int H, int W, int chunk_bits, uint8_t* scratch,
                              int64_t scratch_bytes, uint8_t* out, int32_t* status, casync_stream stream) {
  if (int st = check_args("mjpegdec_decode", batch, H, W, 0)) return st;
  CASYNC_REQUIRE(chunk_bits >= 32 && chunk_bits % 32 == 0 && chunk_bits <= (1 << 30), "mjpegdec_decode: chunk_bits %d is not a multiple of 32 in 32..2^30",
                 chunk_bits);
  if (batch == 0) return CASYNC_OK;
  CASYNC_REQUIRE(data && rec && scratch && out && status, "mjpegdec_decode: null pointer");
  CASYNC_REQUIRE(((uintptr_t)data & 3) == 0 && ((uintptr_t)scratch & 15) == 0 && ((uintptr_t)status & 3) == 0,
                 "mjpegdec_decode: data and status must be 4-byte aligned, scratch 16-byte aligned");
  CASYNC_REQUIRE(data_bytes >= 0 && data_bytes < (1ll << 31), "mjpegdec_decode: data of %lld bytes", (long long)data_bytes);
  long long total_sub = 0;
  for (int f = 0; f < batch; ++f) {
    const int32_t* r = rec + (size_t)f * REC_WORDS;
    const int scan_off = r[0], scan_len = r[1], sub = r[2], ri = r[3], nseg = r[4], seg_off = r[5], tab_off = r[6], nsub = r[7], sub_base = r[8], pre = r[9];
    CASYNC_REQUIRE(pre >= 0 && pre <= 3, "mjpegdec_decode: record %d: status %d", f, pre);
    CASYNC_REQUIRE(sub >= 0 && sub < SAMPLINGS, "mjpegdec_decode: record %d: sampling %d is none of 0 (4:4:4), 1 (4:2:2), 2 (4:2:0), 3 (gray)", f, sub);
    CASYNC_REQUIRE(sub_base == total_sub, "mjpegdec_decode: record %d: its subsequences start at %d, not %lld", f, sub_base, total_sub);
    if (pre) {
      CASYNC_REQUIRE(nsub == 0, "mjpegdec_decode: record %d: a frame with a status has no subsequences", f);
      continue;
    }
    const Geo g = Mjpeg::geometry(H, W, sub, ri);
    CASYNC_REQUIRE(ri >= 0 && ri <= 65535, "mjpegdec_decode: record %d: restart interval %d", f, ri);
    CASYNC_REQUIRE(scan_off >= 0 && scan_len >= 0 && scan_len < (1 << 27) && (long long)scan_off + scan_len <= data_bytes,
                   "mjpegdec_decode: record %d: scan [%d, +%d) outside the data", f, scan_off, scan_len);
    CASYNC_REQUIRE(nseg == (g.n_mcu + g.ri - 1) / g.ri, "mjpegdec_decode: record %d: %d segments, the geometry has %d", f, nseg, (g.n_mcu + g.ri - 1) / g.ri);
    CASYNC_REQUIRE(seg_off >= 0 && seg_off % 4 == 0 && (long long)seg_off + 4ll * (3ll * nseg + 1) <= data_bytes,
                   "mjpegdec_decode: record %d: segment list outside the data", f);
    CASYNC_REQUIRE(tab_off >= 0 && tab_off % 4 == 0 && (long long)tab_off + TAB_BYTES <= data_bytes, "mjpegdec_decode: record %d: tables outside the data", f);
    CASYNC_REQUIRE(nsub >= nseg && (long long)nsub <= (long long)scan_len * 8 / chunk_bits + nseg, "mjpegdec_decode: record %d: %d subsequences", f, nsub);
    CASYNC_REQUIRE(nsub <= MAX_SUBSEQUENCES, "mjpegdec_decode: record %d: %d subsequences, at most %d a frame (a longer chunk_bits, or the host)", f, nsub,
                   MAX_SUBSEQUENCES);
    total_sub += nsub;
  }
  long long blocks, plane_bytes;
  frame_caps(H, W, &blocks, &plane_bytes);
  const long long subs_bytes = align_up(total_sub * (long long)sizeof(SubState)), coef_bytes = (long long)batch * blocks * 128;
  const long long need = subs_bytes + coef_bytes + (long long)batch * plane_bytes;
  CASYNC_REQUIRE(scratch_bytes >= need, "mjpegdec_decode: scratch of %lld bytes, casync_op_mjpegdec_workspace_bytes says %lld", (long long)scratch_bytes, need);
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
      const Geo g = Mjpeg::geometry(H, W, r[2], r[3]);
      if (r[7] > launch_sub) launch_sub = r[7];
      if (g.n_mcu * g.bpm > launch_blocks) launch_blocks = g.n_mcu * g.bpm;
    }
    if (int st = casync_launch(mjpegdec_sync_kernel, dim3(n), dim3(SYNC_THREADS), 0, s, (const unsigned char*)data, recs, f0, H, W, chunk_bits, subs,
                               (int*)status))
      return st;
    if (!any) continue;
    if (int st = casync_launch(mjpegdec_write_kernel, dim3((launch_sub + 255) / 256, n), dim3(256), 0, s, (const unsigned char*)data, recs, f0, H, W,
                               chunk_bits, (const SubState*)subs, coef, blocks * 64))
      return st;
    if (int st = casync_launch(mjpegdec_idct_kernel, dim3((launch_blocks + 63) / 64, n), dim3(64), 0, s, (const unsigned char*)data, recs, f0, H, W,
                               (const short*)coef, blocks * 64, planes, plane_bytes))
      return st;
    if (int st = casync_launch(mjpegdec_color_kernel, dim3((unsigned)((groups + 255) / 256), n), dim3(256), 0, s, recs, f0, H, W,
                               (const unsigned char*)planes, plane_bytes, (unsigned char*)out))
      return st;
  }
  return CASYNC_OK;
}

}  // extern "C"
