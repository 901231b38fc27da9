// Baseline JPEG files -> uint8 BGR frames [B,H,W,3] on the device, byte for byte what libjpeg's default integer path decodes
// (islow inverse DCT, fancy chroma upsampling, 16-bit fixed-point colour; calipsync_amd/jpeg.py decode_jpeg_host is the numpy
// twin).  The encoders are csrc/jpeg_enc.hip and csrc/jpeg_enc420.hip; this file shares no code with them.
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
#include "common.h"

namespace {

constexpr int FRAMES_PER_LAUNCH = 64;
constexpr int REC_WORDS = 16;                      // the host's record
constexpr int TAB_BYTES = 384 + 8 + 4 * 832;       // quantisation [3][64] u16 (natural order) | dc table of each component, 0 | ac table, 0 | 4 Huffman tables
constexpr int HUFF0 = 392, HUFF_BYTES = 832;       // a Huffman table: lut [256] u16 (length << 8 | symbol of a code of up to 8 bits) | maxcode [8] (lengths
                                                   // 9..16, -1: none) | valoff [8] (index of the length's first symbol - its first code) | symbols [256]
constexpr int SYNC_THREADS = 512;
constexpr int MAX_SUBSEQUENCES = 1 << 17;         // per frame: the rounds of the plan are bounded by the subsequences, a round sweeps them all
constexpr long long ALIGN = 256;

struct DecRec { int scan_off, scan_len, sub, ri, nseg, seg_off, tab_off, nsub, sub_base, pre_status, pad0, pad1; };
struct DecRecs { DecRec r[FRAMES_PER_LAUNCH]; };

struct alignas(16) SubState {                      // one subsequence
  unsigned ent_p, ent_sz;                          // entry state: bit position in the scan; slot | zigzag << 8
  unsigned x_p, x_sz;                              // exit state of the latest decode
  int n, errn;                                     // blocks finished; blocks finished ahead of an invalid code, or -1
  int dc[3];                                       // sum of the DC differences per component
  int first;                                       // blocks of its segment finished ahead of it
  int pred[3];                                     // DC predictors at its entry
  int seg;                                         // its segment; bit 30: it is the segment's first, bit 29: its last
  int changed, dead;                               // the entry state changed in this round; an invalid code lies ahead of it in the segment
};
constexpr int SEG_FIRST = 1 << 30, SEG_LAST = 1 << 29, SEG_MASK = SEG_LAST - 1;

__device__ const unsigned char ZZ_NAT_DEV[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
};

struct Geo { int bpm, mrows, mcols, n_mcu, ri; };
__host__ __device__ inline Geo geometry(int H, int W, int sub, int ri) {
  Geo g;
  const int s = sub ? 16 : 8;
  g.bpm = sub ? 6 : 3;
  g.mrows = (H + s - 1) / s;
  g.mcols = (W + s - 1) / s;
  g.n_mcu = g.mrows * g.mcols;
  g.ri = ri > 0 && ri < g.n_mcu ? ri : g.n_mcu;
  return g;
}
// blocks the geometry gives segment j, and (first) the stream index of its first block
__device__ __forceinline__ int seg_blocks(const Geo& g, int j, long long* base) {
  const long long mcu0 = (long long)j * g.ri;
  if (mcu0 >= g.n_mcu) {
    *base = 0;
    return 0;
  }
  *base = mcu0 * g.bpm;
  const long long left = g.n_mcu - mcu0;
  return (int)(left < g.ri ? left : g.ri) * g.bpm;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// One segment's bytes: scan[s0 .. s1).  Byte k is stuffing iff it is 0x00 behind 0xFF inside the segment; a position never lies
// in one.  Bytes from s1 on read as zero.
struct Stream {
  const unsigned char* scan;
  unsigned s0, s1;
  __device__ __forceinline__ unsigned byte(unsigned k) const { return k < s1 ? scan[k] : 0u; }
  __device__ __forceinline__ bool stuffed(unsigned k) const { return k > s0 && k < s1 && scan[k] == 0u && scan[k - 1] == 0xFFu; }
  __device__ __forceinline__ unsigned norm(unsigned p) const { return stuffed(p >> 3) ? ((p >> 3) + 1u) << 3 : p; }
  // the 32 data bits from position p on; skips: bit n set where a stuffed byte lies right ahead of the n-th data byte
  __device__ __forceinline__ unsigned window(unsigned p, unsigned* skips) const {
    unsigned k = p >> 3, i = k, m = 0;
    unsigned prev = (k > s0 && k - 1u < s1) ? scan[k - 1u] : 0u;
    unsigned long long acc = 0;
    int n = 0;
    for (int it = 0; it < 10 && n < 5; ++it) {                  // no two stuffed bytes in a row: five data bytes within ten
      const unsigned b = byte(i);
      if (b == 0u && prev == 0xFFu && i > s0 && i < s1) {
        m |= 1u << n;
        prev = 0u;
      } else {
        acc = (acc << 8) | b;
        prev = b;
        ++n;
      }
      ++i;
    }
    *skips = m;
    return (unsigned)(acc >> (8u - (p & 7u)));
  }
  __device__ __forceinline__ unsigned advance(unsigned p, unsigned bits, unsigned skips) const {      // bits <= 31
    const unsigned t = (p & 7u) + bits, nb = t >> 3;
    return (((p >> 3) + nb + (unsigned)__popc(skips & ((2u << nb) - 1u))) << 3) | (t & 7u);
  }
};

// the Huffman code at the top of w in the table at tab (LDS) -> its length (0: none) and symbol
__device__ __forceinline__ unsigned huff_decode(const unsigned char* tab, unsigned w, unsigned* sym) {
  const unsigned e = reinterpret_cast<const unsigned short*>(tab)[w >> 24];
  if (e) {
    *sym = e & 0xFFu;
    const unsigned len = e >> 8;
    return len <= 8u ? len : 0u;
  }
  const int* maxcode = reinterpret_cast<const int*>(tab + 512);
  const int* valoff = reinterpret_cast<const int*>(tab + 544);
  for (int l = 9; l <= 16; ++l) {
    const int code = (int)(w >> (32 - l));
    if (code <= maxcode[l - 9]) {
      *sym = tab[576 + ((code + valoff[l - 9]) & 255)];
      return (unsigned)l;
    }
  }
  return 0u;
}

struct SubResult { unsigned p, sz; int n, errn, dc[3]; };

// The symbols that start at positions p <= .. < end, from state (p, slot, zigzag).  WRITE: the coefficients of blocks
// first + 0 .. below cap go to coef[(base + block) * 64 + natural index], DC as values from pred.
template <bool WRITE>
__device__ __forceinline__ SubResult run_sub(const Stream& st, const unsigned char* tab, int bpm, unsigned p, unsigned sz, unsigned end, int first,
                                             int cap, int* pred, short* coef) {
  SubResult r;
  r.n = 0;
  r.errn = -1;
  r.dc[0] = r.dc[1] = r.dc[2] = 0;
  int s = (int)(sz & 0xFFu) % bpm, z = (int)((sz >> 8) & 63u);
  const unsigned budget = end > p ? end - p : 0u;               // every symbol takes a bit or more
  for (unsigned it = 0; it < budget && p < end; ++it) {
    unsigned skips, sym;
    const unsigned w = st.window(p, &skips);
    const int c = bpm == 3 ? s : (s < 4 ? 0 : s - 3);
    const bool dc = z == 0;
    const unsigned sel = tab[384 + (dc ? 0 : 4) + c] & 1u;
    const unsigned len = huff_decode(tab + HUFF0 + ((dc ? 0u : 2u) + sel) * HUFF_BYTES, w, &sym);
    bool bad = len == 0u, done = false;
    unsigned cat = 0;
    if (!bad) {
      if (dc) {
        cat = sym;
        bad = cat > 11u;
      } else {
        cat = sym & 15u;
        const int run = (int)(sym >> 4);
        if (cat == 0u) {
          if (run == 15) {
            z += 16;
            bad = z > 64;
            done = z == 64;
          } else {
            done = true;
          }
        } else {
          z += run;
          bad = z > 63;
        }
      }
    }
    if (bad) {
      r.errn = r.n;
      r.p = st.norm(end);
      r.sz = 0;
      return r;
    }
    int v = 0;
    if (cat) {
      const unsigned bits = (w << len) >> (32u - cat);
      v = bits < (1u << (cat - 1u)) ? (int)bits - (int)((1u << cat) - 1u) : (int)bits;
    }
    if (dc) {
      r.dc[c] += v;
      if (WRITE) {
        pred[c] += v;
        if (first + r.n < cap) coef[((long long)first + r.n) * 64] = (short)pred[c];
      }
      z = 1;
    } else if (cat) {
      if (WRITE && first + r.n < cap) coef[((long long)first + r.n) * 64 + ZZ_NAT_DEV[z & 63]] = (short)v;
      ++z;
      done = z == 64;
    }
    p = st.advance(p, len + cat, skips);
    if (done) {
      z = 0;
      s = s + 1 == bpm ? 0 : s + 1;
      ++r.n;
    }
  }
  r.p = p;
  r.sz = (unsigned)s | ((unsigned)z << 8);
  return r;
}

// The segment list of a frame: start [nseg] | end [nseg] | first subsequence [nseg + 1], byte offsets relative to the scan
struct SegList {
  const int* w;
  int nseg, scan_len;
  __device__ __forceinline__ int find(int g) const {            // the last segment whose first subsequence is <= g
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (w[2 * nseg + mid] <= g) lo = mid;
      else hi = mid - 1;
    }
    return lo;
  }
  __device__ __forceinline__ unsigned start(int j) const { return (unsigned)clampi(w[j], 0, scan_len); }
  __device__ __forceinline__ unsigned end(int j) const { return (unsigned)clampi(w[nseg + j], (int)start(j), scan_len); }
};

// The stream and the bit range [b0, b1) of subsequence g, which lies in segment j
__device__ __forceinline__ Stream sub_range(const unsigned char* scan, const SegList& sl, int j, int g, int chunk_bits, unsigned* b0, unsigned* b1,
                                            bool* is_first, bool* is_last) {
  Stream st;
  st.scan = scan;
  st.s0 = sl.start(j);
  st.s1 = sl.end(j);
  int k = g - sl.w[2 * sl.nseg + j];
  k = k < 0 ? 0 : k;
  *is_first = k == 0;
  *is_last = g + 1 >= sl.w[2 * sl.nseg + j + 1];
  const unsigned long long lo = (unsigned long long)st.s0 * 8u + (unsigned long long)k * (unsigned)chunk_bits, hi = (unsigned long long)st.s1 * 8u;
  *b0 = (unsigned)(lo < hi ? lo : hi);
  const unsigned long long nx = lo + (unsigned)chunk_bits;
  *b1 = (unsigned)(*is_last || nx > hi ? hi : nx);
  return st;
}

__device__ __forceinline__ void load_tables(const unsigned char* data, const DecRec& rec, unsigned* tab_s, int tid, int threads) {
  const unsigned* src = reinterpret_cast<const unsigned*>(data + rec.tab_off);
  for (int i = tid; i < TAB_BYTES / 4; i += threads) tab_s[i] = src[i];
}

// grid (frames of this launch), SYNC_THREADS.  subs: every frame's subsequences, frame f's from rec.sub_base on.
__global__ __launch_bounds__(SYNC_THREADS) void jpegdec_sync_kernel(const unsigned char* __restrict__ data, DecRecs recs, int frame0, int H, int W,
                                                                    int chunk_bits, SubState* subs_all, int* __restrict__ status) {
  __shared__ unsigned tab_s[TAB_BYTES / 4];
  __shared__ int any_s, key_s;
  __shared__ int tot_n[SYNC_THREADS], tot_dc[3][SYNC_THREADS], tot_flags[SYNC_THREADS];       // flags: 1 dead, 2 the range held a segment's first
  __shared__ int in_n[SYNC_THREADS], in_dc[3][SYNC_THREADS], in_dead[SYNC_THREADS];
  const int tid = threadIdx.x;
  const DecRec rec = recs.r[blockIdx.x];
  if (rec.pre_status) {                                          // uniform: the host found the segment count wrong
    if (tid == 0) status[frame0 + blockIdx.x] = rec.pre_status;
    return;
  }
  const Geo geo = geometry(H, W, rec.sub, rec.ri);
  const unsigned char* scan = data + rec.scan_off;
  const unsigned char* tab = reinterpret_cast<const unsigned char*>(tab_s);
  SegList sl;
  sl.w = reinterpret_cast<const int*>(data + rec.seg_off);
  sl.nseg = rec.nseg;
  sl.scan_len = rec.scan_len;
  SubState* subs = subs_all + rec.sub_base;
  const int nsub = rec.nsub;
  load_tables(data, rec, tab_s, tid, SYNC_THREADS);
  for (int g = tid; g < nsub; g += SYNC_THREADS) {
    const int j = sl.find(g);
    unsigned b0, b1;
    bool is_first, is_last;
    const Stream st = sub_range(scan, sl, j, g, chunk_bits, &b0, &b1, &is_first, &is_last);
    SubState s = {};
    s.ent_p = is_first ? b0 : st.norm(b0);
    s.seg = j | (is_first ? SEG_FIRST : 0) | (is_last ? SEG_LAST : 0);
    s.changed = 1;
    s.errn = -1;
    subs[g] = s;
  }
  __syncthreads();
  for (int round = 0; round <= nsub; ++round) {                 // subsequence k is right after k rounds
    if (tid == 0) any_s = 0;
    for (int g = tid; g < nsub; g += SYNC_THREADS) {
      if (!subs[g].changed) continue;
      const int j = subs[g].seg & SEG_MASK;
      unsigned b0, b1;
      bool is_first, is_last;
      const Stream st = sub_range(scan, sl, j, g, chunk_bits, &b0, &b1, &is_first, &is_last);
      const SubResult r = run_sub<false>(st, tab, geo.bpm, subs[g].ent_p, subs[g].ent_sz, b1, 0, 0, nullptr, nullptr);
      subs[g].x_p = r.p;
      subs[g].x_sz = r.sz;
      subs[g].n = r.n;
      subs[g].errn = r.errn;
      subs[g].dc[0] = r.dc[0];
      subs[g].dc[1] = r.dc[1];
      subs[g].dc[2] = r.dc[2];
    }
    __syncthreads();
    bool mine = false;
    for (int g = tid; g < nsub; g += SYNC_THREADS) {
      int changed = 0;
      if (!(subs[g].seg & SEG_FIRST) && g > 0) {
        const unsigned xp = subs[g - 1].x_p, xsz = subs[g - 1].x_sz;
        if (xp != subs[g].ent_p || xsz != subs[g].ent_sz) {
          subs[g].ent_p = xp;
          subs[g].ent_sz = xsz;
          changed = 1;
        }
      }
      subs[g].changed = changed;
      mine |= changed != 0;
    }
    if (mine) any_s = 1;
    __syncthreads();
    const bool more = any_s != 0;
    __syncthreads();
    if (!more) break;
  }
  // segmented prefix sum over the subsequences: thread t takes a contiguous range, thread 0 joins the ranges' totals
  const int per = (nsub + SYNC_THREADS - 1) / SYNC_THREADS;
  const int g0 = tid * per < nsub ? tid * per : nsub, g1 = g0 + per < nsub ? g0 + per : nsub;
  {
    int n = 0, dc0 = 0, dc1 = 0, dc2 = 0, flags = 0;
    for (int g = g0; g < g1; ++g) {
      if (subs[g].seg & SEG_FIRST) {
        n = dc0 = dc1 = dc2 = 0;
        flags = 2;
      }
      subs[g].first = n;
      subs[g].pred[0] = dc0;
      subs[g].pred[1] = dc1;
      subs[g].pred[2] = dc2;
      subs[g].dead = flags & 1;
      if (!(flags & 1)) {
        if (subs[g].errn >= 0) {
          n += subs[g].errn;
          flags |= 1;
        } else {
          n += subs[g].n;
          dc0 += subs[g].dc[0];
          dc1 += subs[g].dc[1];
          dc2 += subs[g].dc[2];
        }
      }
    }
    tot_n[tid] = n;
    tot_dc[0][tid] = dc0;
    tot_dc[1][tid] = dc1;
    tot_dc[2][tid] = dc2;
    tot_flags[tid] = flags;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0, dc0 = 0, dc1 = 0, dc2 = 0, dead = 0;
    for (int t = 0; t < SYNC_THREADS; ++t) {
      in_n[t] = n;
      in_dc[0][t] = dc0;
      in_dc[1][t] = dc1;
      in_dc[2][t] = dc2;
      in_dead[t] = dead;
      if (tot_flags[t] & 2) {
        n = tot_n[t];
        dc0 = tot_dc[0][t];
        dc1 = tot_dc[1][t];
        dc2 = tot_dc[2][t];
        dead = tot_flags[t] & 1;
      } else if (!dead) {
        n += tot_n[t];
        dc0 += tot_dc[0][t];
        dc1 += tot_dc[1][t];
        dc2 += tot_dc[2][t];
        dead = tot_flags[t] & 1;
      }
    }
    key_s = 0x7FFFFFFF;
  }
  __syncthreads();
  for (int g = g0; g < g1 && !(subs[g].seg & SEG_FIRST); ++g) {
    if (in_dead[tid]) {
      subs[g].first = in_n[tid];
      subs[g].dead = 1;
    } else {
      subs[g].first += in_n[tid];
      subs[g].pred[0] += in_dc[0][tid];
      subs[g].pred[1] += in_dc[1][tid];
      subs[g].pred[2] += in_dc[2][tid];
    }
  }
  __syncthreads();
  // status: the first segment that breaks a rule; within it an invalid code ahead of its last block (1) goes before its count (2, 3)
  for (int g = g0; g < g1; ++g) {
    const SubState s = subs[g];
    const int j = s.seg & SEG_MASK;
    long long base;
    const int want = seg_blocks(geo, j, &base);
    const int jj = j < (1 << 28) ? j : (1 << 28) - 1;
    if (!s.dead && s.errn >= 0 && s.first + s.errn < want) atomicMin(&key_s, jj * 4 + 1);
    if (s.seg & SEG_LAST) {
      const int total = s.dead ? s.first : s.first + (s.errn >= 0 ? s.errn : s.n);
      if (total < want) atomicMin(&key_s, jj * 4 + 2);
      if (total > want) atomicMin(&key_s, jj * 4 + 3);
    }
  }
  __syncthreads();
  if (tid == 0) status[frame0 + blockIdx.x] = key_s == 0x7FFFFFFF ? 0 : key_s & 3;
}

// grid (ceil(subsequences of the largest frame / 256), frames of this launch), 256 threads.  coef: [frame][blocks][64] int16, zeroed.
__global__ __launch_bounds__(256) void jpegdec_write_kernel(const unsigned char* __restrict__ data, DecRecs recs, int frame0, int H, int W, int chunk_bits,
                                                            const SubState* __restrict__ subs_all, short* __restrict__ coef_all, long long coef_stride) {
  __shared__ unsigned tab_s[TAB_BYTES / 4];
  const DecRec rec = recs.r[blockIdx.y];
  if (rec.pre_status || (int)(blockIdx.x * 256u) >= rec.nsub) return;      // uniform
  load_tables(data, rec, tab_s, threadIdx.x, 256);
  __syncthreads();
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= rec.nsub) return;
  const SubState s = subs_all[rec.sub_base + g];
  if (s.dead) return;
  const Geo geo = geometry(H, W, rec.sub, rec.ri);
  SegList sl;
  sl.w = reinterpret_cast<const int*>(data + rec.seg_off);
  sl.nseg = rec.nseg;
  sl.scan_len = rec.scan_len;
  const int j = s.seg & SEG_MASK;
  unsigned b0, b1;
  bool is_first, is_last;
  const Stream st = sub_range(data + rec.scan_off, sl, j, g, chunk_bits, &b0, &b1, &is_first, &is_last);
  long long base;
  const int want = seg_blocks(geo, j, &base);
  int pred[3] = {s.pred[0], s.pred[1], s.pred[2]};
  short* coef = coef_all + (long long)(frame0 + blockIdx.y) * coef_stride + base * 64;
  run_sub<true>(st, reinterpret_cast<const unsigned char*>(tab_s), geo.bpm, s.ent_p, s.ent_sz, b1, s.first, want, pred, coef);
}

// One pass of libjpeg's accurate integer inverse DCT (jidctint: 13 constant bits) on eight values, descaled by N bits.
template <int N>
__device__ __forceinline__ void idct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  constexpr int R = 1 << (N - 1);
  int z1 = (d2 + d6) * 4433;
  const int e2 = z1 - d6 * 15137, e3 = z1 + d2 * 6270;
  const int e0 = (d0 + d4) << 13, e1 = (d0 - d4) << 13;
  const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  int t0 = d7, t1 = d5, t2 = d3, t3 = d1;
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * 9633;
  t0 *= 2446;
  t1 *= 16819;
  t2 *= 25172;
  t3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  d0 = (t10 + t3 + R) >> N;
  d7 = (t10 - t3 + R) >> N;
  d1 = (t11 + t2 + R) >> N;
  d6 = (t11 - t2 + R) >> N;
  d2 = (t12 + t1 + R) >> N;
  d5 = (t12 - t1 + R) >> N;
  d3 = (t13 + t0 + R) >> N;
  d4 = (t13 - t0 + R) >> N;
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
  const unsigned short* q = q_s + 64 * c;
  int d[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint4 v = src[i];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d[8 * i + 2 * k] = (int)(short)(w[k] & 0xFFFFu) * (int)q[8 * i + 2 * k];
      d[8 * i + 2 * k + 1] = (int)(short)(w[k] >> 16) * (int)q[8 * i + 2 * k + 1];
    }
  }
#pragma unroll
  for (int x = 0; x < 8; ++x) idct8<11>(d[x], d[8 + x], d[16 + x], d[24 + x], d[32 + x], d[40 + x], d[48 + x], d[56 + x]);      // columns first
#pragma unroll
  for (int y = 0; y < 8; ++y) idct8<18>(d[y * 8], d[y * 8 + 1], d[y * 8 + 2], d[y * 8 + 3], d[y * 8 + 4], d[y * 8 + 5], d[y * 8 + 6], d[y * 8 + 7]);
  const Planes pl = planes_of(geo);
  unsigned char* dst = planes_all + (long long)(frame0 + blockIdx.y) * plane_stride + pl.off[c] + ((long long)by * 8) * pl.pw[c] + bx * 8;
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      lo |= (unsigned)clampi(d[y * 8 + x] + 128, 0, 255) << (8 * x);
      hi |= (unsigned)clampi(d[y * 8 + 4 + x] + 128, 0, 255) << (8 * x);
    }
    *reinterpret_cast<uint2*>(dst + (long long)y * pl.pw[c]) = make_uint2(lo, hi);
  }
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
  unsigned char px[12];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int yv = (int)((yy >> (8 * i)) & 0xFFu), u = cb[i] - 128, v = cr[i] - 128;
    px[3 * i] = (unsigned char)clampi(yv + ((116130 * u + 32768) >> 16), 0, 255);
    px[3 * i + 1] = (unsigned char)clampi(yv + ((-22554 * u - 46802 * v + 32768) >> 16), 0, 255);
    px[3 * i + 2] = (unsigned char)clampi(yv + ((91881 * v + 32768) >> 16), 0, 255);
  }
  unsigned char* dst = out + ((long long)(frame0 + blockIdx.y) * H + y) * W * 3 + (long long)x0 * 3;
  if (x0 + 4 <= W && ((uintptr_t)dst & 3) == 0) {
    unsigned* dw = reinterpret_cast<unsigned*>(dst);
#pragma unroll
    for (int i = 0; i < 3; ++i)
      dw[i] = (unsigned)px[4 * i] | ((unsigned)px[4 * i + 1] << 8) | ((unsigned)px[4 * i + 2] << 16) | ((unsigned)px[4 * i + 3] << 24);
  } else {
    const int n = W - x0 < 4 ? W - x0 : 4;
    for (int i = 0; i < 3 * n; ++i) dst[i] = px[i];
  }
}

long long align_up(long long v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

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
    CASYNC_REQUIRE(subsampling == 0 || sub == 2, "jpegdec_decode: record %d is 4:4:4 in a call sized for 4:2:0", f);
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
