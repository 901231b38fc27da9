// What the two JPEG decoders (jpeg_dec.hip: 4:4:4 and 4:2:0; jpeg_dec_mjpeg.hip: those plus 4:2:2, grayscale and files without
// their Huffman tables) have in common on the device: the record and the subsequence state, the bit reader of a restart segment,
// the Huffman lookup, the symbol loop of a subsequence, the bodies of the plan (sync) and write kernels, libjpeg's islow inverse
// DCT of one block and the colour arithmetic of four pixels.  A sampling traits type S tells them the geometry of an MCU
// (S::geometry) and the component of each of its block slots (S::comp).  Everything sits in the anonymous namespace: the two
// objects stay independent translation units, each with its own kernels under its own names.  Each .hip keeps its traits, the
// layout of its sample planes, its four __global__ kernels, its upsampling and the host side of its two entries.
//
// Bounds (the rules at the top of jpeg_dec.hip hold for every user of this header): no stream content forms an address or bounds
// a loop; bit reads past a segment's end return zeros; every value read from a table or a segment list is clamped or masked
// before use; no global atomics.
#pragma once
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
template <bool WRITE, class S>
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
    const int c = S::comp(bpm, s);
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

// The plan kernel's body: grid (frames of this launch), SYNC_THREADS.  subs: every frame's subsequences, frame f's from rec.sub_base on.
template <class S>
__device__ __forceinline__ void sync_body(const unsigned char* __restrict__ data, const DecRecs& recs, int frame0, int H, int W, int chunk_bits,
                                          SubState* subs_all, int* __restrict__ status) {
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
  const Geo geo = S::geometry(H, W, rec.sub, rec.ri);
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
      const SubResult r = run_sub<false, S>(st, tab, geo.bpm, subs[g].ent_p, subs[g].ent_sz, b1, 0, 0, nullptr, nullptr);
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

// The write kernel's body: grid (ceil(subsequences of the largest frame / 256), frames of this launch), 256 threads.  coef: [frame][blocks][64] int16, zeroed.
template <class S>
__device__ __forceinline__ void write_body(const unsigned char* __restrict__ data, const DecRecs& recs, int frame0, int H, int W, int chunk_bits,
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
  const Geo geo = S::geometry(H, W, rec.sub, rec.ri);
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
  run_sub<true, S>(st, reinterpret_cast<const unsigned char*>(tab_s), geo.bpm, s.ent_p, s.ent_sz, b1, s.first, want, pred, coef);
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

// One block: 64 int16 coefficients in natural order at src, dequantised by q [64] (natural order), through the two passes of
// jidctint (columns first), +128, clamp, eight 8-byte stores into a sample plane of `pitch` bytes a row.
__device__ __forceinline__ void idct_block(const uint4* __restrict__ src, const unsigned short* q, unsigned char* __restrict__ dst, long long pitch) {
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
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      lo |= (unsigned)clampi(d[y * 8 + x] + 128, 0, 255) << (8 * x);
      hi |= (unsigned)clampi(d[y * 8 + 4 + x] + 128, 0, 255) << (8 * x);
    }
    *reinterpret_cast<uint2*>(dst + (long long)y * pitch) = make_uint2(lo, hi);
  }
}

// Four pixels of a row: Y in the bytes of yy, Cb and Cr per pixel -> BGR at dst (the row's pixel x0 of W), 4-byte stores where the
// row allows.
__device__ __forceinline__ void store_bgr4(unsigned yy, const int* cb, const int* cr, unsigned char* __restrict__ dst, int x0, int W) {
  unsigned char px[12];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int yv = (int)((yy >> (8 * i)) & 0xFFu), u = cb[i] - 128, v = cr[i] - 128;
    px[3 * i] = (unsigned char)clampi(yv + ((116130 * u + 32768) >> 16), 0, 255);
    px[3 * i + 1] = (unsigned char)clampi(yv + ((-22554 * u - 46802 * v + 32768) >> 16), 0, 255);
    px[3 * i + 2] = (unsigned char)clampi(yv + ((91881 * v + 32768) >> 16), 0, 255);
  }
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

__host__ inline long long align_up(long long v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

}  // namespace
