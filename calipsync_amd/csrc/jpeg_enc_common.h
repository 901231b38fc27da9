// What the two baseline JPEG encoders (jpeg_enc.hip 4:4:4, jpeg_enc420.hip 4:2:0) have in common, device and host: the Annex K
// tables, the integer DCT and the quantisation of one block, the bit buffer's put_bits, the AC walk of a block, the close of a
// row, the plan and pack kernels' bodies, the 629-byte header and the host side of the three entries, to which a JpegVariant
// describes a sampling.  Everything sits in the anonymous namespace: the two objects stay independent translation units, each with
// its own copy of the tables and its own kernels under its own names.  Each .hip keeps its pixel load, its colour (and downsample)
// code, the order of an MCU's blocks and its row kernel.
#pragma once
#include "common.h"

namespace {

constexpr int HEADER_BYTES = 629;
constexpr int BITBUF_WORDS = 2048;                 // bits of a chunk in flight: 8 KB before a second window
constexpr unsigned ROW_OVERFLOW = 0xFFFFFFFFu;     // row length of a row that outgrew its slot
constexpr int MAX_FRAMES_PER_LAUNCH = 32768;       // grid.y

struct JpegQuant {                                 // zigzag order: luma, chroma
  unsigned short q[2][64];
  float rcp[2][64];                                // 1 / (8 q), rounded to nearest
};
struct JpegHeader { unsigned w[(HEADER_BYTES + 3) / 4]; };

__device__ const unsigned HUFF_DC_LUMA[12] = {
    0x20000, 0x30002, 0x30003, 0x30004, 0x30005, 0x30006, 0x4000e, 0x5001e, 0x6003e, 0x7007e, 0x800fe, 0x901fe,
};
__device__ const unsigned HUFF_AC_LUMA[256] = {
    0x4000a, 0x20000, 0x20001, 0x30004, 0x4000b, 0x5001a, 0x70078, 0x800f8, 0xa03f6, 0x10ff82, 0x10ff83, 0x00000,
    0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x4000c, 0x5001b, 0x70079, 0x901f6, 0xb07f6, 0x10ff84, 0x10ff85,
    0x10ff86, 0x10ff87, 0x10ff88, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x5001c, 0x800f9, 0xa03f7,
    0xc0ff4, 0x10ff89, 0x10ff8a, 0x10ff8b, 0x10ff8c, 0x10ff8d, 0x10ff8e, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x6003a, 0x901f7, 0xc0ff5, 0x10ff8f, 0x10ff90, 0x10ff91, 0x10ff92, 0x10ff93, 0x10ff94, 0x10ff95, 0x00000,
    0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x6003b, 0xa03f8, 0x10ff96, 0x10ff97, 0x10ff98, 0x10ff99, 0x10ff9a,
    0x10ff9b, 0x10ff9c, 0x10ff9d, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x7007a, 0xb07f7, 0x10ff9e,
    0x10ff9f, 0x10ffa0, 0x10ffa1, 0x10ffa2, 0x10ffa3, 0x10ffa4, 0x10ffa5, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x7007b, 0xc0ff6, 0x10ffa6, 0x10ffa7, 0x10ffa8, 0x10ffa9, 0x10ffaa, 0x10ffab, 0x10ffac, 0x10ffad, 0x00000,
    0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x800fa, 0xc0ff7, 0x10ffae, 0x10ffaf, 0x10ffb0, 0x10ffb1, 0x10ffb2,
    0x10ffb3, 0x10ffb4, 0x10ffb5, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x901f8, 0xf7fc0, 0x10ffb6,
    0x10ffb7, 0x10ffb8, 0x10ffb9, 0x10ffba, 0x10ffbb, 0x10ffbc, 0x10ffbd, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901f9, 0x10ffbe, 0x10ffbf, 0x10ffc0, 0x10ffc1, 0x10ffc2, 0x10ffc3, 0x10ffc4, 0x10ffc5, 0x10ffc6, 0x00000,
    0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x901fa, 0x10ffc7, 0x10ffc8, 0x10ffc9, 0x10ffca, 0x10ffcb, 0x10ffcc,
    0x10ffcd, 0x10ffce, 0x10ffcf, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0xa03f9, 0x10ffd0, 0x10ffd1,
    0x10ffd2, 0x10ffd3, 0x10ffd4, 0x10ffd5, 0x10ffd6, 0x10ffd7, 0x10ffd8, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0xa03fa, 0x10ffd9, 0x10ffda, 0x10ffdb, 0x10ffdc, 0x10ffdd, 0x10ffde, 0x10ffdf, 0x10ffe0, 0x10ffe1, 0x00000,
    0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0xb07f8, 0x10ffe2, 0x10ffe3, 0x10ffe4, 0x10ffe5, 0x10ffe6, 0x10ffe7,
    0x10ffe8, 0x10ffe9, 0x10ffea, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x10ffeb, 0x10ffec, 0x10ffed,
    0x10ffee, 0x10ffef, 0x10fff0, 0x10fff1, 0x10fff2, 0x10fff3, 0x10fff4, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0xb07f9, 0x10fff5, 0x10fff6, 0x10fff7, 0x10fff8, 0x10fff9, 0x10fffa, 0x10fffb, 0x10fffc, 0x10fffd, 0x10fffe, 0x00000,
    0x00000, 0x00000, 0x00000, 0x00000,
};
__device__ const unsigned HUFF_DC_CHROMA[12] = {
    0x20000, 0x20001, 0x20002, 0x30006, 0x4000e, 0x5001e, 0x6003e, 0x7007e, 0x800fe, 0x901fe, 0xa03fe, 0xb07fe,
};
__device__ const unsigned HUFF_AC_CHROMA[256] = {
    0x20000, 0x20001, 0x30004, 0x4000a, 0x50018, 0x50019, 0x60038, 0x70078, 0x901f4, 0xa03f6, 0xc0ff4, 0x00000,
    0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x4000b, 0x60039, 0x800f6, 0x901f5, 0xb07f6, 0xc0ff5, 0x10ff88,
    0x10ff89, 0x10ff8a, 0x10ff8b, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x5001a, 0x800f7, 0xa03f7,
    0xc0ff6, 0xf7fc2, 0x10ff8c, 0x10ff8d, 0x10ff8e, 0x10ff8f, 0x10ff90, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x5001b, 0x800f8, 0xa03f8, 0xc0ff7, 0x10ff91, 0x10ff92, 0x10ff93, 0x10ff94, 0x10ff95, 0x10ff96, 0x00000,
    0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x6003a, 0x901f6, 0x10ff97, 0x10ff98, 0x10ff99, 0x10ff9a, 0x10ff9b,
    0x10ff9c, 0x10ff9d, 0x10ff9e, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x6003b, 0xa03f9, 0x10ff9f,
    0x10ffa0, 0x10ffa1, 0x10ffa2, 0x10ffa3, 0x10ffa4, 0x10ffa5, 0x10ffa6, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x70079, 0xb07f7, 0x10ffa7, 0x10ffa8, 0x10ffa9, 0x10ffaa, 0x10ffab, 0x10ffac, 0x10ffad, 0x10ffae, 0x00000,
    0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x7007a, 0xb07f8, 0x10ffaf, 0x10ffb0, 0x10ffb1, 0x10ffb2, 0x10ffb3,
    0x10ffb4, 0x10ffb5, 0x10ffb6, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x800f9, 0x10ffb7, 0x10ffb8,
    0x10ffb9, 0x10ffba, 0x10ffbb, 0x10ffbc, 0x10ffbd, 0x10ffbe, 0x10ffbf, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901f7, 0x10ffc0, 0x10ffc1, 0x10ffc2, 0x10ffc3, 0x10ffc4, 0x10ffc5, 0x10ffc6, 0x10ffc7, 0x10ffc8, 0x00000,
    0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x901f8, 0x10ffc9, 0x10ffca, 0x10ffcb, 0x10ffcc, 0x10ffcd, 0x10ffce,
    0x10ffcf, 0x10ffd0, 0x10ffd1, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x901f9, 0x10ffd2, 0x10ffd3,
    0x10ffd4, 0x10ffd5, 0x10ffd6, 0x10ffd7, 0x10ffd8, 0x10ffd9, 0x10ffda, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901fa, 0x10ffdb, 0x10ffdc, 0x10ffdd, 0x10ffde, 0x10ffdf, 0x10ffe0, 0x10ffe1, 0x10ffe2, 0x10ffe3, 0x00000,
    0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0xb07f9, 0x10ffe4, 0x10ffe5, 0x10ffe6, 0x10ffe7, 0x10ffe8, 0x10ffe9,
    0x10ffea, 0x10ffeb, 0x10ffec, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000, 0xe3fe0, 0x10ffed, 0x10ffee,
    0x10ffef, 0x10fff0, 0x10fff1, 0x10fff2, 0x10fff3, 0x10fff4, 0x10fff5, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0xa03fa, 0xf7fc3, 0x10fff6, 0x10fff7, 0x10fff8, 0x10fff9, 0x10fffa, 0x10fffb, 0x10fffc, 0x10fffd, 0x10fffe, 0x00000,
    0x00000, 0x00000, 0x00000, 0x00000,
};
const unsigned char DHT_DC_LUMA[28] = {
    0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7,
    8, 9, 10, 11,
};
const unsigned char DHT_AC_LUMA[178] = {
    0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125, 1, 2, 3, 0, 4, 17, 5, 18,
    33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240,
    36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57,
    58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105,
    106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152,
    153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197,
    198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234,
    241, 242, 243, 244, 245, 246, 247, 248, 249, 250,
};
const unsigned char DHT_DC_CHROMA[28] = {
    0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7,
    8, 9, 10, 11,
};
const unsigned char DHT_AC_CHROMA[178] = {
    0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119, 0, 1, 2, 3, 17, 4, 5, 33,
    49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
    21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56,
    57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104,
    105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150,
    151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195,
    196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233,
    234, 242, 243, 244, 245, 246, 247, 248, 249, 250,
};
const unsigned char BASE_LUMA[64] = {
    16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
    56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99,
};
const unsigned char BASE_CHROMA[64] = {
    17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
};
constexpr int ZZ_OF[64] = {
    0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63,
};

// One pass of libjpeg's accurate integer forward DCT (13 constant bits, 2 extra bits between the passes) on eight values.
template <bool FIRST>
__device__ __forceinline__ void fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  constexpr int N = FIRST ? 11 : 15, R = 1 << (N - 1);
  const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) {
    d0 = (t10 + t11) << 2;
    d4 = (t10 - t11) << 2;
  } else {
    d0 = (t10 + t11 + 2) >> 2;
    d4 = (t10 - t11 + 2) >> 2;
  }
  int z1 = (t12 + t13) * 4433;
  d2 = (z1 + t13 * 6270 + R) >> N;
  d6 = (z1 - t12 * 15137 + R) >> N;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d7 = (u4 + z1 + z3 + R) >> N;
  d5 = (u5 + z2 + z4 + R) >> N;
  d3 = (u6 + z2 + z3 + R) >> N;
  d1 = (u7 + z1 + z4 + R) >> N;
}

// The 64 level-shifted samples of one block (row-major) -> DCT, quantisation by table `tab` (0 luma, 1 chroma).  The coefficients
// 4g .. 4g + 3 (zigzag order, 16 bits each, the first in the low half of .x) go to out[g * 64]: sixteen 8-byte stores a lane, the
// lanes side by side, and the walk reads four coefficients at a time.
__device__ __forceinline__ void transform_block(int (&d)[64], const JpegQuant& qt, int tab, uint2* out) {
#pragma unroll
  for (int y = 0; y < 8; ++y) fdct8<true>(d[y * 8], d[y * 8 + 1], d[y * 8 + 2], d[y * 8 + 3], d[y * 8 + 4], d[y * 8 + 5], d[y * 8 + 6], d[y * 8 + 7]);
#pragma unroll
  for (int x = 0; x < 8; ++x) fdct8<false>(d[x], d[8 + x], d[16 + x], d[24 + x], d[32 + x], d[40 + x], d[48 + x], d[56 + x]);
  const unsigned short* q = qt.q[tab];
  const float* rcp = qt.rcp[tab];
  unsigned half[64];                                            // by zigzag position, 16 bits each
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    const int k = ZZ_OF[i];
    const unsigned div = 8u * q[k];
    const unsigned a = d[i] < 0 ? (unsigned)-d[i] : (unsigned)d[i];
    // round half away from zero: floor(n / div) with n < 2^16.  n * rcp is within one of it (both factors are exact to 2^-24),
    // and the remainder says which way
    const unsigned n = a + (div >> 1);
    int m = (int)((float)n * rcp[k]);
    const int rem = (int)n - m * (int)div;
    m += rem < 0 ? -1 : rem >= (int)div ? 1 : 0;
    half[k] = (unsigned)(d[i] < 0 ? -m : m) & 0xFFFFu;
  }
#pragma unroll
  for (int g = 0; g < 16; ++g) out[g * 64] = make_uint2(half[4 * g] | (half[4 * g + 1] << 16), half[4 * g + 2] | (half[4 * g + 3] << 16));
}

// `len` bits of `code` (MSB first) at bit `pos` of the chunk's stream, into the window of the bit buffer that starts at word
// `winbase`: the words outside the window are another window's.  A bit is 1 in one code only, so OR is exact.
__device__ __forceinline__ void put_bits(unsigned* bitbuf, unsigned winbase, unsigned pos, unsigned code, unsigned len) {
  const unsigned long long v = (unsigned long long)code << (64u - len - (pos & 31u));        // len + (pos & 31) <= 26 + 31
  const unsigned w = (pos >> 5) - winbase, hi = (unsigned)(v >> 32), lo = (unsigned)v;
  if (hi && w < (unsigned)BITBUF_WORDS) atomicOr(&bitbuf[w], hi);
  if (lo && w + 1u < (unsigned)BITBUF_WORDS) atomicOr(&bitbuf[w + 1u], lo);
}

// The 63 AC coefficients of the block whose sixteen words lie at cw[g * 64], `next` being cw[0] (its DC position is skipped):
// run lengths with ZRL and EOB through `word(entry, value, category)`.  Four coefficients a read, the next read in flight.
template <typename Word>
__device__ __forceinline__ void walk_ac(const uint2* cw, uint2 next, const unsigned* ac_tab, Word& word) {
  int run = 0;
  for (int g = 0; g < 16; ++g) {
    uint2 four = next;
    if (g < 15) next = cw[(g + 1) * 64];
    if (g == 0) four.x &= 0xFFFF0000u;                          // the DC coefficient is the caller's
    if ((four.x | four.y) == 0u) {
      run += g == 0 ? 3 : 4;
      continue;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j == 0 && g == 0) continue;
      const unsigned w = j < 2 ? four.x : four.y;
      const int v = (int)(short)(j & 1 ? w >> 16 : w & 0xFFFFu);
      if (v == 0) {
        ++run;
        continue;
      }
      for (; run > 15; run -= 16) word(ac_tab[0xF0], 0, 0);     // ZRL
      const unsigned cat = 32u - __clz(v < 0 ? -v : v);
      word(ac_tab[(run << 4) | cat], v, cat);
      run = 0;
    }
  }
  if (run) word(ac_tab[0], 0, 0);                               // EOB
}

// Lane 0 closes the row: RSTn between rows, EOI after the last (never stuffed), and the row's length or ROW_OVERFLOW.
__device__ __forceinline__ void close_row(unsigned char* dst, unsigned cap, unsigned out_pos, int row, int rows, unsigned* len) {
  if (out_pos < cap) dst[out_pos] = 0xFF;
  if (out_pos + 1u < cap) dst[out_pos + 1u] = (unsigned char)(row + 1 < rows ? 0xD0 + (row & 7) : 0xD9);
  *len = out_pos + 2u <= cap ? out_pos + 2u : ROW_OVERFLOW;
}

// The plan kernel of either encoder: one workgroup of 256.  offsets [B+1], status [B].
__device__ __forceinline__ void jpeg_plan_body(const unsigned* __restrict__ row_len, int batch, int rows, long long out_cap,
                                               long long* __restrict__ offsets, int* __restrict__ status) {
  __shared__ long long size_s[256];
  __shared__ int status_s[256];
  const int tid = threadIdx.x;
  long long run = 0;                                            // thread 0's: bytes of the frames so far
  for (int base = 0; base < batch; base += 256) {
    const int f = base + tid;
    if (f < batch) {
      const unsigned* len = row_len + (size_t)f * rows;
      long long sum = HEADER_BYTES;
      bool outgrew = false;
      for (int r = 0; r < rows; ++r) {
        const unsigned l = len[r];
        outgrew |= l == ROW_OVERFLOW;
        sum += l;
      }
      size_s[tid] = outgrew ? 0 : sum;
      status_s[tid] = outgrew ? 1 : 0;
    }
    __syncthreads();
    if (tid == 0) {
      const int n = batch - base < 256 ? batch - base : 256;
      for (int i = 0; i < n; ++i) {
        long long size = size_s[i];
        int st = status_s[i];
        if (st == 0 && run + size > out_cap) {                  // a failed frame contributes nothing; the next one may still fit
          st = 2;
          size = 0;
        }
        offsets[base + i] = run;
        status[base + i] = st;
        run += size;
      }
    }
    __syncthreads();
  }
  if (tid == 0) offsets[batch] = run;
}

// n bytes s -> d by the 256 threads of a workgroup: aligned words to d, single bytes at its two ends.
__device__ __forceinline__ void copy_bytes(unsigned char* d, const unsigned char* s, unsigned n, int tid) {
  unsigned head = (0u - (unsigned)(uintptr_t)d) & 3u;
  if (head > n) head = n;
  const unsigned n_words = (n - head) >> 2, done = head + n_words * 4u;
  if (tid < (int)head) d[tid] = s[tid];
  if (tid >= 32 && tid - 32 < (int)(n - done)) d[done + tid - 32] = s[done + tid - 32];
  unsigned* dw = reinterpret_cast<unsigned*>(d + head);
  const unsigned char* sb = s + head;
  if (((uintptr_t)sb & 3) == 0) {
    const unsigned* sw = reinterpret_cast<const unsigned*>(sb);
    for (unsigned i = tid; i < n_words; i += 256u) dw[i] = sw[i];
  } else {
    for (unsigned i = tid; i < n_words; i += 256u) {
      const unsigned char* q = sb + (size_t)i * 4;
      dw[i] = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16) | ((unsigned)q[3] << 24);
    }
  }
}

// The pack kernel of either encoder: grid (rows, frames of this launch), 256 threads.
__device__ __forceinline__ void jpeg_pack_body(const unsigned* __restrict__ row_len, const unsigned char* __restrict__ slots, int frame0,
                                               long long slot_bytes, const JpegHeader& header, const long long* __restrict__ offsets,
                                               const int* __restrict__ status, unsigned char* __restrict__ out) {
  __shared__ unsigned long long part[256];
  __shared__ unsigned header_s[(HEADER_BYTES + 3) / 4];
  const int tid = threadIdx.x, row = blockIdx.x, rows = gridDim.x;
  const size_t frame = (size_t)frame0 + blockIdx.y;
  if (status[frame] != 0) return;                               // uniform: the frame contributes no byte
  const unsigned* len = row_len + frame * rows;
  unsigned long long ahead = 0;
  for (int r = tid; r < row; r += 256) ahead += len[r];
  part[tid] = ahead;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) part[tid] += part[tid + s];
    __syncthreads();
  }
  unsigned char* frame_out = out + offsets[frame];
  if (row == 0) {
    if (tid < (HEADER_BYTES + 3) / 4) header_s[tid] = header.w[tid];
    __syncthreads();
    copy_bytes(frame_out, reinterpret_cast<const unsigned char*>(header_s), HEADER_BYTES, tid);
  }
  copy_bytes(frame_out + HEADER_BYTES + part[0], slots + (frame * rows + row) * (size_t)slot_bytes, len[row], tid);
}

// ---- host ----
// One sampling, as the shared host code sees it.
struct JpegVariant {
  const char* name;                                // "jpeg" or "jpeg420": the prefix of its entries, as the messages spell it
  int mcu;                                         // edge of an MCU in pixels, 8 or 16: a row of the kernels is a row of MCUs
  int blocks;                                      // 8 x 8 blocks an MCU codes, 3 or 6
  void (*rows_kernel)(const unsigned char*, int, int, int, JpegQuant, long long, unsigned*, unsigned char*);
  void (*plan_kernel)(const unsigned*, int, int, long long, long long*, int*);
  void (*pack_kernel)(const unsigned*, const unsigned char*, int, long long, JpegHeader, const long long*, const int*, unsigned char*);
};

int check_size(const JpegVariant& v, const char* entry, int H, int W, int quality) {
  CASYNC_REQUIRE(H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "%s_%s: a frame of %d x %d (h x w) is outside 1..65535", v.name, entry, H, W);
  CASYNC_REQUIRE(quality >= 1 && quality <= 100, "%s_%s: quality %d is outside 1..100", v.name, entry, quality);
  return CASYNC_OK;
}

void quant_tables(int quality, JpegQuant& qt) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) {
      const int v = ((t ? BASE_CHROMA : BASE_LUMA)[k] * scale + 50) / 100;
      qt.q[t][k] = (unsigned short)(v < 1 ? 1 : v > 255 ? 255 : v);
      qt.rcp[t][k] = 1.0f / (float)(8 * qt.q[t][k]);
    }
}

unsigned char* segment(unsigned char* p, int marker, const unsigned char* body, int n) {
  *p++ = 0xFF;
  *p++ = (unsigned char)marker;
  *p++ = (unsigned char)((n + 2) >> 8);
  *p++ = (unsigned char)((n + 2) & 0xFF);
  for (int i = 0; i < n; ++i) *p++ = body[i];
  return p;
}

// The HEADER_BYTES from SOI to SOS.  luma_sampling: 0x11, or 0x22 where Y samples 2 x 2; one restart interval per row of MCUs.
void build_header(int H, int W, const JpegQuant& qt, int luma_sampling, int mcu, unsigned char* out) {
  unsigned char* p = out;
  unsigned char body[192];
  *p++ = 0xFF;
  *p++ = 0xD8;
  const unsigned char jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  p = segment(p, 0xE0, jfif, 14);
  for (int t = 0; t < 2; ++t) {
    body[0] = (unsigned char)t;
    for (int k = 0; k < 64; ++k) body[1 + k] = (unsigned char)qt.q[t][k];
    p = segment(p, 0xDB, body, 65);
  }
  const unsigned char sof[15] = {8, (unsigned char)(H >> 8), (unsigned char)(H & 0xFF), (unsigned char)(W >> 8), (unsigned char)(W & 0xFF),
                                 3, 1, (unsigned char)luma_sampling, 0, 2, 0x11, 1, 3, 0x11, 1};
  p = segment(p, 0xC0, sof, 15);
  const struct { int id; const unsigned char* t; int n; } dht[4] = {{0x00, DHT_DC_LUMA, (int)sizeof(DHT_DC_LUMA)}, {0x10, DHT_AC_LUMA, (int)sizeof(DHT_AC_LUMA)},
                                                                   {0x01, DHT_DC_CHROMA, (int)sizeof(DHT_DC_CHROMA)},
                                                                   {0x11, DHT_AC_CHROMA, (int)sizeof(DHT_AC_CHROMA)}};
  for (const auto& h : dht) {
    body[0] = (unsigned char)h.id;
    for (int i = 0; i < h.n; ++i) body[1 + i] = h.t[i];
    p = segment(p, 0xC4, body, 1 + h.n);
  }
  const int interval = (W + mcu - 1) / mcu;
  const unsigned char dri[2] = {(unsigned char)(interval >> 8), (unsigned char)(interval & 0xFF)};
  p = segment(p, 0xDD, dri, 2);
  const unsigned char sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  p = segment(p, 0xDA, sos, 10);
}

constexpr long long LEN_ALIGN = 256;                            // the slots start on a 256-byte boundary of the scratch buffer

long long lengths_bytes(long long batch, int rows) { return (batch * rows * 4 + LEN_ALIGN - 1) / LEN_ALIGN * LEN_ALIGN; }

// slot_bytes 0: twice the raw bytes of the samples a row of MCUs codes
long long default_slot(const JpegVariant& v, int W) { return 2ll * 64 * v.blocks * ((W + v.mcu - 1) / v.mcu); }

// casync_op_<name>_header
int jpeg_header_entry(const JpegVariant& v, int H, int W, int quality, uint8_t* out, int cap) {
  if (int st = check_size(v, "header", H, W, quality)) return st;
  CASYNC_REQUIRE(out && cap >= HEADER_BYTES, "%s_header: needs %d bytes, got %d", v.name, HEADER_BYTES, out ? cap : 0);
  JpegQuant qt;
  quant_tables(quality, qt);
  build_header(H, W, qt, 0x11 * (v.mcu / 8), v.mcu, out);
  return HEADER_BYTES;
}

// casync_op_<name>_workspace_bytes
int64_t jpeg_workspace_entry(const JpegVariant& v, int batch, int H, int W, int64_t slot_bytes) {
  if (int st = check_size(v, "workspace_bytes", H, W, 50)) return st;
  CASYNC_REQUIRE(batch >= 0 && slot_bytes >= 0, "%s_workspace_bytes: batch %d, slot_bytes %lld", v.name, batch, (long long)slot_bytes);
  const int rows = (H + v.mcu - 1) / v.mcu;
  if (slot_bytes == 0) slot_bytes = default_slot(v, W);
  return lengths_bytes(batch, rows) + (long long)batch * rows * slot_bytes;
}

// casync_op_<name>_encode
int jpeg_encode_entry(const JpegVariant& v, const uint8_t* frames_bgr, int batch, int H, int W, int quality, int64_t slot_bytes, uint8_t* scratch,
                      int64_t scratch_bytes, uint8_t* out, int64_t out_cap, int64_t* offsets, int32_t* status, casync_stream stream) {
  if (int st = check_size(v, "encode", H, W, quality)) return st;
  CASYNC_REQUIRE(batch >= 0, "%s_encode: batch %d", v.name, batch);
  CASYNC_REQUIRE(slot_bytes >= 0 && out_cap >= 0, "%s_encode: slot_bytes %lld, out_cap %lld", v.name, (long long)slot_bytes, (long long)out_cap);
  if (batch == 0) return CASYNC_OK;
  CASYNC_REQUIRE(frames_bgr && scratch && out && offsets && status, "%s_encode: null pointer", v.name);
  CASYNC_REQUIRE(((uintptr_t)scratch & 3) == 0 && ((uintptr_t)offsets & 7) == 0 && ((uintptr_t)status & 3) == 0,
                 "%s_encode: scratch and status must be 4-byte aligned, offsets 8-byte aligned", v.name);
  const int rows = (H + v.mcu - 1) / v.mcu;
  if (slot_bytes == 0) slot_bytes = default_slot(v, W);
  const long long need = lengths_bytes(batch, rows) + (long long)batch * rows * slot_bytes;
  CASYNC_REQUIRE(scratch_bytes >= need, "%s_encode: scratch of %lld bytes, casync_op_%s_workspace_bytes says %lld", v.name, (long long)scratch_bytes,
                 v.name, need);
  JpegQuant qt;
  quant_tables(quality, qt);
  JpegHeader header = {};
  build_header(H, W, qt, 0x11 * (v.mcu / 8), v.mcu, reinterpret_cast<unsigned char*>(header.w));
  unsigned* row_len = reinterpret_cast<unsigned*>(scratch);
  unsigned char* slots = scratch + lengths_bytes(batch, rows);
  hipStream_t s = (hipStream_t)stream;
  for (int f0 = 0; f0 < batch; f0 += MAX_FRAMES_PER_LAUNCH) {
    const int n = batch - f0 < MAX_FRAMES_PER_LAUNCH ? batch - f0 : MAX_FRAMES_PER_LAUNCH;
    if (int st = casync_launch(v.rows_kernel, dim3(rows, n), dim3(64), 0, s, frames_bgr, f0, H, W, qt, (long long)slot_bytes, row_len, slots)) return st;
  }
  if (int st = casync_launch(v.plan_kernel, dim3(1), dim3(256), 0, s, (const unsigned*)row_len, batch, rows, (long long)out_cap, (long long*)offsets,
                             (int*)status))
    return st;
  for (int f0 = 0; f0 < batch; f0 += MAX_FRAMES_PER_LAUNCH) {
    const int n = batch - f0 < MAX_FRAMES_PER_LAUNCH ? batch - f0 : MAX_FRAMES_PER_LAUNCH;
    if (int st = casync_launch(v.pack_kernel, dim3(rows, n), dim3(256), 0, s, (const unsigned*)row_len, (const unsigned char*)slots, f0,
                               (long long)slot_bytes, header, (const long long*)offsets, (const int*)status, out))
      return st;
  }
  return CASYNC_OK;
}

}  // namespace
