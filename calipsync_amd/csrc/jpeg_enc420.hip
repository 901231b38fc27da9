// 4:2:0 baseline JPEG of finished frames on the device: uint8 BGR [B,H,W,3] -> B complete JFIF files (Y sampled 2 x 2, the Annex K
// Huffman tables, one restart interval per row of 16 x 16 MCUs), byte for byte what libjpeg's integer baseline path writes with
// its default chroma subsampling (calipsync_amd/jpeg.py encode_jpeg_host(..., subsampling="4:2:0") is the numpy twin; DESIGN.md
// section 8i).
//
// Shared with the 4:4:4 encoder (jpeg_enc.hip), in jpeg_enc_common.h: the tables, the DCT and quantisation of a block
// (transform_block), put_bits, the AC walk of a block (walk_ac), the close of a row (close_row), the bodies of the plan and pack
// kernels, the header and the host side of the three entries.  This file's own: the load of a quadrant with chroma's row padding,
// Y of a quadrant, the 2 x 2 chroma downsample and its transform in place, where a block lies in LDS (block_at), the DC words,
// dummies and block order of a lane's half MCU (walk_mcu), and the row kernel.  The second half of a chunk (prefix sum, windows,
// stuffing, carry) is the same text in both row kernels: shared, it cost device time.
//
//   jpeg420_encode_rows_kernel  one wave per MCU row of one frame.  32 MCUs at a time, two lanes each: the even lane takes the
//                             top 16 x 8 pixels, the odd lane the bottom ones (six blocks to one lane are 48 KB of LDS a wave
//                             and 1.9 times the time).  A lane takes its two 8 x 8 quadrants in turn:
//                             Y of the quadrant through the two DCT passes and the quantisation in registers into LDS
//                             (zigzag order, four coefficients to an 8-byte word), and the quadrant's 4 x 4 share of the
//                             2 x 2 averaged Cb and Cr samples into the LDS words their coefficients replace; once both
//                             halves are in, the even lane transforms Cb and the odd lane Cr.  A Y block past the frame's
//                             whole 8 x 8 blocks is a dummy: no DCT, it codes as DC difference 0 and EOB.  The six DC values
//                             of an MCU are replaced by their differences, and each lane walks three blocks (the even lane
//                             Y00, Y01, Y10, the odd lane Y11, Cb, Cr) twice (a word of zeros is four zeros of a run): once
//                             to count its code bits, and, after a wave prefix sum of the counts, once to OR the bits into
//                             an LDS bit buffer at its own offset.  A second wave pass counts the 0xFF bytes ahead of each
//                             byte (ballot + popcount) and writes the stuffed bytes to the row's slot of the scratch buffer.
//                             The partial last byte and the three DC predictors are carried from one 32-MCU chunk to the
//                             next; the row ends with its 1-bit padding and RSTn or EOI.  A chunk whose bits outgrow the bit
//                             buffer is emitted in several windows of it (every lane walks again and keeps the words of the
//                             window).  A row that outgrows its slot stops being written at the slot's end and is marked.
//   jpeg420_plan_kernel, jpeg420_pack_kernel   the shared bodies under this encoder's names, on MCU rows.
//
// The output is a pure function of the input: no global atomics, nothing that depends on scheduling, every global byte has one
// writer and plain vector stores.  LDS: 24 KB of coefficients + 8 KB of bits per wave.  No scratch.
#include "jpeg_enc_common.h"

namespace {

// The 8 x 8 pixels of one quadrant of an MCU, packed B | G << 8 | R << 16, the last column repeated past the frame's edge.  Rows
// past the edge: FOR_CHROMA false repeats the last row (Y's padding); true repeats the last PAIR of rows that holds a row of the
// frame, the second of the pair being the first again under an odd H (the last downsampled chroma row is what is repeated, and
// averaging two copies of the last row is something else).  Both are the same rows wherever y0 + 8 <= H.
template <bool FOR_CHROMA>
__device__ __forceinline__ void load_quadrant(const unsigned char* __restrict__ src, int H, int W, int y0, int x0, unsigned (&px)[64]) {
  const bool inside = x0 + 8 <= W;
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    int yy = y0 + y;
    if (FOR_CHROMA) {
      const int last_pair = (H - 1) >> 1;
      yy = 2 * ((yy >> 1) < last_pair ? (yy >> 1) : last_pair) + (yy & 1);
    }
    yy = yy < H ? yy : H - 1;
    const unsigned char* p = src + (size_t)yy * W * 3;
    if (inside && ((uintptr_t)p & 3) == 0) {                   // 24 bytes as six aligned words (x0 * 3 is a multiple of 24)
      const unsigned* pw = reinterpret_cast<const unsigned*>(p + (size_t)x0 * 3);
      unsigned w[7];
#pragma unroll
      for (int i = 0; i < 6; ++i) w[i] = pw[i];
      w[6] = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int s = 3 * c, i = s >> 2, sh = (s & 3) * 8;
        const unsigned long long two = ((unsigned long long)w[i + 1] << 32) | w[i];
        px[y * 8 + c] = (unsigned)(two >> sh) & 0xFFFFFFu;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int xx = x0 + c < W ? x0 + c : W - 1;
        const unsigned char* q = p + (size_t)xx * 3;
        px[y * 8 + c] = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
      }
    }
  }
}

// Y of the quadrant in px -> its block at `out`
__device__ __forceinline__ void transform_luma(const unsigned (&px)[64], const JpegQuant& qt, uint2* out) {
  int d[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    const int b = px[i] & 0xFF, g = (px[i] >> 8) & 0xFF, r = (px[i] >> 16) & 0xFF;
    d[i] = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) - 128;
  }
  transform_block(d, qt, 0, out);
}

// Cb and Cr of the quadrant in px, averaged 2 x 2 with libjpeg's bias (1 in even output columns, 2 in odd ones; a quadrant
// starts on an even one) and level-shifted: the quadrant's 4 x 4 samples of each, 16 bits each, as rows 4 qy .. 4 qy + 3, half
// qx, of the 8 x 8 sample image at cb / cr (word g = 2 row + half holds four samples of a row, as transform_block's output does)
__device__ __forceinline__ void downsample_chroma(const unsigned (&px)[64], int qy, int qx, uint2* cb, uint2* cr) {
#pragma unroll 1
  for (int comp = 1; comp < 3; ++comp) {
    const int kr = comp == 1 ? -11059 : 32768, kg = comp == 1 ? -21709 : -27439, kb = comp == 1 ? 32768 : -5329;
    uint2* out = (comp == 1 ? cb : cr) + (8 * qy + qx) * 64;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned s[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int sum = 1 + (i & 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned p = px[(2 * j + (k >> 1)) * 8 + 2 * i + (k & 1)];
          const int b = p & 0xFF, g = (p >> 8) & 0xFF, r = (p >> 16) & 0xFF;
          sum += (kr * r + kg * g + kb * b + (128 << 16) + 32767) >> 16;
        }
        s[i] = (unsigned)((sum >> 2) - 128) & 0xFFFFu;
      }
      out[2 * j * 64] = make_uint2(s[0] | (s[1] << 16), s[2] | (s[3] << 16));
    }
  }
}

// The 8 x 8 chroma samples downsample_chroma left at `blk` -> their coefficients, in place
__device__ __forceinline__ void transform_chroma(const JpegQuant& qt, uint2* blk) {
  int d[64];
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const uint2 four = blk[g * 64];
    d[4 * g] = (int)(short)(four.x & 0xFFFFu);
    d[4 * g + 1] = (int)(short)(four.x >> 16);
    d[4 * g + 2] = (int)(short)(four.y & 0xFFFFu);
    d[4 * g + 3] = (int)(short)(four.y >> 16);
  }
  transform_block(d, qt, 1, blk);
}

// Where block c (Y00, Y01, Y10, Y11, Cb, Cr) of the MCU of lanes `even` and `even + 1` lies in the coefficient image
// [slot][word g][lane]: the lane that transformed it holds it in its own column (the top lane the top Y blocks and Cb)
__device__ __forceinline__ int block_at(int c, int even) { return c < 4 ? (c & 1) * 16 * 64 + even + (c >> 1) : 2 * 16 * 64 + even + (c - 4); }

// The code words of the lane's half of its MCU in stream order (the even lane Y00, Y01, Y10, the odd one Y11, Cb, Cr; the DC
// position of a block holds its DC difference; bit c of `dummies`: Y block c is a dummy, difference 0 and EOB, its LDS words
// are not read); EMIT: into the bit buffer from bit `pos` on.  -> the bit after the last.
template <bool EMIT>
__device__ __forceinline__ unsigned walk_mcu(const uint2* coef, int lane, unsigned dummies, unsigned pos, unsigned* bitbuf, unsigned winbase) {
  const int first = 3 * (lane & 1), even = lane & ~1;
  auto word = [&](unsigned entry, int v, unsigned cat) {        // Huffman code of the symbol, then the low `cat` bits of v (v - 1 if negative)
    const unsigned len = (entry >> 16) + cat;
    if (EMIT) {
      const unsigned low = (unsigned)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
      put_bits(bitbuf, winbase, pos, ((entry & 0xFFFFu) << cat) | low, len);
    }
    pos += len;
  };
  for (int c = first; c < first + 3; ++c) {
    const unsigned* dc_tab = c >= 4 ? HUFF_DC_CHROMA : HUFF_DC_LUMA;
    const unsigned* ac_tab = c >= 4 ? HUFF_AC_CHROMA : HUFF_AC_LUMA;
    if ((dummies >> c) & 1u) {
      word(dc_tab[0], 0, 0);
      word(ac_tab[0], 0, 0);
      continue;
    }
    const uint2* cw = coef + block_at(c, even);
    const uint2 next = cw[0];
    const int dv = (int)(short)(next.x & 0xFFFFu);
    const unsigned dcat = 32u - __clz(dv < 0 ? -dv : dv);
    word(dc_tab[dcat], dv, dcat);
    walk_ac(cw, next, ac_tab, word);
  }
  return pos;
}

// grid (MCU rows, frames of this launch), one wave each.  row_len [frames][rows], slots [frames][rows][slot_bytes].
__global__ __launch_bounds__(64) void jpeg420_encode_rows_kernel(const unsigned char* __restrict__ frames, int frame0, int H, int W, JpegQuant qt,
                                                                 long long slot_bytes, unsigned* __restrict__ row_len,
                                                                 unsigned char* __restrict__ slots) {
  __shared__ uint2 coef[3 * 16 * 64];                           // [slot][word g][lane], see block_at
  __shared__ unsigned bitbuf[BITBUF_WORDS];
  const int lane = threadIdx.x, row = blockIdx.x, rows = gridDim.x;
  const int half = lane & 1, even = lane & ~1;                  // the lane takes the top (0) or the bottom (1) half of its MCU
  const size_t frame = (size_t)frame0 + blockIdx.y;
  const int n_mcu = (W + 15) >> 4;
  const int y_rows = (H + 7) >> 3, y_cols = (W + 7) >> 3;       // whole 8 x 8 blocks of Y: the blocks past them are dummies
  const unsigned char* src = frames + frame * H * W * 3;
  const size_t slot = frame * rows + row;
  unsigned char* dst = slots + slot * (size_t)slot_bytes;
  const unsigned cap = slot_bytes > 0x7FFFFFFFll ? 0x7FFFFFFFu : (unsigned)slot_bytes;      // a row is below 2^24 bytes
  int pred_y = 0, pred_cb = 0, pred_cr = 0;
  unsigned carry = 0, carry_n = 0;                              // the bits of the partial last byte of the chunks so far
  unsigned out_pos = 0;                                         // bytes of the row so far, whether they fitted or not

  for (int chunk = 0; chunk < n_mcu; chunk += 32) {
    const int n_active = n_mcu - chunk < 32 ? n_mcu - chunk : 32;                // MCUs: two lanes each
    const bool active = (lane >> 1) < n_active, last = chunk + 32 >= n_mcu;
    const int mcu = chunk + (lane >> 1);
    unsigned dummies = 0;                                       // bit c: Y block c (2 qy + qx) of the lane's MCU, the same in both its lanes
#pragma unroll
    for (int quad = 0; quad < 4; ++quad)
      if (2 * row + (quad >> 1) >= y_rows || 2 * mcu + (quad & 1) >= y_cols) dummies |= 1u << quad;
    if (active) {
#pragma unroll 1
      for (int qx = 0; qx < 2; ++qx) {                          // the two quadrants of the lane's half
        const int y0 = row * 16 + half * 8, x0 = mcu * 16 + qx * 8;
        const bool dummy = (dummies >> (2 * half + qx)) & 1u;
        unsigned px[64];
        if (!dummy) {
          load_quadrant<false>(src, H, W, y0, x0, px);
          transform_luma(px, qt, coef + qx * 16 * 64 + lane);
        }
        if (dummy || y0 + 8 > H) load_quadrant<true>(src, H, W, y0, x0, px);      // below the frame chroma repeats other rows than Y
        downsample_chroma(px, half, qx, coef + 2 * 16 * 64 + even, coef + 2 * 16 * 64 + even + 1);
      }
    }
    __syncthreads();                                            // both halves of the chroma samples are in
    if (active) transform_chroma(qt, coef + 2 * 16 * 64 + lane);        // the top lane Cb, the bottom lane Cr
    __syncthreads();
    {                                                           // every DC value becomes its difference, in place: both lanes of an MCU
      int dc[6], last_y = 0;                                    // read, the even one writes.  A dummy repeats the Y block before it
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const bool real = active && !(c < 4 && ((dummies >> c) & 1u));
        dc[c] = real ? (int)(short)(coef[block_at(c, even)].x & 0xFFFFu) : 0;
        if (c < 4) last_y = real ? dc[c] : last_y;              // block 0 is never a dummy
      }
      const int left_y = __shfl_up(last_y, 2), left_cb = __shfl_up(dc[4], 2), left_cr = __shfl_up(dc[5], 2);
      int before = lane < 2 ? pred_y : left_y;
      const int before_cb = lane < 2 ? pred_cb : left_cb, before_cr = lane < 2 ? pred_cr : left_cr;
      pred_y = __shfl(last_y, 2 * n_active - 1);
      pred_cb = __shfl(dc[4], 2 * n_active - 1);
      pred_cr = __shfl(dc[5], 2 * n_active - 1);
      __syncthreads();                                          // every lane has read the values
      if (active && half == 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          if (c < 4 && ((dummies >> c) & 1u)) continue;
          const int diff = dc[c] - (c < 4 ? before : c == 4 ? before_cb : before_cr);
          uint2* w = &coef[block_at(c, even)];
          w->x = (w->x & 0xFFFF0000u) | ((unsigned)diff & 0xFFFFu);
          if (c < 4) before = dc[c];
        }
      }
    }
    __syncthreads();
    const unsigned n_bits = active ? walk_mcu<false>(coef, lane, dummies, 0u, bitbuf, 0u) : 0u;
    unsigned incl = n_bits;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    const unsigned start = carry_n + incl - n_bits;
    const unsigned total = carry_n + __shfl(incl, 63);
    const unsigned pad = last ? (0u - total) & 7u : 0u;         // 1-bits up to the byte boundary at the end of the row
    const unsigned n_bytes = (total + pad) >> 3;                // whole bytes of this chunk's stream
    unsigned winbase = 0;
    for (;; winbase += BITBUF_WORDS) {
      for (int i = lane; i < BITBUF_WORDS; i += 64) bitbuf[i] = 0u;
      __syncthreads();
      if (lane == 0 && carry_n) put_bits(bitbuf, winbase, 0u, carry, carry_n);
      if (active) walk_mcu<true>(coef, lane, dummies, start, bitbuf, winbase);
      if (lane == 0 && pad) put_bits(bitbuf, winbase, total, (1u << pad) - 1u, pad);
      __syncthreads();
      const unsigned lo = winbase * 4u;
      const unsigned hi = n_bytes < lo + BITBUF_WORDS * 4u ? n_bytes : lo + BITBUF_WORDS * 4u;
      for (unsigned base = lo; base < hi; base += 64u) {        // byte stuffing: every 0xFF is followed by 0x00
        const unsigned i = base + lane;
        const bool valid = i < hi;
        const unsigned b = valid ? (bitbuf[(i >> 2) - winbase] >> (24u - 8u * (i & 3u))) & 0xFFu : 0u;
        const unsigned long long ff = __ballot(b == 0xFFu);
        const unsigned at = out_pos + (i - base) + (unsigned)__popcll(ff & ((1ull << lane) - 1ull));
        if (valid && at < cap) dst[at] = (unsigned char)b;
        if (b == 0xFFu && at + 1u < cap) dst[at + 1u] = 0;
        out_pos += (hi - base < 64u ? hi - base : 64u) + (unsigned)__popcll(ff);
      }
      if ((winbase + BITBUF_WORDS) * 32u >= total + pad) break;
    }
    carry_n = total & 7u;                                       // 0 after the padded last chunk
    if (!last && carry_n) {
      const unsigned i = total >> 3;                            // its word lies in the last window
      carry = ((bitbuf[(i >> 2) - winbase] >> (24u - 8u * (i & 3u))) & 0xFFu) >> (8u - carry_n);
    }
    if (last) carry_n = 0;
    __syncthreads();                                            // the next chunk overwrites both buffers
  }
  if (lane == 0) close_row(dst, cap, out_pos, row, rows, row_len + slot);
}

__global__ __launch_bounds__(256) void jpeg420_plan_kernel(const unsigned* __restrict__ row_len, int batch, int rows, long long out_cap,
                                                           long long* __restrict__ offsets, int* __restrict__ status) {
  jpeg_plan_body(row_len, batch, rows, out_cap, offsets, status);
}

__global__ __launch_bounds__(256) void jpeg420_pack_kernel(const unsigned* __restrict__ row_len, const unsigned char* __restrict__ slots, int frame0,
                                                           long long slot_bytes, JpegHeader header, const long long* __restrict__ offsets,
                                                           const int* __restrict__ status, unsigned char* __restrict__ out) {
  jpeg_pack_body(row_len, slots, frame0, slot_bytes, header, offsets, status, out);
}

const JpegVariant VARIANT = {"jpeg420", 16, 6, jpeg420_encode_rows_kernel, jpeg420_plan_kernel, jpeg420_pack_kernel};

}  // namespace

extern "C" {

int casync_op_jpeg420_header(int H, int W, int quality, uint8_t* out, int cap) { return jpeg_header_entry(VARIANT, H, W, quality, out, cap); }

int64_t casync_op_jpeg420_workspace_bytes(int batch, int H, int W, int64_t slot_bytes) { return jpeg_workspace_entry(VARIANT, batch, H, W, slot_bytes); }

int casync_op_jpeg420_encode(const uint8_t* frames_bgr, int batch, int H, int W, int quality, int64_t slot_bytes, uint8_t* scratch,
                             int64_t scratch_bytes, uint8_t* out, int64_t out_cap, int64_t* offsets, int32_t* status, casync_stream stream) {
  return jpeg_encode_entry(VARIANT, frames_bgr, batch, H, W, quality, slot_bytes, scratch, scratch_bytes, out, out_cap, offsets, status, stream);
}

}  // extern "C"
