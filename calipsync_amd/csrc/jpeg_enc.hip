// Baseline JPEG of finished frames on the device: uint8 BGR [B,H,W,3] -> B complete JFIF files (4:4:4, the Annex K Huffman
// tables, one restart interval per row of 8 x 8 blocks), byte for byte what libjpeg's integer baseline path writes
// (calipsync_amd/jpeg.py encode_jpeg_host is the numpy twin).
//
// Shared with the 4:2:0 encoder (jpeg_enc420.hip), in jpeg_enc_common.h: the tables, the DCT and quantisation of a block
// (transform_block), put_bits, the AC walk of a block (walk_ac), the close of a row (close_row), the bodies of the plan and pack
// kernels, the header and the host side of the three entries.  This file's own: the load of an MCU's 8 x 8 pixels, the colour
// conversion of a component, the DC words and block order of an MCU (walk_mcu) and the row kernel.  The second half of a chunk
// (prefix sum, windows, stuffing, carry) is the same text in both row kernels: shared, it cost device time.
//
//   jpeg_encode_rows_kernel   one wave per block row of one frame.  64 MCUs at a time, one per lane: the lane converts its 8 x 8
//                             pixels to Y, Cb, Cr, runs the two DCT passes and the quantisation in registers and leaves the
//                             coefficients in LDS in zigzag order, four to an 8-byte word.  It then walks them twice (a word
//                             of zeros is four zeros of a run): once to count its code bits, and, after a wave prefix sum of
//                             the counts, once to OR the bits into an LDS bit buffer at its own offset.  A second wave pass
//                             counts the 0xFF bytes ahead of each byte (ballot + popcount) and writes the stuffed bytes to
//                             the row's slot of the scratch buffer.  The partial last byte and the
//                             three DC predictors are carried from one 64-MCU chunk to the next; the row ends with its 1-bit
//                             padding and RSTn or EOI.  A chunk whose bits outgrow the bit buffer (128 bytes per MCU) is emitted in
//                             several windows of it (every lane walks again and keeps the words of the window).  A row that
//                             outgrows its slot stops being written at the slot's end and is marked.
//   jpeg_plan_kernel          one workgroup: per frame 629 + the sum of its row lengths, its status (1: a row outgrew its slot,
//                             2: it would pass out_cap), and the exclusive prefix over the frames -> offsets [B+1].
//   jpeg_pack_kernel          one workgroup per block row of a frame with status 0: the prefix of the row lengths ahead of it,
//                             then a copy of the slot's bytes (and, for row 0, of the header) to their place in `out`.
//
// The output is a pure function of the input: no global atomics, nothing that depends on scheduling, every global byte has one
// writer and plain vector stores.  LDS: 24 KB of coefficients + 8 KB of bits per wave.  No scratch.
#include "jpeg_enc_common.h"

namespace {

// The 8 x 8 pixels of one MCU, packed B | G << 8 | R << 16, the last column and row repeated past the frame's edge.
__device__ __forceinline__ void load_mcu(const unsigned char* __restrict__ src, int H, int W, int y0, int x0, unsigned (&px)[64]) {
  const bool inside = x0 + 8 <= W;
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    const int yy = y0 + y < H ? y0 + y : H - 1;
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

// Component comp (0 Y, 1 Cb, 2 Cr) of the MCU in px: colour, level shift, then transform_block into coef[(comp*16 + g)*64 + lane].
// comp is a run-time value on purpose: one copy of the code, one block of 64 values live.
__device__ __forceinline__ void transform_component(const unsigned (&px)[64], const JpegQuant& qt, int comp, uint2* coef, int lane) {
  const int cr = comp == 0 ? 19595 : comp == 1 ? -11059 : 32768;
  const int cg = comp == 0 ? 38470 : comp == 1 ? -21709 : -27439;
  const int cb = comp == 0 ? 7471 : comp == 1 ? 32768 : -5329;
  const int add = comp == 0 ? 32768 : (128 << 16) + 32767;
  int d[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    const int b = px[i] & 0xFF, g = (px[i] >> 8) & 0xFF, r = (px[i] >> 16) & 0xFF;
    d[i] = ((cr * r + cg * g + cb * b + add) >> 16) - 128;
  }
  transform_block(d, qt, comp ? 1 : 0, coef + comp * 16 * 64 + lane);
}

// The code words of the lane's MCU in stream order; EMIT: into the bit buffer from bit `pos` on.  -> the bit after the last.
template <bool EMIT>
__device__ __forceinline__ unsigned walk_mcu(const uint2* coef, int lane, const int (&diff)[3], unsigned pos, unsigned* bitbuf, unsigned winbase) {
  auto word = [&](unsigned entry, int v, unsigned cat) {        // Huffman code of the symbol, then the low `cat` bits of v (v - 1 if negative)
    const unsigned len = (entry >> 16) + cat;
    if (EMIT) {
      const unsigned low = (unsigned)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
      put_bits(bitbuf, winbase, pos, ((entry & 0xFFFFu) << cat) | low, len);
    }
    pos += len;
  };
  for (int c = 0; c < 3; ++c) {
    const unsigned* dc_tab = c ? HUFF_DC_CHROMA : HUFF_DC_LUMA;
    const unsigned* ac_tab = c ? HUFF_AC_CHROMA : HUFF_AC_LUMA;
    const int dv = diff[c];
    const unsigned dcat = 32u - __clz(dv < 0 ? -dv : dv);
    word(dc_tab[dcat], dv, dcat);
    const uint2* cw = coef + c * 16 * 64 + lane;
    walk_ac(cw, cw[0], ac_tab, word);
  }
  return pos;
}

// grid (block rows, frames of this launch), one wave each.  row_len [frames][rows], slots [frames][rows][slot_bytes].
__global__ __launch_bounds__(64) void jpeg_encode_rows_kernel(const unsigned char* __restrict__ frames, int frame0, int H, int W, JpegQuant qt,
                                                              long long slot_bytes, unsigned* __restrict__ row_len,
                                                              unsigned char* __restrict__ slots) {
  __shared__ uint2 coef[3 * 16 * 64];
  __shared__ unsigned bitbuf[BITBUF_WORDS];
  const int lane = threadIdx.x, row = blockIdx.x, rows = gridDim.x;
  const size_t frame = (size_t)frame0 + blockIdx.y;
  const int n_mcu = (W + 7) >> 3;
  const unsigned char* src = frames + frame * H * W * 3;
  const size_t slot = frame * rows + row;
  unsigned char* dst = slots + slot * (size_t)slot_bytes;
  const unsigned cap = slot_bytes > 0x7FFFFFFFll ? 0x7FFFFFFFu : (unsigned)slot_bytes;      // a row is below 2^24 bytes
  int pred[3] = {0, 0, 0};
  unsigned carry = 0, carry_n = 0;                              // the bits of the partial last byte of the chunks so far
  unsigned out_pos = 0;                                         // bytes of the row so far, whether they fitted or not

  for (int chunk = 0; chunk < n_mcu; chunk += 64) {
    const int n_active = n_mcu - chunk < 64 ? n_mcu - chunk : 64;
    const bool active = lane < n_active, last = chunk + 64 >= n_mcu;
    if (active) {
      unsigned px[64];
      load_mcu(src, H, W, row * 8, (chunk + lane) * 8, px);
#pragma unroll 1
      for (int comp = 0; comp < 3; ++comp) transform_component(px, qt, comp, coef, lane);
    }
    __syncthreads();
    int diff[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int dc = active ? (int)(short)(coef[(c * 16) * 64 + lane].x & 0xFFFFu) : 0;
      const int left = __shfl_up(dc, 1);
      diff[c] = dc - (lane == 0 ? pred[c] : left);
      pred[c] = __shfl(dc, n_active - 1);
    }
    const unsigned n_bits = active ? walk_mcu<false>(coef, lane, diff, 0u, bitbuf, 0u) : 0u;
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
      if (active) walk_mcu<true>(coef, lane, diff, start, bitbuf, winbase);
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

__global__ __launch_bounds__(256) void jpeg_plan_kernel(const unsigned* __restrict__ row_len, int batch, int rows, long long out_cap,
                                                        long long* __restrict__ offsets, int* __restrict__ status) {
  jpeg_plan_body(row_len, batch, rows, out_cap, offsets, status);
}

__global__ __launch_bounds__(256) void jpeg_pack_kernel(const unsigned* __restrict__ row_len, const unsigned char* __restrict__ slots, int frame0,
                                                        long long slot_bytes, JpegHeader header, const long long* __restrict__ offsets,
                                                        const int* __restrict__ status, unsigned char* __restrict__ out) {
  jpeg_pack_body(row_len, slots, frame0, slot_bytes, header, offsets, status, out);
}

const JpegVariant VARIANT = {"jpeg", 8, 3, jpeg_encode_rows_kernel, jpeg_plan_kernel, jpeg_pack_kernel};

}  // namespace

extern "C" {

int casync_op_jpeg_header(int H, int W, int quality, uint8_t* out, int cap) { return jpeg_header_entry(VARIANT, H, W, quality, out, cap); }

int64_t casync_op_jpeg_workspace_bytes(int batch, int H, int W, int64_t slot_bytes) { return jpeg_workspace_entry(VARIANT, batch, H, W, slot_bytes); }

int casync_op_jpeg_encode(const uint8_t* frames_bgr, int batch, int H, int W, int quality, int64_t slot_bytes, uint8_t* scratch,
                          int64_t scratch_bytes, uint8_t* out, int64_t out_cap, int64_t* offsets, int32_t* status, casync_stream stream) {
  return jpeg_encode_entry(VARIANT, frames_bgr, batch, H, W, quality, slot_bytes, scratch, scratch_bytes, out, out_cap, offsets, status, stream);
}

}  // extern "C"
