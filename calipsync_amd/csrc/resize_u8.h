// The 8-bit cv::resize INTER_LINEAR of OpenCV 4.x (resize.cpp: the fixed-point path, with its switch to INTER_AREA at an exact 2x
// decimation), one destination sample at a time: what the frame kernels (frame_ops.hip) and the trainer's batch kernel
// (train_ops.hip) both restate.  oracle/frame_ops_oracle.py resize_linear_u8 is the same arithmetic on the CPU.  Everything sits in
// the anonymous namespace: the two objects stay independent translation units, each with its own copy of these inlined bodies.
//
// Floating point that must round like the host's: a file that includes this switches contraction off first
// (#pragma clang fp contract(off) at its head).
#pragma once
#include "common.h"

namespace {

// ---- cv::resize INTER_LINEAR tables, one destination index at a time (resize.cpp) ----
struct Tap { int s0, s1; float f; };
__device__ __forceinline__ Tap linear_tap_x(int d, int src, int dst) {
  const double inv_scale = (double)dst / (double)src, scale = 1.0 / inv_scale;
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= src - 1) { f = 0.f; s = src - 1; }
  return Tap{s, s + 1 < src ? s + 1 : src - 1, f};     // weight of s1 is 0 wherever s + 1 leaves the row
}
__device__ __forceinline__ Tap linear_tap_y(int d, int src, int dst) {   // rows are clipped, weights kept
  const double inv_scale = (double)dst / (double)src, scale = 1.0 / inv_scale;
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  const int s = (int)floorf(f);
  f -= (float)s;
  const int y0 = s < 0 ? 0 : (s > src - 1 ? src - 1 : s);
  const int y1 = s + 1 < 0 ? 0 : (s + 1 > src - 1 ? src - 1 : s + 1);
  return Tap{y0, y1, f};
}
__device__ __forceinline__ int coef(float c) { return __float2int_rn(c * 2048.f); }   // saturate_cast<short>(c * 2048): cvRound

// 8-bit bilinear sample of destination pixel (dy, dx), channel c, of a (sh x sw) -> (dh x dw) resize.
// fetch(y, x, c) returns the source byte.
template <class F>
__device__ __forceinline__ unsigned char resize_u8_at(F fetch, int sh, int sw, int dh, int dw, int dy, int dx, int c) {
  if (sh == dh && sw == dw) return fetch(dy, dx, c);
  if (sw == 2 * dw && sh == 2 * dh)   // exact 2x decimation: cv::resize switches INTER_LINEAR to INTER_AREA
    return (unsigned char)((fetch(2 * dy, 2 * dx, c) + fetch(2 * dy, 2 * dx + 1, c) + fetch(2 * dy + 1, 2 * dx, c) +
                            fetch(2 * dy + 1, 2 * dx + 1, c) + 2) >> 2);
  const Tap tx = linear_tap_x(dx, sw, dw), ty = linear_tap_y(dy, sh, dh);
  const int a0 = coef(1.f - tx.f), a1 = coef(tx.f), b0 = coef(1.f - ty.f), b1 = coef(ty.f);
  const int h0 = fetch(ty.s0, tx.s0, c) * a0 + fetch(ty.s0, tx.s1, c) * a1;     // HResizeLinear (int, unshifted)
  const int h1 = fetch(ty.s1, tx.s0, c) * a0 + fetch(ty.s1, tx.s1, c) * a1;
  const int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;   // VResizeLinear 8u fixed point
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

}  // namespace
