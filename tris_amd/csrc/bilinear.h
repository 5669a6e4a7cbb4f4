// Bilinear source-index arithmetic shared by every resize of the library: the NCHW resize and the response maps
// (heads.hip), the evaluation post-processing (eval.hip) and the channels-last decoder upsample (seg.hip).  One copy of
// the expressions, so the layouts agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// PyTorch source-index conventions (upsample_bilinear2d): align_corners=False: src = (dst+0.5)*in/out-0.5 clamped
// at 0; True: src = dst*(in-1)/(out-1).
struct Lerp { int i0, i1; float w1; };
__device__ __forceinline__ Lerp lerp_of(int dst, int in, int out, int align) {
  float src;
  if (align) {
    float sc = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
    src = sc * (float)dst;
  } else {
    float sc = (float)in / (float)out;
    src = sc * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
  }
  Lerp l;
  l.i0 = (int)src;
  if (l.i0 > in - 1) l.i0 = in - 1;
  l.i1 = l.i0 + (l.i0 < in - 1 ? 1 : 0);
  l.w1 = src - (float)l.i0;
  return l;
}
// The align_corners=False position of lerp_of as the exact rational (in (2 dst + 1) - out) / (2 out), clamped at 0: the index by integer
// division, each weight by ONE float division of its own numerator (w0 is not 1 - w1), so both carry a RELATIVE error of 2^-24 however
// small they are.  lerp_of's float position is off by a few ulps of the POSITION, an absolute error in the weight that an element-wise
// bound in terms of sum_k w_k |v_k| cannot absorb (csrc/attnpool.hip: the positional grid of AttentionPool2d).  Same indices as lerp_of
// wherever the float position does not round across an integer.  in, out <= 2^14.
struct LerpQ { int i0, i1; float w0, w1; };
__device__ __forceinline__ LerpQ lerp_exact_of(int dst, int in, int out) {
  int num = in * (2 * dst + 1) - out;
  const int den = 2 * out;
  if (num < 0) num = 0;
  LerpQ l;
  l.i0 = num / den;
  const int r = num - l.i0 * den;
  if (l.i0 > in - 1) l.i0 = in - 1;
  l.i1 = l.i0 + (l.i0 < in - 1 ? 1 : 0);
  l.w1 = (float)r / (float)den;
  l.w0 = (float)(den - r) / (float)den;
  return l;
}
// weight with which input index `y` contributes to output index `dst`
__device__ __forceinline__ float contrib(int dst, int in, int out, int align, int y) {
  Lerp l = lerp_of(dst, in, out, align);
  float w = 0.f;
  if (l.i0 == y) w += 1.0f - l.w1;
  if (l.i1 == y) w += l.w1;
  return w;
}
// conservative output window [lo, hi] that can reference input index y
__device__ __forceinline__ void window(int y, int in, int out, int align, int& lo, int& hi) {
  if (in == 1) { lo = 0; hi = out - 1; return; }
  float a, b;
  if (align) {
    float inv = out > 1 ? (float)(out - 1) / (float)(in - 1) : 0.f;
    a = ((float)y - 1.f) * inv;
    b = ((float)y + 1.f) * inv;
  } else {
    float r = (float)out / (float)in;
    a = ((float)y - 0.5f) * r - 0.5f;
    b = ((float)y + 1.5f) * r - 0.5f;
  }
  lo = (int)floorf(a) - 1;
  hi = (int)ceilf(b) + 1;
  if (y == 0 || lo < 0) lo = 0;
  if (y == in - 1 || hi > out - 1) hi = out - 1;
}

// align_corners=True sample of an SxS map at output pixel (oy, ox) of an oH x oW grid (validate.py:180)
__device__ __forceinline__ float sample_ac(const float* __restrict__ m, int S, int oH, int oW, int oy, int ox) {
  float sy = oH > 1 ? (float)(S - 1) / (float)(oH - 1) : 0.f, sx = oW > 1 ? (float)(S - 1) / (float)(oW - 1) : 0.f;
  float fy = sy * (float)oy, fx = sx * (float)ox;
  int y0 = min((int)fy, S - 1), x0 = min((int)fx, S - 1);
  int y1 = y0 + (y0 < S - 1 ? 1 : 0), x1 = x0 + (x0 < S - 1 ? 1 : 0);
  float wy = fy - (float)y0, wx = fx - (float)x0;
  float v00 = m[y0 * S + x0], v01 = m[y0 * S + x1], v10 = m[y1 * S + x0], v11 = m[y1 * S + x1];
  float top = v00 + wx * (v01 - v00), bot = v10 + wx * (v11 - v10);
  return top + wy * (bot - top);
}
// The same expressions for an Sh x Sw map (overlay.hip), with contraction off: the source position stays a float32 product of its
// own, so position and weight are exactly the float32 values F.interpolate defines and the weight's subtraction is exact.  Fused
// into that subtraction (what the compiler does by default), the product would move the weight by up to half an ulp of the POSITION.
__device__ __forceinline__ float sample_ac_rect(const float* __restrict__ m, int Sh, int Sw, int oH, int oW, int oy, int ox) {
#pragma clang fp contract(off)
  float sy = oH > 1 ? (float)(Sh - 1) / (float)(oH - 1) : 0.f, sx = oW > 1 ? (float)(Sw - 1) / (float)(oW - 1) : 0.f;
  float fy = sy * (float)oy, fx = sx * (float)ox;
  int y0 = min((int)fy, Sh - 1), x0 = min((int)fx, Sw - 1);
  int y1 = y0 + (y0 < Sh - 1 ? 1 : 0), x1 = x0 + (x0 < Sw - 1 ? 1 : 0);
  float wy = fy - (float)y0, wx = fx - (float)x0;
  float v00 = m[y0 * Sw + x0], v01 = m[y0 * Sw + x1], v10 = m[y1 * Sw + x0], v11 = m[y1 * Sw + x1];
  float top = v00 + wx * (v01 - v00), bot = v10 + wx * (v11 - v10);
  return top + wy * (bot - top);
}

}  // namespace
