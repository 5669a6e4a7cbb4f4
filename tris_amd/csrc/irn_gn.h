// What the IRNet network kernels (irnnet.hip) and their backward (irntrain.hip) share: 16-byte accesses, the element-wise grid, and
// the fixed row-block layout of the GroupNorm sums -- one copy, so that forward and backward partition an image the same way.
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

inline int ew_grid(long n) {
  long g = (n + 255) / 256;
  return (int)(g < 8192 ? (g < 1 ? 1 : g) : 8192);
}

constexpr int GN_BLOCKS = 256;   // row blocks per image at most (fixed for a shape: the sums are reproducible)

inline int gn_blocks(long HW) {
  long nb = (HW + 63) / 64;
  return (int)(nb < GN_BLOCKS ? (nb < 1 ? 1 : nb) : GN_BLOCKS);
}

inline bool gn_shape_ok(int C, int G) {
  return C >= 4 && C <= 1024 && C % 4 == 0 && 256 % (C / 4) == 0 && G >= 1 && G <= 256 && C % G == 0 && (C / G) % 4 == 0;
}

}  // namespace
