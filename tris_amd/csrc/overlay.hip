// Heat-map presentation of the K response maps of ONE image (demo.py:28-48, 94-96): bilinear resize (align_corners=True) to
// the picture's size, clamp at 0, min-max normalise over the OUTPUT grid, quantise to 8 bits by truncation, colour table,
// 0.6 / 0.4 blend with the picture -- uint8 out.  Two launches whatever K is: a range pass that leaves per-block
// (min, max, first arg-max) partials, and a paint pass whose blocks fold the <= 256 partials of their sentence themselves.
// min / max / first-arg-max do not depend on the order they are folded in and no pixel reads another sentence's data, so a
// sentence's outputs are bit-identical whatever K it shares the call with.  The source maps are read through the cache (a
// Stage-2 map is size x size and does not fit LDS); the 768-byte colour table sits in LDS.
#include "common.h"
#include "tris_hip.h"
#include "bilinear.h"

namespace {

constexpr int PAINT_NB = 256;                     // range-pass blocks per sentence at most (= paint-pass threads per block)
constexpr long PAINT_WS_PER_K = PAINT_NB * 16;    // bytes: float min[256] | float max[256] | long arg[256]

struct Range { float lo, hi; long arg; };

__device__ __forceinline__ void fold(Range& a, float lo, float hi, long arg) {
  a.lo = fminf(a.lo, lo);
  if (hi > a.hi || (hi == a.hi && arg < a.arg)) { a.hi = hi; a.arg = arg; }
}
// block-wide fold (blockDim.x == 256); every thread gets the result
__device__ __forceinline__ Range block_fold(Range r, float* slo, float* shi, long* sarg) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    float lo = __shfl_xor(r.lo, o, 64), hi = __shfl_xor(r.hi, o, 64);
    long arg = __shfl_xor((long long)r.arg, o, 64);
    fold(r, lo, hi, arg);
  }
  if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = r.lo; shi[threadIdx.x >> 6] = r.hi; sarg[threadIdx.x >> 6] = r.arg; }
  __syncthreads();
  Range t = {slo[0], shi[0], sarg[0]};
#pragma unroll
  for (int w = 1; w < 4; ++w) fold(t, slo[w], shi[w], sarg[w]);
  return t;
}

// pass 1: grid (nb, K).  u = max(sample, 0) over the H x W grid of sentence blockIdx.y -> partials of this block
__global__ __launch_bounds__(256) void paint_range_kernel(const float* __restrict__ maps, int Sh, int Sw, int H, int W,
                                                          float* __restrict__ ws) {
  __shared__ float slo[4], shi[4];
  __shared__ long sarg[4];
  const int k = blockIdx.y;
  const float* m = maps + (long)k * Sh * Sw;
  const long n = (long)H * W;
  Range r = {INFINITY, -INFINITY, 0x7fffffffffffffffL};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float u = fmaxf(sample_ac_rect(m, Sh, Sw, H, W, (int)(i / W), (int)(i % W)), 0.f);
    r.lo = fminf(r.lo, u);
    if (u > r.hi) { r.hi = u; r.arg = i; }      // ascending i: the first of equal maxima stays
  }
  r = block_fold(r, slo, shi, sarg);
  if (threadIdx.x == 0) {
    char* base = (char*)ws + (long)k * PAINT_WS_PER_K;
    ((float*)base)[blockIdx.x] = r.lo;
    ((float*)base)[PAINT_NB + blockIdx.x] = r.hi;
    ((long*)(base + PAINT_NB * 8))[blockIdx.x] = r.arg;
  }
}

struct alignas(4) Bytes12 { unsigned a, b, c; };

__device__ __forceinline__ unsigned pack4(const unsigned char* b) {
  return (unsigned)b[0] | ((unsigned)b[1] << 8) | ((unsigned)b[2] << 16) | ((unsigned)b[3] << 24);
}

// pass 2: grid (bx, K).  A thread owns groups of 4 pixels = 12 heat bytes, cut on the FLAT pixel index of the [K][H][W] output so
// that every whole group is 4-byte (heat) and 16-byte (norm) aligned whatever H * W is; the at most two groups a sentence shares
// with its neighbours are written per byte, each side its own pixels.
__global__ __launch_bounds__(256) void paint_kernel(const float* __restrict__ maps, int Sh, int Sw,
                                                    const unsigned char* __restrict__ image, int H, int W,
                                                    const unsigned char* __restrict__ lut, int mode, int nb,
                                                    unsigned char* __restrict__ heat, float* __restrict__ norm,
                                                    float* __restrict__ range, long* __restrict__ argmax,
                                                    const float* __restrict__ ws) {
  __shared__ float slo[4], shi[4];
  __shared__ long sarg[4];
  __shared__ unsigned char slut[768];
  const int k = blockIdx.y;
  for (int i = threadIdx.x; i < 768; i += 256) slut[i] = lut[i];
  const char* base = (const char*)ws + (long)k * PAINT_WS_PER_K;
  Range r = {INFINITY, -INFINITY, 0x7fffffffffffffffL};
  if ((int)threadIdx.x < nb) {
    r.lo = ((const float*)base)[threadIdx.x];
    r.hi = ((const float*)base)[PAINT_NB + threadIdx.x];
    r.arg = ((const long*)(base + PAINT_NB * 8))[threadIdx.x];
  }
  r = block_fold(r, slo, shi, sarg);              // (its barrier also publishes slut)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    range[2 * k] = r.lo;
    range[2 * k + 1] = r.hi;
    argmax[k] = r.arg;
  }
  const float lo = r.lo, denom = r.hi - r.lo + 1e-5f;
  const float* m = maps + (long)k * Sh * Sw;
  const long n = (long)H * W, first = (long)k * n, last = first + n;          // flat pixel range of this sentence
  const long g0 = first >> 2, g1 = (last + 3) >> 2;
  for (long g = g0 + (long)blockIdx.x * 256 + threadIdx.x; g < g1; g += (long)gridDim.x * 256) {
    const long p0 = g << 2;
    const bool whole = p0 >= first && p0 + 4 <= last;
    long q = (p0 > first ? p0 : first) - first;                                // first pixel of the group inside the sentence
    int y = (int)(q / W), x = (int)(q - (long)y * W);
    unsigned char px[12], im[12];
    float nv[4];
    const bool im_vec = whole && image && (((uintptr_t)(image + 3 * q)) & 3) == 0;
    if (im_vec) {
      Bytes12 v = *(const Bytes12*)(image + 3 * q);
      unsigned w3[3] = {v.a, v.b, v.c};
#pragma unroll
      for (int j = 0; j < 12; ++j) im[j] = (unsigned char)(w3[j >> 2] >> (8 * (j & 3)));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long p = p0 + j;
      const bool in = p >= first && p < last;
      if (in) {
        float u = fmaxf(sample_ac_rect(m, Sh, Sw, H, W, y, x), 0.f);
        float t = mode == TRIS_PAINT_UNIT ? fminf(u, 1.f) : (u - lo) / denom;
        int idx = (int)(t * 255.f);
        idx = idx < 0 ? 0 : (idx > 255 ? 255 : idx);
        nv[j] = t;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          unsigned col = slut[3 * idx + c];
          if (image) {
            unsigned pic = im_vec ? im[3 * j + c] : image[3 * (p - first) + c];
            col = (3u * col + 2u * pic + 2u) / 5u;
          }
          px[3 * j + c] = (unsigned char)col;
        }
        if (++x == W) { x = 0; ++y; }
      }
    }
    if (whole) {
      Bytes12 o = {pack4(px), pack4(px + 4), pack4(px + 8)};
      *(Bytes12*)(heat + 3 * p0) = o;
      if (norm) *(float4*)(norm + p0) = make_float4(nv[0], nv[1], nv[2], nv[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long p = p0 + j;
        if (p >= first && p < last) {
          heat[3 * p] = px[3 * j];
          heat[3 * p + 1] = px[3 * j + 1];
          heat[3 * p + 2] = px[3 * j + 2];
          if (norm) norm[p] = nv[j];
        }
      }
    }
  }
}

}  // namespace

extern "C" long tris_cam_paint_workspace_bytes(int K, int H, int W) {
  if (K < 0 || H < 1 || W < 1) return -1;
  return (long)K * PAINT_WS_PER_K;
}

extern "C" int tris_cam_paint_f32(const float* maps, int K, int Sh, int Sw, const unsigned char* image, int H, int W,
                                  const unsigned char* lut, int mode, unsigned char* heat, float* norm, float* range,
                                  long* argmax, void* workspace, void* stream) {
  if (K < 0 || K > 65535 || Sh < 1 || Sw < 1 || H < 1 || W < 1 || (mode != TRIS_PAINT_MINMAX && mode != TRIS_PAINT_UNIT))
    return (int)hipErrorInvalidValue;
  if (K == 0) return 0;
  if (!maps || !lut || !heat || !range || !argmax || !workspace || ((uintptr_t)heat & 3) || ((uintptr_t)norm & 15) ||
      ((uintptr_t)workspace & 7))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const long n = (long)H * W;
  long nbl = (n + 1023) / 1024;                   // >= 4 pixels per thread before a second block is worth its partial
  const int nb = (int)(nbl > PAINT_NB ? PAINT_NB : nbl);
  hipLaunchKernelGGL(paint_range_kernel, dim3(nb, K), dim3(256), 0, st, maps, Sh, Sw, H, W, (float*)workspace);
  TRIS_LAUNCH_CHECK();
  long gb = (n / 4 + 2 + 255) / 256;              // groups of a sentence, the two shared ones included
  const int bx = (int)(gb > 128 ? 128 : gb);      // x K sentences; larger pictures stride (480 x 640: three groups a thread)
  hipLaunchKernelGGL(paint_kernel, dim3(bx, K), dim3(256), 0, st, maps, Sh, Sw, image, H, W, lut, mode, nb, heat, norm, range,
                     argmax, (const float*)workspace);
  TRIS_LAUNCH_CHECK();
  return 0;
}
