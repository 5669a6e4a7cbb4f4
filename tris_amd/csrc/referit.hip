// ReferIt evaluation (validate_referit.py, dataset/Dataset_referit.py): the K sentences of one image share its size, so their
// targets are decoded from run lengths and their response maps are scored in launches whose number does not depend on K.
//
// (a) tris_rle_decode_sum_u8: dataset/Dataset_referit.py:141-144 -- cocomask.decode + sum over the segments + astype(uint8).
//     One lane per ROW-MAJOR output pixel: a wave stores 64 consecutive bytes, and reads the run boundaries of a segment by
//     binary search (the boundaries of one segment are a few hundred int32: they stay in cache, and a search is <= ~10 steps).
//     The other mapping -- lanes along a column, where neighbouring lanes share a run, transposed through LDS to the row-major
//     output -- saves searches but pays a tile transpose and a barrier for a mask that is read once; DESIGN section 17.
// (b) tris_eval_post_group_f32: validate_referit.py:160-171 for K maps -- the expressions of eval.hip (signed = 0) and of
//     seg.hip's signed evaluation (signed = 1), with the sentence on blockIdx.y.  Maxima, first arg-maxima and integer counts
//     do not depend on the order they are reduced in, so the records and cams equal the single entries bit for bit.  No atomics:
//     every pass leaves per-block partials and a one-block-per-sentence pass folds them.
#include "common.h"
#include "tris_hip.h"
#include "bilinear.h"

namespace {

constexpr int kMaxBlocks = 1024;                 // blocks per sentence, as the single-sentence entries
constexpr int kWsFloats = 6 * kMaxBlocks + 8;    // per sentence: [0, 2048) max partials | [2048] max | [2049] arg-max | [2056 ..) counts

inline int blocks_of(long n) {
  long nb = (n + 255) / 256;
  return (int)(nb > kMaxBlocks ? kMaxBlocks : nb);
}

// ---------------------------------------------------------------------------------------------------------------- (a)
// ends: inclusive prefix sums of every segment's counts (column-major position where each run ends); seg_off[s] .. seg_off[s+1]
// the slice of segment s; ranges[k] = {first segment, one past the last} of sentence k.
__global__ __launch_bounds__(256) void rle_decode_sum_kernel(const int* __restrict__ ends, const long* __restrict__ seg_off,
                                                             const int* __restrict__ ranges, int H, int W,
                                                             unsigned char* __restrict__ out) {
  const int k = blockIdx.y;
  const int s0 = ranges[2 * k], s1 = ranges[2 * k + 1];
  const long n = (long)H * W;
  unsigned char* o = out + (long)k * n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int y = (int)(i / W), x = (int)(i % W);
    const int p = x * H + y;                                  // column-major position (H*W <= 2^24)
    int c = 0;
    for (int s = s0; s < s1; ++s) {
      const int* e = ends + seg_off[s];
      const int nr = (int)(seg_off[s + 1] - seg_off[s]);
      int lo = 0, hi = nr;                                    // first run whose end lies beyond p = the run that holds p
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= p) lo = mid + 1; else hi = mid;
      }
      c += (lo < nr && (lo & 1)) ? 1 : 0;                     // odd runs are foreground; past the last run: background
    }
    o[i] = (unsigned char)c;
  }
}

// ---------------------------------------------------------------------------------------------------------------- (b)
// pass 1: per-block (max, first arg-max) of the raw resized map
__global__ __launch_bounds__(256) void group_max_kernel(const float* __restrict__ maps, int S, int oH, int oW, float* __restrict__ ws_all) {
  __shared__ float sv[256];
  __shared__ int si[256];
  const float* m = maps + (long)blockIdx.y * S * S;
  float* ws = ws_all + (long)blockIdx.y * kWsFloats;
  const long n = (long)oH * oW;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float v = sample_ac(m, S, oH, oW, (int)(i / oW), (int)(i % oW));
    if (v > best) { best = v; bi = (int)i; }
  }
  sv[threadIdx.x] = best;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      float ov = sv[threadIdx.x + o];
      int oi = si[threadIdx.x + o];
      if (ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < si[threadIdx.x])) { sv[threadIdx.x] = ov; si[threadIdx.x] = oi; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { ws[2 * blockIdx.x] = sv[0]; ws[2 * blockIdx.x + 1] = __int_as_float(si[0]); }
}
// pass 2: one block per sentence folds the partials
__device__ __forceinline__ void fold_best(float* sv, int* si, float& best, int& bi) {   // 256 threads -> thread 0 holds the result
  sv[threadIdx.x] = best;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      const float ov = sv[threadIdx.x + o];
      const int oi = si[threadIdx.x + o];
      if (ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < si[threadIdx.x])) { sv[threadIdx.x] = ov; si[threadIdx.x] = oi; }
    }
    __syncthreads();
  }
  best = sv[0];
  bi = si[0];
}
__global__ __launch_bounds__(256) void group_max_final_kernel(float* __restrict__ ws_all, int nb) {
  __shared__ float sv[256];
  __shared__ int si[256];
  float* ws = ws_all + (long)blockIdx.x * kWsFloats;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int b = threadIdx.x; b < nb; b += 256) {
    float v = ws[2 * b];
    int i = __float_as_int(ws[2 * b + 1]);
    if (v > best || (v == best && i < bi)) { best = v; bi = i; }
  }
  fold_best(sv, si, best, bi);
  if (threadIdx.x == 0) {
    ws[2 * kMaxBlocks] = best;
    ws[2 * kMaxBlocks + 1] = __int_as_float(bi);
  }
}
// pass 3: normalise, threshold, count; per-block {I, U, best normalised value, its first index}
__global__ __launch_bounds__(256) void group_count_kernel(const float* __restrict__ maps, int S, const unsigned char* __restrict__ targets,
                                                          int oH, int oW, float* __restrict__ cams, float* __restrict__ ws_all) {
  __shared__ int ri[256], ru[256], bi[256];
  __shared__ float bv[256];
  const long n = (long)oH * oW;
  const float* m = maps + (long)blockIdx.y * S * S;
  const unsigned char* target = targets + (long)blockIdx.y * n;
  float* cam = cams ? cams + (long)blockIdx.y * n : nullptr;
  float* ws = ws_all + (long)blockIdx.y * kWsFloats;
  const float denom = ws[2 * kMaxBlocks] + 1e-5f;
  int I = 0, U = 0, besti = 0x7fffffff;
  float best = -INFINITY;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = sample_ac(m, S, oH, oW, (int)(i / oW), (int)(i % oW)) / denom;
    if (cam) cam[i] = v;
    const bool p = v > 1e-9f, t = target[i] != 0;
    I += (p && t) ? 1 : 0;
    U += (p || t) ? 1 : 0;
    if (v > best) { best = v; besti = (int)i; }
  }
  ri[threadIdx.x] = I; ru[threadIdx.x] = U; bv[threadIdx.x] = best; bi[threadIdx.x] = besti;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      const int j = threadIdx.x + o;
      ri[threadIdx.x] += ri[j];
      ru[threadIdx.x] += ru[j];
      if (bv[j] > bv[threadIdx.x] || (bv[j] == bv[threadIdx.x] && bi[j] < bi[threadIdx.x])) { bv[threadIdx.x] = bv[j]; bi[threadIdx.x] = bi[j]; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float* o = ws + 2 * kMaxBlocks + 8 + 4 * blockIdx.x;
    o[0] = __int_as_float(ri[0]);
    o[1] = __int_as_float(ru[0]);
    o[2] = bv[0];
    o[3] = __int_as_float(bi[0]);
  }
}
// pass 4: one block per sentence -> the record.  signed = 0: the arg-max of the raw map (tris_eval_post_f32);
// signed = 1: the first arg-max of the normalised map, index 0 for an all-NaN map (tris_eval_post_signed_f32)
__global__ __launch_bounds__(256) void group_final_kernel(const float* __restrict__ ws_all, int nb, const unsigned char* __restrict__ targets, long n,
                                   int is_signed, long* __restrict__ records) {
  __shared__ float sv[256];
  __shared__ int si[256];
  __shared__ long sI[256], sU[256];
  const float* ws = ws_all + (long)blockIdx.x * kWsFloats;
  long I = 0, U = 0;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int b = threadIdx.x; b < nb; b += 256) {
    const float* o = ws + 2 * kMaxBlocks + 8 + 4 * b;
    I += __float_as_int(o[0]);
    U += __float_as_int(o[1]);
    const int i = __float_as_int(o[3]);
    if (o[2] > best || (o[2] == best && i < bi)) { best = o[2]; bi = i; }
  }
  sI[threadIdx.x] = I;
  sU[threadIdx.x] = U;
  fold_best(sv, si, best, bi);                  // (its barriers also publish sI / sU)
  if (threadIdx.x != 0) return;
  I = 0;
  U = 0;
  for (int t = 0; t < 256; ++t) { I += sI[t]; U += sU[t]; }
  if (is_signed) { if (bi == 0x7fffffff) bi = 0; }
  else bi = __float_as_int(ws[2 * kMaxBlocks + 1]);
  long* r = records + 4 * (long)blockIdx.x;
  r[0] = I;
  r[1] = U;
  r[2] = bi;
  r[3] = (bi >= 0 && (long)bi < n) ? (long)targets[(long)blockIdx.x * n + bi] : 0;
}

}  // namespace

extern "C" int tris_rle_decode_sum_u8(const int* ends, const long* seg_off, const int* ranges, int K, int H, int W,
                                      unsigned char* out, void* stream) {
  if (K < 0 || H < 1 || W < 1 || (long)H * W > (1L << 24)) return (int)hipErrorInvalidValue;
  if (K == 0) return 0;
  if (K > 65535 || ranges == nullptr || seg_off == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rle_decode_sum_kernel, dim3(blocks_of((long)H * W), K), dim3(256), 0, (hipStream_t)stream, ends, seg_off,
                     ranges, H, W, out);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" long tris_eval_post_group_workspace_bytes(int K) { return K < 0 ? -1 : (long)K * kWsFloats * (long)sizeof(float); }

extern "C" int tris_eval_post_group_f32(const float* maps, int S, const unsigned char* targets, int K, int oH, int oW, float* cams,
                                        long* records, int is_signed, float* workspace, void* stream) {
  const long n = (long)oH * oW;
  if (K < 0 || S < 1 || oH < 1 || oW < 1 || n > 0x7fffffffL) return (int)hipErrorInvalidValue;
  if (K == 0) return 0;
  if (K > 65535 || maps == nullptr || targets == nullptr || records == nullptr || workspace == nullptr) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int nb = blocks_of(n);
  hipLaunchKernelGGL(group_max_kernel, dim3(nb, K), dim3(256), 0, st, maps, S, oH, oW, workspace);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(group_max_final_kernel, dim3(K), dim3(256), 0, st, workspace, nb);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(group_count_kernel, dim3(nb, K), dim3(256), 0, st, maps, S, targets, oH, oW, cams, workspace);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(group_final_kernel, dim3(K), dim3(256), 0, st, (const float*)workspace, nb, targets, n, is_signed, records);
  TRIS_LAUNCH_CHECK();
  return 0;
}
