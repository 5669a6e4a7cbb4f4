// Scoring of the Stage-1 -> Stage-2 artefacts against REFER ground truth that stays run ends (tris_amd/pseudo_eval.py; DESIGN
// section 21): response maps (validate.py:183-190 over a whole threshold sweep), CRF labels (IRNet/step_refer/cam_to_ir_label.py:72-76)
// and instance masks (IRNet/step_refer/make_ins_seg_labels.py:160-163).  No full-size target is formed: the ground-truth bit of a
// pixel is read from the (ends, seg_off) arena of dataset/rle_arena.py, as referit.hip's decoder reads it.
//
// (a) tris_score_maps_f32: G maps of one size, one ref each.  Per pixel: bin = the number of thresholds below the value (a search
//     in the ascending list; strict, float32), bit = ground truth; LDS integer adds into the workgroup's [T+1][2] counters.
// (b) tris_score_counts_u8: a uint8 stack [K,H,W], one ref.  Per pixel: the byte sum over K, the bit, LDS adds into [256][2].
// (c) tris_score_planes_u8: the same stack and ref, optionally on the grid of source pixels a NEAREST resize reads.  Per sample: the
//     integer sum over K (no wrap), which planes are set, the bit; LDS adds into [K+3][2]: sum 0 / 1 / above, then a row per plane.
// All: every workgroup writes its counters as one partial row, a second launch sums the rows of a map in block order into int64.
// Integer sums do not depend on the order anyway; there are no global atomics and the result is the same bytes on every run.
//
// The map is row-major and the arena column-major (p = x*H + y).  A workgroup takes tiles of 64 columns x 64 rows: a lane owns a
// column, a wave 16 rows of it, so a wave reads 256 contiguous bytes of a map row, and a lane's positions p0 .. p0+15 are
// consecutive in the arena: one binary search per segment finds the run that holds p0 (the search of referit.hip's decoder) and
// the run index then only moves forward down the column ((c) on a sampled grid: the positions x*H + yidx[..] do not decrease but are
// not consecutive, and its walk takes them as they are).  Of a pixel's segment count only "at least one" and "at least two" are
// kept, one bit per row each.  A ref whose runs (all its segments together) fit kStage words is staged in LDS once per workgroup;
// a longer one is searched in global memory.  The walk is the same function on either pointer.
#include "common.h"
#include "tris_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64;               // columns of a tile: one per lane
constexpr int kRows = 16;                // rows a lane walks down its column
constexpr int kTileH = kRows * (kThreads / 64);
constexpr int kMaxBlocks = 256;          // partial rows per map; a workgroup strides over the tiles beyond
constexpr int kStage = 4096;             // run ends of one ref held in LDS (16 KiB)
constexpr int kMaxSeg = 255;             // segments per ref (the decoded sum is a byte, dataset/rle_arena.py)
constexpr int kMaxThr = 64;
constexpr int kCountBins = 256;
constexpr int kMaxPlanes = 255;          // planes of one stack (their sum is Stage 2's byte target)

inline long tiles_of(int H, int W) { return (long)((H + kTileH - 1) / kTileH) * ((W + kTileW - 1) / kTileW); }
inline int blocks_of(int H, int W) {
  const long t = tiles_of(H, W);
  return (int)(t > kMaxBlocks ? kMaxBlocks : t);
}

// the runs of segments s0 .. s1-1 into LDS when they fit: s_off[j] = start of segment s0 + j inside s_ends, j = 0 .. s1 - s0.
// The answer is the same for every thread of the workgroup.  The caller places the barrier.
__device__ __forceinline__ bool stage_ref(const int* __restrict__ ends, const long* __restrict__ seg_off, int s0, int s1, int* s_ends,
                                          int* s_off) {
  const long base = seg_off[s0];
  const long total = seg_off[s1] - base;
  if (total > kStage) return false;
  for (int j = threadIdx.x; j <= s1 - s0; j += kThreads) s_off[j] = (int)(seg_off[s0 + j] - base);
  for (int i = threadIdx.x; i < (int)total; i += kThreads) s_ends[i] = ends[base + i];
  return true;
}

// One segment over the positions p0 .. p0 + rows - 1: bit k of `any` is set where at least one segment so far covers p0 + k, of
// `multi` where at least two do.  The run that holds p0 is the first whose end lies beyond it (the search of referit.hip's
// rle_decode_sum_kernel, restated: there it is written into the kernel's loop); further down the column the index only grows.
// Odd runs are foreground; past the last run: background.
__device__ __forceinline__ void walk_segment(const int* e, int nr, int p0, int rows, unsigned& any, unsigned& multi) {
  int lo = 0, hi = nr;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= p0) lo = mid + 1; else hi = mid;
  }
  for (int k = 0; k < rows && lo < nr; ++k) {
    while (lo < nr && e[lo] <= p0 + k) ++lo;
    const unsigned f = (lo < nr && (lo & 1)) ? (1u << k) : 0u;
    multi |= any & f;
    any |= f;
  }
}

// ground-truth bits of the rows p0 .. p0 + rows - 1 of one column.  gt_rule 0: covered by exactly one segment
// (ReferDataset.load_mask); 1: covered at all (validate's target != 0)
__device__ __forceinline__ unsigned column_bits(bool staged, const int* s_ends, const int* s_off, const int* __restrict__ ends,
                                                const long* __restrict__ seg_off, int s0, int s1, int p0, int rows, int gt_rule) {
  unsigned any = 0, multi = 0;
  if (staged) {
    for (int s = 0; s < s1 - s0; ++s) walk_segment(s_ends + s_off[s], s_off[s + 1] - s_off[s], p0, rows, any, multi);
  } else {
    for (int s = s0; s < s1; ++s) walk_segment(ends + seg_off[s], (int)(seg_off[s + 1] - seg_off[s]), p0, rows, any, multi);
  }
  return gt_rule ? any : (any & ~multi);
}

// a lane's place in tile t: its column x, first row y0 and the number of rows it owns there (0: nothing)
__device__ __forceinline__ int tile_place(int t, int H, int W, int& x, int& y0) {
  const int tiles_x = (W + kTileW - 1) / kTileW;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  x = tx * kTileW + (threadIdx.x & 63);
  y0 = ty * kTileH + (threadIdx.x >> 6) * kRows;
  if (x >= W || y0 >= H) return 0;
  return H - y0 < kRows ? H - y0 : kRows;
}

// equal keys of consecutive rows are added once: a lane holds (key, count) and hands it to LDS when the key changes
__device__ __forceinline__ void add_key(int* s_h, int key, int& cur, int& cnt) {
  if (key == cur) { ++cnt; return; }
  if (cnt) atomicAdd(&s_h[cur], cnt);            // LDS integer add
  cur = key;
  cnt = 1;
}

// ---------------------------------------------------------------------------------------------------------------- (a)
__global__ __launch_bounds__(kThreads) void score_maps_kernel(const float* __restrict__ maps, const int* __restrict__ ends,
                                                              const long* __restrict__ seg_off, const int* __restrict__ ranges,
                                                              const float* __restrict__ thresholds, int T, int H, int W, int tiles,
                                                              int gt_rule, int* __restrict__ partial) {
  __shared__ int s_ends[kStage];
  __shared__ int s_off[kMaxSeg + 1];
  __shared__ float s_thr[kMaxThr];
  __shared__ int s_h[2 * (kMaxThr + 1)];
  const int g = blockIdx.y;
  const int s0 = ranges[2 * g], s1 = ranges[2 * g + 1];
  const int width = 2 * (T + 1);
  for (int j = threadIdx.x; j < width; j += kThreads) s_h[j] = 0;
  for (int j = threadIdx.x; j < T; j += kThreads) s_thr[j] = thresholds[j];
  const bool staged = stage_ref(ends, seg_off, s0, s1, s_ends, s_off);
  __syncthreads();
  const float* m = maps + (long)g * H * W;
  int cur = 0, cnt = 0;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    int x, y0;
    const int rows = tile_place(t, H, W, x, y0);
    if (rows == 0) continue;
    float v[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) v[k] = k < rows ? m[(y0 + k) * W + x] : 0.f;      // (H*W <= 2^24: the index is an int)
    const unsigned bits = column_bits(staged, s_ends, s_off, ends, seg_off, s0, s1, x * H + y0, rows, gt_rule);
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      if (k < rows) {
        int lo = 0, hi = T;                                   // thresholds ascend: v > t holds for a prefix (none for a NaN)
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (v[k] > s_thr[mid]) lo = mid + 1; else hi = mid;
        }
        add_key(s_h, 2 * lo + (int)((bits >> k) & 1u), cur, cnt);
      }
    }
  }
  if (cnt) atomicAdd(&s_h[cur], cnt);
  __syncthreads();
  int* row = partial + ((long)g * gridDim.x + blockIdx.x) * width;
  for (int j = threadIdx.x; j < width; j += kThreads) row[j] = s_h[j];
}

// ---------------------------------------------------------------------------------------------------------------- (b)
__global__ __launch_bounds__(kThreads) void score_counts_kernel(const unsigned char* __restrict__ stack, int K,
                                                                const int* __restrict__ ends, const long* __restrict__ seg_off, int s0,
                                                                int s1, int H, int W, int tiles, int gt_rule, int* __restrict__ partial) {
  __shared__ int s_ends[kStage];
  __shared__ int s_off[kMaxSeg + 1];
  __shared__ int s_h[2 * kCountBins];
  const long n = (long)H * W;
  for (int j = threadIdx.x; j < 2 * kCountBins; j += kThreads) s_h[j] = 0;
  const bool staged = stage_ref(ends, seg_off, s0, s1, s_ends, s_off);
  __syncthreads();
  int cur = 0, cnt = 0;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    int x, y0;
    const int rows = tile_place(t, H, W, x, y0);
    if (rows == 0) continue;
    const unsigned bits = column_bits(staged, s_ends, s_off, ends, seg_off, s0, s1, x * H + y0, rows, gt_rule);
    for (int k = 0; k < rows; ++k) {
      const unsigned char* px = stack + (y0 + k) * W + x;
      unsigned sum = 0;
      for (int j = 0; j < K; ++j) sum += px[j * n];
      add_key(s_h, 2 * (int)(sum & 255u) + (int)((bits >> k) & 1u), cur, cnt);       // a byte sum, as numpy's uint8 accumulator
    }
  }
  if (cnt) atomicAdd(&s_h[cur], cnt);
  __syncthreads();
  int* row = partial + (long)blockIdx.x * (2 * kCountBins);
  for (int j = threadIdx.x; j < 2 * kCountBins; j += kThreads) row[j] = s_h[j];
}

// ---------------------------------------------------------------------------------------------------------------- (c)
// One segment over the positions base + ys[k], k < rows, of one source column: walk_segment for positions that are not consecutive.
// Entries of ys below 0 are skipped (their bits stay 0); the others do not decrease down the column (the host's duty: a table that
// did would give wrong bits, never a read outside the runs).  The search runs at the first position that counts.
__device__ __forceinline__ void walk_segment_at(const int* e, int nr, int base, const int (&ys)[kRows], int rows, unsigned& any,
                                                unsigned& multi) {
  int lo = -1;
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    if (k < rows && ys[k] >= 0 && lo < nr) {
      const int p = base + ys[k];
      if (lo < 0) {
        int hi = nr;
        lo = 0;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (e[mid] <= p) lo = mid + 1; else hi = mid;
        }
      } else {
        while (lo < nr && e[lo] <= p) ++lo;
      }
      const unsigned f = (lo < nr && (lo & 1)) ? (1u << k) : 0u;
      multi |= any & f;
      any |= f;
    }
  }
}

__device__ __forceinline__ unsigned column_bits_at(bool staged, const int* s_ends, const int* s_off, const int* __restrict__ ends,
                                                   const long* __restrict__ seg_off, int s0, int s1, int base, const int (&ys)[kRows],
                                                   int rows, int gt_rule) {
  unsigned any = 0, multi = 0;
  if (staged) {
    for (int s = 0; s < s1 - s0; ++s) walk_segment_at(s_ends + s_off[s], s_off[s + 1] - s_off[s], base, ys, rows, any, multi);
  } else {
    for (int s = s0; s < s1; ++s) walk_segment_at(ends + seg_off[s], (int)(seg_off[s + 1] - seg_off[s]), base, ys, rows, any, multi);
  }
  return gt_rule ? any : (any & ~multi);
}

// tiles of the output grid [Hout][Wout]; sample (y, x) is source pixel (yidx[y], xidx[x]), or (y, x) itself without tables.  A
// sample whose index lies outside the canvas has every plane 0 and bit 0.  Counters [K + 3][2]: rows 0 .. 2 the integer sum over
// the planes (0, 1, 2 and above), row 3 + j the samples where plane j is not 0.  A lane goes plane by plane down its 16 rows, so a
// plane costs it two LDS adds per tile, and keeps the 16 sums in registers.
__global__ __launch_bounds__(kThreads) void score_planes_kernel(const unsigned char* __restrict__ stack, int K,
                                                                const int* __restrict__ ends, const long* __restrict__ seg_off, int s0,
                                                                int s1, int H, int W, const int* __restrict__ yidx,
                                                                const int* __restrict__ xidx, int Hout, int Wout, int tiles, int gt_rule,
                                                                int* __restrict__ partial) {
  __shared__ int s_ends[kStage];
  __shared__ int s_off[kMaxSeg + 1];
  __shared__ int s_h[2 * (kMaxPlanes + 3)];
  const size_t n = (size_t)H * W;
  const int width = 2 * (K + 3);
  for (int j = threadIdx.x; j < width; j += kThreads) s_h[j] = 0;
  const bool staged = stage_ref(ends, seg_off, s0, s1, s_ends, s_off);
  __syncthreads();
  int cur = 0, cnt = 0;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    int x, y0;
    const int rows = tile_place(t, Hout, Wout, x, y0);
    if (rows == 0) continue;
    int xs = xidx ? xidx[x] : x;
    if ((unsigned)xs >= (unsigned)W) xs = -1;
    int ys[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      int v = -1;
      if (k < rows && xs >= 0) {
        v = yidx ? yidx[y0 + k] : y0 + k;
        if ((unsigned)v >= (unsigned)H) v = -1;
      }
      ys[k] = v;
    }
    const unsigned bits = xs < 0 ? 0u : column_bits_at(staged, s_ends, s_off, ends, seg_off, s0, s1, xs * H, ys, rows, gt_rule);
    unsigned sum[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) sum[k] = 0;
    for (int j = 0; j < K; ++j) {
      const unsigned char* plane = stack + (size_t)j * n;         // (64 bits: 255 planes of 2^24 pixels)
      unsigned on = 0;
#pragma unroll
      for (int k = 0; k < kRows; ++k) {
        const unsigned b = ys[k] >= 0 ? plane[ys[k] * W + xs] : 0u;          // (H*W <= 2^24: the index is an int)
        sum[k] += b;
        on |= b ? (1u << k) : 0u;
      }
      const int c1 = __popc(on & bits), c0 = __popc(on & ~bits);
      if (c0) atomicAdd(&s_h[2 * (3 + j)], c0);              // LDS integer adds
      if (c1) atomicAdd(&s_h[2 * (3 + j) + 1], c1);
    }
#pragma unroll
    for (int k = 0; k < kRows; ++k)
      if (k < rows) add_key(s_h, 2 * (int)(sum[k] < 2u ? sum[k] : 2u) + (int)((bits >> k) & 1u), cur, cnt);
  }
  if (cnt) atomicAdd(&s_h[cur], cnt);
  __syncthreads();
  int* row = partial + (long)blockIdx.x * width;
  for (int j = threadIdx.x; j < width; j += kThreads) row[j] = s_h[j];
}

// second launch of all three: one workgroup per map sums its nb partial rows, block 0 first, into int64
__global__ __launch_bounds__(kThreads) void score_fold_kernel(const int* __restrict__ partial, int nb, int width, long* __restrict__ hist) {
  const int* rows = partial + (long)blockIdx.x * nb * width;
  for (int j = threadIdx.x; j < width; j += kThreads) {
    long s = 0;
    for (int b = 0; b < nb; ++b) s += rows[(long)b * width + j];
    hist[(long)blockIdx.x * width + j] = s;
  }
}

inline bool bad_canvas(int H, int W) { return H < 1 || W < 1 || (long)H * W > (1L << 24); }

}  // namespace

extern "C" int tris_score_stage_capacity(void) { return kStage; }

extern "C" long tris_score_workspace_bytes(int G, int H, int W, int bins) {
  if (G < 0 || bad_canvas(H, W) || bins < 1 || bins > kCountBins) return -1;
  return (long)G * blocks_of(H, W) * 2 * bins * (long)sizeof(int);
}

extern "C" int tris_score_maps_f32(const float* maps, const int* ends, const long* seg_off, const int* ranges, int G, int H, int W,
                                   const float* thresholds, int T, int gt_rule, long* hist, void* workspace, void* stream) {
  if (G < 0 || bad_canvas(H, W) || T < 1 || T > kMaxThr || (gt_rule != 0 && gt_rule != 1)) return (int)hipErrorInvalidValue;
  if (G == 0) return 0;
  if (G > 65535 || maps == nullptr || ends == nullptr || seg_off == nullptr || ranges == nullptr || thresholds == nullptr ||
      hist == nullptr || workspace == nullptr)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int nb = blocks_of(H, W);
  hipLaunchKernelGGL(score_maps_kernel, dim3(nb, G), dim3(kThreads), 0, st, maps, ends, seg_off, ranges, thresholds, T, H, W,
                     (int)tiles_of(H, W), gt_rule, (int*)workspace);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(score_fold_kernel, dim3(G), dim3(kThreads), 0, st, (const int*)workspace, nb, 2 * (T + 1), hist);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_score_counts_u8(const unsigned char* stack, int K, const int* ends, const long* seg_off, int seg_lo, int seg_hi,
                                    int H, int W, int gt_rule, long* hist, void* workspace, void* stream) {
  if (bad_canvas(H, W) || K < 0 || K > 255 || seg_lo < 0 || seg_hi < seg_lo || seg_hi - seg_lo > kMaxSeg ||
      (gt_rule != 0 && gt_rule != 1))
    return (int)hipErrorInvalidValue;
  if ((K > 0 && stack == nullptr) || ends == nullptr || seg_off == nullptr || hist == nullptr || workspace == nullptr)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int nb = blocks_of(H, W);
  hipLaunchKernelGGL(score_counts_kernel, dim3(nb), dim3(kThreads), 0, st, stack, K, ends, seg_off, seg_lo, seg_hi, H, W,
                     (int)tiles_of(H, W), gt_rule, (int*)workspace);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(score_fold_kernel, dim3(1), dim3(kThreads), 0, st, (const int*)workspace, nb, 2 * kCountBins, hist);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" long tris_score_planes_workspace_bytes(int K, int Hout, int Wout) {
  if (K < 0 || K > kMaxPlanes || bad_canvas(Hout, Wout)) return -1;
  return (long)blocks_of(Hout, Wout) * 2 * (K + 3) * (long)sizeof(int);
}

extern "C" int tris_score_planes_u8(const unsigned char* stack, int K, const int* ends, const long* seg_off, int seg_lo, int seg_hi,
                                    int H, int W, const int* yidx, const int* xidx, int Hout, int Wout, int gt_rule, long* table,
                                    void* workspace, void* stream) {
  if (bad_canvas(H, W) || bad_canvas(Hout, Wout) || K < 0 || K > kMaxPlanes || seg_lo < 0 || seg_hi < seg_lo ||
      seg_hi - seg_lo > kMaxSeg || (gt_rule != 0 && gt_rule != 1))
    return (int)hipErrorInvalidValue;
  if ((yidx == nullptr) != (xidx == nullptr) || (yidx == nullptr && (Hout != H || Wout != W))) return (int)hipErrorInvalidValue;
  if ((K > 0 && stack == nullptr) || ends == nullptr || seg_off == nullptr || table == nullptr || workspace == nullptr)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int nb = blocks_of(Hout, Wout);
  hipLaunchKernelGGL(score_planes_kernel, dim3(nb), dim3(kThreads), 0, st, stack, K, ends, seg_off, seg_lo, seg_hi, H, W, yidx, xidx,
                     Hout, Wout, (int)tiles_of(Hout, Wout), gt_rule, (int*)workspace);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(score_fold_kernel, dim3(1), dim3(kThreads), 0, st, (const int*)workspace, nb, 2 * (K + 3), table);
  TRIS_LAUNCH_CHECK();
  return 0;
}
