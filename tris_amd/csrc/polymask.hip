// REFER segmentation targets from polygons (dataset/refer.py:279-291 getMask, dataset/ReferDataset.py load_mask): the producer of
// the run-length arena that referit.hip decodes.  DESIGN section 19.
//
// cocomask._poly_to_counts (maskApi.c rleFrPoly) walks every edge of the x5 upsampled polygon with n = max(dx, dy) integer steps,
// keeps the steps at which the walk enters another pixel column, sorts the column-major positions of those crossings and takes
// differences.  The point of step d depends on d alone, so every pair of consecutive steps is examined by a thread of its own:
//
//   (a) tris_poly_count_runs: one workgroup per polygon, threads strided over (edge, step) -> kept crossings + 1 (the closing H*W).
//   (b) tris_poly_emit_runs:  the same walk; a kept crossing takes the next free slot of the polygon's slice (an LDS counter), the
//       slice is sorted ascending -- in LDS up to kSortCap ends, in place in global memory beyond -- and H*W closes it.  The sort
//       is a bitonic network whose comparators all put the minimum at the lower index: a comparator that reaches past the end of
//       the slice is dropped (the missing element stands for +inf), so any length is sorted, and the order in which the crossings
//       took their slots does not show in the result.
//   (c) tris_rle_target_nearest_u8: a ref's training target straight from its runs, at the positions Pillow's NEAREST resize reads.
//
// Only the rounded point of a step, int(ys + s*t + 0.5), needs floating point: three separate IEEE double operations in numpy's
// order, no contraction.  Everything else is the integer form of cocomask.py:44-52 (dataset/poly_arena.py: runs_numpy).
//
// What the host has checked (dataset/poly_arena.py) and the kernels rely on: |coordinate| <= 2^20, H*W <= 2^24, poly_off
// non-decreasing, seg_off the exclusive scan of n_runs.
#include "common.h"
#include "tris_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kEdgeChunk = 256;   // edges whose step counts are scanned at once
constexpr int kSortCap = 4096;    // run ends of one polygon sorted in LDS; longer slices are sorted in global memory

struct EdgeLds {
  int xs[kEdgeChunk], ys[kEdgeChunk];   // start of the walk (after cocomask's flip)
  int n[kEdgeChunk];                    // steps
  int form[kEdgeChunk];                 // bit 0: flipped (t = n - d), bit 1: x is the stepping axis (dx >= dy)
  double s[kEdgeChunk];                 // slope of the other axis
  int scan[kEdgeChunk];                 // inclusive scan of n
};

// the point (u, v) of step d of edge e (cocomask.py:29-40)
__device__ __forceinline__ int2 step_point(const EdgeLds& E, int e, int d) {
#pragma clang fp contract(off)
  const int form = E.form[e];
  const bool xmajor = (form & 2) != 0;
  const int t = (form & 1) ? E.n[e] - d : d;
  const int xs = E.xs[e], ys = E.ys[e];
  const double st = E.s[e] * (double)t;
  const int stepped = t + (xmajor ? xs : ys);
  const int rounded = (int)(((double)(xmajor ? ys : xs) + st) + 0.5);
  return xmajor ? make_int2(stepped, rounded) : make_int2(rounded, stepped);
}

// steps (d - 1, d) of edge e: the run boundary it leaves, or -1 (cocomask.py:44-52 in integers)
__device__ __forceinline__ int step_crossing(const EdgeLds& E, int e, int d, int h, int w) {
  const int2 p0 = step_point(E, e, d - 1), p1 = step_point(E, e, d);
  const int u0 = p0.x, v0 = p0.y, u1 = p1.x, v1 = p1.y;
  if (u1 == u0) return -1;
  const int xk = u1 < u0 ? u1 : u1 - 1;
  if (xk < 2 || (xk - 2) % 5 != 0) return -1;
  const int xc = (xk - 2) / 5;
  if (xc > w - 1) return -1;
  const int vk = v1 < v0 ? v1 : v0;
  int yc = vk <= 2 ? 0 : (vk + 2) / 5;              // ceil((vk - 2) / 5)
  if (yc > h) yc = h;
  return xc * h + yc;
}

// all comparators ascending; a[i] for i >= n stands for +inf.  Every thread of the block calls it.
template <typename T>
__device__ __forceinline__ void sort_ascending(T* a, int n) {
  int m = 1;
  while (m < n) m <<= 1;
  const int half = m >> 1;
  for (int k = 2; k <= m; k <<= 1) {
    for (int c = threadIdx.x; c < half; c += kThreads) {          // mirror step of the merge of two sorted halves
      const int l = (c / (k >> 1)) * k + (c % (k >> 1));
      const int r = l ^ (k - 1);
      if (r < n) {
        const int x = a[l], y = a[r];
        if (x > y) { a[l] = y; a[r] = x; }
      }
    }
    __syncthreads();
    for (int j = k >> 2; j >= 1; j >>= 1) {
      for (int c = threadIdx.x; c < half; c += kThreads) {
        const int l = (c / j) * 2 * j + (c % j);
        const int r = l + j;
        if (r < n) {
          const int x = a[l], y = a[r];
          if (x > y) { a[l] = y; a[r] = x; }
        }
      }
      __syncthreads();
    }
  }
}

// EMIT = 0: n_runs[p] = kept crossings + 1.  EMIT = 1: the sorted run ends of polygon p into ends[seg_off[p] .. seg_off[p + 1]).
// A polygon without vertices is a segment the host fills (an RLE annotation, coordinates beyond the bound): it is left alone.
template <int EMIT>
__global__ __launch_bounds__(kThreads) void poly_runs_kernel(const int* __restrict__ verts, const long* __restrict__ poly_off,
                                                             const int* __restrict__ hw, const long* __restrict__ seg_off,
                                                             int* __restrict__ n_runs, int* ends) {
  __shared__ EdgeLds E;
  __shared__ int red[4];
  __shared__ int slots;
  __shared__ int buf[EMIT ? kSortCap : 1];
  const int p = blockIdx.x, tid = threadIdx.x;
  const long v0 = poly_off[p];
  const int nv = (int)(poly_off[p + 1] - v0);
  if (nv <= 0) {
    if (!EMIT && tid == 0) n_runs[p] = 1;
    return;
  }
  const int h = hw[2 * p], w = hw[2 * p + 1];
  int cap = 0;                       // EMIT: slots of the slice ahead of the closing H*W
  int* dst = nullptr;
  bool in_lds = false;
  if (EMIT) {
    const long len = seg_off[p + 1] - seg_off[p];
    if (len < 1) return;
    cap = (int)(len - 1);
    in_lds = len <= kSortCap;
    dst = ends + seg_off[p];
    if (tid == 0) slots = 0;
  }
  int kept = 0;
  const int* pv = verts + 2 * v0;
  for (int e0 = 0; e0 < nv; e0 += kEdgeChunk) {
    __syncthreads();                 // (the previous chunk has been read; `slots` is set)
    {
      const int e = e0 + tid;
      int n = 0;
      if (e < nv) {
        const int e1 = e + 1 == nv ? 0 : e + 1;
        int xs = pv[2 * e], ys = pv[2 * e + 1], xe = pv[2 * e1], ye = pv[2 * e1 + 1];
        const int dx = xe > xs ? xe - xs : xs - xe, dy = ye > ys ? ye - ys : ys - ye;
        const bool xmajor = dx >= dy;
        const bool flip = xmajor ? xs > xe : ys > ye;
        if (flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
        n = xmajor ? dx : dy;
        E.xs[tid] = xs;
        E.ys[tid] = ys;
        E.form[tid] = (flip ? 1 : 0) | (xmajor ? 2 : 0);
        E.s[tid] = n == 0 ? 0.0 : (xmajor ? (double)(ye - ys) / (double)dx : (double)(xe - xs) / (double)dy);
      }
      E.n[tid] = n;
      E.scan[tid] = n;
    }
    __syncthreads();
    for (int o = 1; o < kEdgeChunk; o <<= 1) {
      const int add = tid >= o ? E.scan[tid - o] : 0;
      __syncthreads();
      E.scan[tid] += add;
      __syncthreads();
    }
    const int total = E.scan[kEdgeChunk - 1];     // <= 256 * 2^21
    for (int i = tid; i < total; i += kThreads) {
      int lo = 0, hi = kEdgeChunk - 1;            // the edge that holds step i: first e with scan[e] > i
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (E.scan[mid] <= i) lo = mid + 1; else hi = mid;
      }
      const int d = i - (E.scan[lo] - E.n[lo]) + 1;
      const int a = step_crossing(E, lo, d, h, w);
      if (a >= 0) {
        if (EMIT) {
          const int slot = atomicAdd(&slots, 1);
          if (slot < cap) {
            if (in_lds) buf[slot] = a; else dst[slot] = a;
          }
        } else {
          ++kept;
        }
      }
    }
  }
  if (!EMIT) {
    kept = block_isum_256(kept, red);
    if (tid == 0) n_runs[p] = kept + 1;
    return;
  }
  __syncthreads();
  const int len = cap + 1;
  if (tid == 0) {
    if (in_lds) buf[cap] = h * w; else dst[cap] = h * w;
  }
  __syncthreads();
  if (in_lds) {
    sort_ascending(buf, len);
    for (int i = tid; i < len; i += kThreads) dst[i] = buf[i];
  } else {
    sort_ascending(dst, len);
  }
}

// ---------------------------------------------------------------------------------------------------------------- (c)
__global__ __launch_bounds__(256) void rle_target_nearest_kernel(const int* __restrict__ ends, const long* __restrict__ seg_off, int s0,
                                                                 int s1, int H, const int* __restrict__ yidx,
                                                                 const int* __restrict__ xidx, int Hout, int Wout,
                                                                 unsigned char* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Hout * Wout) return;
  const int ys = yidx[i / Wout], xs = xidx[i % Wout];
  int c = 0;
  if (ys >= 0 && xs >= 0) {
    const int p = xs * H + ys;                                // column-major position (H*W <= 2^24)
    for (int s = s0; s < s1; ++s) {
      const int* e = ends + seg_off[s];
      const int nr = (int)(seg_off[s + 1] - seg_off[s]);
      int lo = 0, hi = nr;                                    // as rle_decode_sum_kernel (referit.hip)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= p) lo = mid + 1; else hi = mid;
      }
      c += (lo < nr && (lo & 1)) ? 1 : 0;
    }
  }
  out[i] = c == 1 ? 1 : 0;
}

}  // namespace

extern "C" int tris_poly_sort_capacity(void) { return kSortCap; }

extern "C" int tris_poly_count_runs(const int* verts, const long* poly_off, const int* hw, int P, int* n_runs, void* stream) {
  if (P < 0) return (int)hipErrorInvalidValue;
  if (P == 0) return 0;
  if (poly_off == nullptr || hw == nullptr || n_runs == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(poly_runs_kernel<0>, dim3(P), dim3(kThreads), 0, (hipStream_t)stream, verts, poly_off, hw, (const long*)nullptr,
                     n_runs, (int*)nullptr);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_poly_emit_runs(const int* verts, const long* poly_off, const int* hw, const long* seg_off, int P, int* ends,
                                   void* stream) {
  if (P < 0) return (int)hipErrorInvalidValue;
  if (P == 0) return 0;
  if (poly_off == nullptr || hw == nullptr || seg_off == nullptr || ends == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(poly_runs_kernel<1>, dim3(P), dim3(kThreads), 0, (hipStream_t)stream, verts, poly_off, hw, seg_off, (int*)nullptr,
                     ends);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_rle_target_nearest_u8(const int* ends, const long* seg_off, int seg_lo, int seg_hi, int H, int W, const int* yidx,
                                          const int* xidx, int Hout, int Wout, unsigned char* out, void* stream) {
  if (H < 1 || W < 1 || (long)H * W > (1L << 24) || Hout < 1 || Wout < 1 || (long)Hout * Wout > (1L << 24)) return (int)hipErrorInvalidValue;
  if (seg_lo < 0 || seg_hi < seg_lo || seg_hi - seg_lo > 255) return (int)hipErrorInvalidValue;
  if (seg_off == nullptr || yidx == nullptr || xidx == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rle_target_nearest_kernel, dim3(cdiv((long)Hout * Wout, 256)), dim3(256), 0, (hipStream_t)stream, ends, seg_off,
                     seg_lo, seg_hi, H, yidx, xidx, Hout, Wout, out);
  TRIS_LAUNCH_CHECK();
  return 0;
}
