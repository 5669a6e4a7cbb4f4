// Instance-mask synthesis: the post-network half of IRNet's make_ins_seg_labels (IRNet/step_refer/make_ins_seg_labels.py,
// IRNet/misc/indexing.py).  (response map, edge map, displacement field) -> instance masks for the Stage-2 pseudo labels.
//   centroid refinement  ->  connected components of the weak-displacement regions  ->  instance map  ->  per-instance maps
//   -> edge -> sparse affinity (34 directions, radius 5)  ->  random walk v <- v T, 2^exp_times steps (never the dense N x N
//   matrix)  ->  x4 upsample, normalise, arg-max against the background  ->  connected fragments with area and score.
// All f32 on the vector ALU except the centroid refinement, which follows the reference's numpy promotion to f64, and the
// accumulation of the column sums.
#include "common.h"
#include "tris_hip.h"
#include "bilinear.h"
#include "unionfind.h"

namespace {

// ---------------------------------------------------------------------------------------------- centroid refinement
// make_ins_seg_labels.py:18-56.  One thread per pixel: a trajectory depends on the field alone.  The reference subtracts an
// int32 array from the float32 centroid, which numpy promotes to float64: the fractions, the four products and their sum are
// float64, and `centroid += sum` adds in float64 and rounds to float32 once.  The same operations in the same order, without
// contraction, give the same bits.
__global__ __launch_bounds__(256) void irn_centroids_kernel(const float* __restrict__ dp, int h, int w, int iterations,
                                                            int* __restrict__ out) {
#pragma clang fp contract(off)
  int p = blockIdx.x * 256 + threadIdx.x;
  int n = h * w;
  if (p >= n) return;
  const float* d0 = dp;
  const float* d1 = dp + n;
  float cy = (float)(p / w), cx = (float)(p % w);
  const float ymax = (float)(h - 1), xmax = (float)(w - 1);
  for (int it = 0; it < iterations; ++it) {
    // (the clamps only guard the gathers against a non-finite field; a finite trajectory stays inside by the clip below)
    int uy = min(max((int)ceilf(cy), 0), h - 1), dy = min(max((int)floorf(cy), 0), h - 1);
    int ux = min(max((int)ceilf(cx), 0), w - 1), dx = min(max((int)floorf(cx), 0), w - 1);
    double yc = (double)cy - (double)dy, xc = (double)cx - (double)dx;
    double oy = 1.0 - yc, ox = 1.0 - xc;
    int uu = uy * w + ux, du = dy * w + ux, ud = uy * w + dx, dd = dy * w + dx;
    double my = (double)d0[uu] * yc * xc + (double)d0[du] * oy * xc + (double)d0[ud] * yc * ox + (double)d0[dd] * oy * ox;
    double mx = (double)d1[uu] * yc * xc + (double)d1[du] * oy * xc + (double)d1[ud] * yc * ox + (double)d1[dd] * oy * ox;
    cy = (float)((double)cy + my);
    cx = (float)((double)cx + mx);
    cy = fminf(fmaxf(cy, 0.f), ymax);
    cx = fminf(fmaxf(cx, 0.f), xmax);
  }
  out[p] = (int)rintf(cy);       // round half to even, as np.round
  out[n + p] = (int)rintf(cx);
}

// cluster_centroids (:58-66): dp_strength = sqrt(dp[1]^2 + dp[0]^2) < thres, f32 one operation at a time
__global__ __launch_bounds__(256) void irn_weak_mask_kernel(const float* __restrict__ dp, int n, float thres,
                                                            unsigned char* __restrict__ mask) {
#pragma clang fp contract(off)
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  float a = dp[n + p] * dp[n + p];
  float b = dp[p] * dp[p];
  mask[p] = sqrtf(a + b) < thres ? 1 : 0;
}

// ---------------------------------------------------------------------------------------- connected-component labelling
// Union-find on the pixel grid (4-connectivity, unionfind.h), in the manner of Komura's label-equivalence method.  A component's
// root is its minimum linear index = its first pixel in raster order; ranking the roots by index gives skimage's numbering.
// Every foreground pixel starts linked to its upper neighbour, else to its left one, else to itself: the links already span each
// component except where a pixel has both neighbours, and only those pairs are united (with atomics) after a compression pass
// has shortened the chains -- in a solid region they then meet at a common root at once and no atomic is issued.
__global__ __launch_bounds__(256) void cc_init_kernel(const unsigned char* __restrict__ img, int H, int W, int* __restrict__ parent) {
  int n = H * W;
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  long o = (long)blockIdx.y * n;
  const unsigned char* im = img + o;
  int v = -1;
  if (im[p]) v = (p >= W && im[p - W]) ? p - W : ((p % W) > 0 && im[p - 1]) ? p - 1 : p;
  parent[o + p] = v;
}
// parent[p] <- the root of p
__global__ __launch_bounds__(256) void cc_compress_kernel(int* parent, int n) {
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  int* L = parent + (long)blockIdx.y * n;
  int a = uf_load(L, p);
  if (a < 0 || a == p) return;
  __atomic_store_n(&L[p], uf_root(L, a), __ATOMIC_RELAXED);
}
__global__ __launch_bounds__(256) void cc_merge_kernel(const unsigned char* __restrict__ img, int H, int W, int* parent) {
  int n = H * W;
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  long o = (long)blockIdx.y * n;
  const unsigned char* im = img + o;
  if (!im[p]) return;
  if (p >= W && im[p - W] && (p % W) > 0 && im[p - 1]) uf_unite(parent + o, p, p - 1);   // (the other links are the initial ones)
}
// root[p] = the root of p (or -1), flag[p] = p is a root
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* __restrict__ parent, int n, int* __restrict__ root,
                                                         int* __restrict__ flag) {
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  long o = (long)blockIdx.y * n;
  int r = uf_load(parent + o, p) >= 0 ? uf_root(parent + o, p) : -1;
  root[o + p] = r;
  flag[o + p] = (r == p) ? 1 : 0;
}
// exclusive prefix count of flags, in place: rank[i] = number of set flags before i; count = total.  One workgroup per image;
// each thread walks a contiguous run of n / 1024 flags, so its loads are strided across the wave (a known cost of the labelling:
// about 400 sequential loads per thread at 638 x 639).
__global__ __launch_bounds__(1024) void rank_flags_kernel(int* __restrict__ flag, int n, int* __restrict__ count) {
  __shared__ int s[1024];
  int* f = flag + (long)blockIdx.x * n;
  int t = threadIdx.x;
  int len = (n + 1023) / 1024;
  int lo = min(t * len, n), hi = min(lo + len, n);
  int c = 0;
  for (int i = lo; i < hi; ++i) c += f[i];
  s[t] = c;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    int v = t >= o ? s[t - o] : 0;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  int run = s[t] - c;
  for (int i = lo; i < hi; ++i) {
    int v = f[i];
    f[i] = run;
    run += v;
  }
  if (t == 1023) count[blockIdx.x] = s[1023];
}
__global__ __launch_bounds__(256) void cc_final_kernel(int* __restrict__ labels, const int* __restrict__ rank, int n) {
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  long o = (long)blockIdx.y * n;
  int r = labels[o + p];
  labels[o + p] = r >= 0 ? rank[o + r] + 1 : 0;
}

// ---------------------------------------------------------------------------------------------------- instance map
// cluster_centroids (:69-75): the weak-region label under each pixel's centroid, compressed to 0..K-1 in label order
__global__ __launch_bounds__(256) void irn_mark_kernel(const int* __restrict__ cen, const int* __restrict__ lab, int n, int w,
                                                       int n_label, int* __restrict__ cl, int* __restrict__ present) {
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  int q = cen[p] * w + cen[n + p];
  q = min(max(q, 0), n - 1);
  int c = min(max(lab[q], 0), n_label);
  cl[p] = c;
  present[c] = 1;   // (every writer stores the same value)
}
__global__ __launch_bounds__(256) void irn_compress_kernel(int* __restrict__ cl, const int* __restrict__ rank, int n) {
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p < n) cl[p] = rank[cl[p]];
}
// separte_score_by_mask (:77-80): out[k] = cam * (instance map == k)
__global__ __launch_bounds__(256) void irn_instance_cam_kernel(const float* __restrict__ cam, const int* __restrict__ inst, int n,
                                                               float* __restrict__ out) {
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  out[(long)blockIdx.y * n + p] = inst[p] == (int)blockIdx.y ? cam[p] : 0.f;
}

// ------------------------------------------------------------------------------------------ edge -> sparse affinity
// indexing.py:18-109: Wt[d][p] = (1 - max of the edge over the path cells from p to p + dir_d) ^ beta where both ends lie in
// the map, 0 where the destination falls outside (the reference pads the edge with 1.0 there, and every path cell lies in
// the bounding box of its two ends).
__global__ __launch_bounds__(256) void irn_affinity_kernel(const float* __restrict__ edge, int h, int w,
                                                           const int* __restrict__ dirs, const int* __restrict__ path_off,
                                                           const int* __restrict__ cells, float beta, float* __restrict__ Wt) {
  int n = h * w;
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  int d = blockIdx.y;
  int y = p / w, x = p % w;
  int ty = y + dirs[2 * d], tx = x + dirs[2 * d + 1];
  float v = 0.f;
  if (ty >= 0 && ty < h && tx >= 0 && tx < w) {
    float m = -INFINITY;
    for (int c = path_off[d]; c < path_off[d + 1]; ++c) m = fmaxf(m, edge[(y + cells[2 * c]) * w + x + cells[2 * c + 1]]);
    v = powf(1.0f - m, beta);
  }
  Wt[(long)d * n + p] = v;
}
// indexing.py:135: the column sum of the symmetric affinity with its unit diagonal, 1 + the 68 incident weights
__global__ __launch_bounds__(256) void irn_colsum_kernel(const float* __restrict__ Wt, int h, int w, const int* __restrict__ dirs,
                                                         int nd, float* __restrict__ colsum) {
  int n = h * w;
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  int y = p / w, x = p % w;
  double s = 1.0;   // one rounding at the end: a column sum that is off by ulps would bias every step of the walk the same way
  for (int d = 0; d < nd; ++d) {
    int dy = dirs[2 * d], dx = dirs[2 * d + 1];
    s += Wt[(long)d * n + p];                       // 0 where p + dir is outside
    int qy = y - dy, qx = x - dx;
    if (qy >= 0 && qx >= 0 && qx < w) s += Wt[(long)d * n + qy * w + qx];
  }
  colsum[p] = (float)s;
}

// ------------------------------------------------------------------------------------------------------- the walk
// One step at pixel p: (v[p] + sum_d Wt[d][p] v[p + dir_d] + Wt[d][p - dir_d] v[p - dir_d]) / colsum[p]  (indexing.py:132-164
// with x T^(2^t) evaluated as 2^t products v T; T is never formed).  Out-of-map neighbours: the forward weight is 0 by
// construction and the index is redirected to p; the backward term is dropped.
__device__ __forceinline__ float walk_gather(const float* __restrict__ v, const float* __restrict__ Wt, const int* __restrict__ dirs, int nd,
                                             int n, int h, int w, int p) {
  int y = p / w, x = p % w;
  float acc = v[p];
  for (int d = 0; d < nd; ++d) {
    int dy = dirs[2 * d], dx = dirs[2 * d + 1];
    int off = dy * w + dx;
    const float* Wd = Wt + (long)d * n;
    bool fwd = (y + dy < h) && (x + dx >= 0) && (x + dx < w);
    bool bwd = (y - dy >= 0) && (x - dx >= 0) && (x - dx < w);
    int qf = fwd ? p + off : p, qb = bwd ? p - off : p;
    float wb = Wd[qb];
    acc += Wd[p] * v[qf];
    acc += (bwd ? wb : 0.f) * v[qb];
  }
  return acc;
}
// one launch per step, rows ping-pong between two global buffers (an LDS-resident one-launch form was measured 4-11x slower:
// DESIGN.md, "Instance-mask synthesis")
__global__ __launch_bounds__(256) void irn_walk_seed_kernel(const float* __restrict__ x, const float* __restrict__ edge, int n,
                                                            float* __restrict__ v) {
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  long o = (long)blockIdx.y * n;
  v[o + p] = x[o + p] * (1.0f - edge[p]);
}
__global__ __launch_bounds__(256) void irn_walk_step_kernel(const float* __restrict__ vin, const float* __restrict__ Wt,
                                                            const float* __restrict__ colsum, const int* __restrict__ dirs,
                                                            int nd, int h, int w, float* __restrict__ vout) {
  int n = h * w;
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  long o = (long)blockIdx.y * n;
  vout[o + p] = walk_gather(vin + o, Wt, dirs, nd, n, h, w, p) / colsum[p];
}

// --------------------------------------------------------------------------------------------------------- finish
// make_ins_seg_labels.py:146-157: x4 bilinear (align_corners=False) cropped to (H, W), / global max, arg-max over
// [background, rows...] with the first maximum winning.
__global__ __launch_bounds__(256) void irn_up_kernel(const float* __restrict__ rw, int K, int h, int w, int H, int W,
                                                     float* __restrict__ up, float* __restrict__ ws) {
  __shared__ float red[4];
  long n = (long)H * W, tot = n * K;
  float best = -INFINITY;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < tot; i += (long)gridDim.x * 256) {
    int k = (int)(i / n);
    int r = (int)(i % n);
    Lerp ly = lerp_of(r / W, h, 4 * h, 0), lx = lerp_of(r % W, w, 4 * w, 0);
    const float* d = rw + (long)k * h * w;
    float v00 = d[ly.i0 * w + lx.i0], v01 = d[ly.i0 * w + lx.i1], v10 = d[ly.i1 * w + lx.i0], v11 = d[ly.i1 * w + lx.i1];
    float top = v00 + lx.w1 * (v01 - v00), bot = v10 + lx.w1 * (v11 - v10);
    float v = top + ly.w1 * (bot - top);
    up[i] = v;
    best = fmaxf(best, v);
  }
  best = block_max_256(best, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = best;
}
__global__ __launch_bounds__(64) void irn_max_final_kernel(float* __restrict__ ws, int nb) {
  float best = -INFINITY;
  for (int b = threadIdx.x; b < nb; b += 64) best = fmaxf(best, ws[b]);
  best = wave_max(best);
  if (threadIdx.x == 0) ws[nb] = best;
}
__global__ __launch_bounds__(256) void irn_argmax_kernel(float* __restrict__ up, int K, long n, float bg, const float* __restrict__ ws,
                                                         int nb, int* __restrict__ labels) {
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float mx = ws[nb];
  float best = bg;
  int bi = 0;
  for (int k = 0; k < K; ++k) {
    float v = up[(long)k * n + i] / mx;
    up[(long)k * n + i] = v;
    if (v > best) { best = v; bi = k + 1; }
  }
  labels[i] = bi;
}

// ----------------------------------------------------------------------------------------------------- fragments
// to_one_hot: masks[k] = (labels == k + base); base 1 drops the background plane (:157)
__global__ __launch_bounds__(256) void irn_label_masks_kernel(const int* __restrict__ labels, long n, int base,
                                                              unsigned char* __restrict__ masks) {
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  masks[(long)blockIdx.y * n + i] = labels[i] == (int)blockIdx.y + base ? 1 : 0;
}
// detect_instance (:82-105): per fragment its mask, its area and max(rw_up * mask) (>= 0: the product is 0 off the mask)
__global__ __launch_bounds__(256) void irn_fragments_kernel(const int* __restrict__ fl, const float* __restrict__ up,
                                                            const int* __restrict__ offsets, long n, int F, int* __restrict__ area,
                                                            int* __restrict__ score_bits, unsigned char* __restrict__ masks) {
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  int k = blockIdx.y;
  int g = -1, bits = 0;
  if (i < n) {
    int f = fl[(long)k * n + i];
    if (f > 0 && offsets[k] + f - 1 < F) {
      g = offsets[k] + f - 1;
      masks[(long)g * n + i] = 1;
      float v = up[(long)k * n + i];
      bits = v > 0.f ? __float_as_int(v) : 0;   // non-negative floats order as their bit patterns
    }
  }
  // every lane of the wave is still active here.  The common case, one fragment under the whole wave, costs two atomics.
  int g0 = g, m = bits;
  for (int o = 32; o > 0; o >>= 1) { g0 = max(g0, __shfl_xor(g0, o, 64)); m = max(m, __shfl_xor(m, o, 64)); }
  if (g0 < 0) return;
  const int cnt = __popcll(__ballot(g >= 0));   // (taken while the whole wave is active)
  if (__all(g < 0 || g == g0)) {
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&area[g0], cnt);
      atomicMax(&score_bits[g0], m);
    }
  } else if (g >= 0) {
    atomicAdd(&area[g], 1);
    atomicMax(&score_bits[g], bits);
  }
}
__global__ __launch_bounds__(256) void irn_fragment_scores_kernel(const int* __restrict__ area, const int* __restrict__ score_bits,
                                                                  int F, long min_area, float* __restrict__ score) {
  int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= F) return;
  score[g] = (long)area[g] < min_area ? 0.f : __int_as_float(score_bits[g]);
}

}  // namespace

#define GRID1(n) dim3(cdiv((n), 256))

extern "C" int tris_irn_centroids_f32(const float* dp, int h, int w, int iterations, int* centroids, void* stream) {
  hipLaunchKernelGGL(irn_centroids_kernel, GRID1((long)h * w), dim3(256), 0, (hipStream_t)stream, dp, h, w, iterations, centroids);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_irn_weak_mask_f32(const float* dp, int h, int w, float thres, unsigned char* mask, void* stream) {
  hipLaunchKernelGGL(irn_weak_mask_kernel, GRID1((long)h * w), dim3(256), 0, (hipStream_t)stream, dp, h * w, thres, mask);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" long tris_cc_workspace_bytes(int B, int H, int W) { return 2L * B * H * W * (long)sizeof(int); }

extern "C" int tris_cc_label_u8(const unsigned char* img, int B, int H, int W, int* labels, int* counts, int* workspace,
                                void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  if ((long)H * W > 0x7fffffffL || B > 65535) return (int)hipErrorInvalidValue;
  int n = H * W;
  int* parent = workspace;
  int* flag = workspace + (long)B * n;
  dim3 grid(cdiv(n, 256), B);
  hipLaunchKernelGGL(cc_init_kernel, grid, dim3(256), 0, st, img, H, W, parent);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_compress_kernel, grid, dim3(256), 0, st, parent, n);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_merge_kernel, grid, dim3(256), 0, st, img, H, W, parent);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_flatten_kernel, grid, dim3(256), 0, st, parent, n, labels, flag);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_flags_kernel, dim3(B), dim3(1024), 0, st, flag, n, counts);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_final_kernel, grid, dim3(256), 0, st, labels, flag, n);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_irn_cluster_i32(const int* centroids, const int* dp_label, int n_label, int h, int w, int* inst_map,
                                    int* n_inst, int* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  int n = h * w;
  if (n_label < 0 || n_label > n) return (int)hipErrorInvalidValue;
  int* present = workspace;   // n_label + 1 words
  hipError_t e = hipMemsetAsync(present, 0, (size_t)(n_label + 1) * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(irn_mark_kernel, GRID1(n), dim3(256), 0, st, centroids, dp_label, n, w, n_label, inst_map, present);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_flags_kernel, dim3(1), dim3(1024), 0, st, present, n_label + 1, n_inst);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(irn_compress_kernel, GRID1(n), dim3(256), 0, st, inst_map, present, n);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_irn_instance_cam_f32(const float* cam, const int* inst_map, int K, int n, float* out, void* stream) {
  if (K <= 0) return 0;
  if (K > 65535) return (int)hipErrorInvalidValue;   // (K is the grid's y extent)
  hipLaunchKernelGGL(irn_instance_cam_kernel, dim3(cdiv(n, 256), K), dim3(256), 0, (hipStream_t)stream, cam, inst_map, n, out);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_irn_affinity_f32(const float* edge, int h, int w, const int* dirs, const int* path_off, const int* path_cells,
                                     int n_dirs, float beta, float* Wt, float* colsum, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  int n = h * w;
  hipLaunchKernelGGL(irn_affinity_kernel, dim3(cdiv(n, 256), n_dirs), dim3(256), 0, st, edge, h, w, dirs, path_off, path_cells,
                     beta, Wt);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(irn_colsum_kernel, GRID1(n), dim3(256), 0, st, Wt, h, w, dirs, n_dirs, colsum);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_irn_walk_f32(const float* x, const float* edge, const float* Wt, const float* colsum, const int* dirs,
                                 int n_dirs, int K, int h, int w, int steps, float* out, float* tmp, void* stream) {
  if (K <= 0) return 0;
  if (K > 65535) return (int)hipErrorInvalidValue;   // (K is the grid's y extent)
  hipStream_t st = (hipStream_t)stream;
  int n = h * w;
  dim3 grid(cdiv(n, 256), K);
  float* cur = (steps & 1) ? tmp : out;   // so that the last step lands in `out`
  float* nxt = (steps & 1) ? out : tmp;
  hipLaunchKernelGGL(irn_walk_seed_kernel, grid, dim3(256), 0, st, x, edge, n, cur);
  TRIS_LAUNCH_CHECK();
  for (int s = 0; s < steps; ++s) {
    hipLaunchKernelGGL(irn_walk_step_kernel, grid, dim3(256), 0, st, cur, Wt, colsum, dirs, n_dirs, h, w, nxt);
    TRIS_LAUNCH_CHECK();
    float* t = cur; cur = nxt; nxt = t;
  }
  return 0;
}

extern "C" int tris_irn_finish_f32(const float* rw, int K, int h, int w, int H, int W, float bg_thres, float* rw_up, int* labels,
                                   float* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (K <= 0 || H > 4 * h || W > 4 * w) return (int)hipErrorInvalidValue;
  long n = (long)H * W;
  int nb = cdiv(n * K, 256);
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(irn_up_kernel, dim3(nb), dim3(256), 0, st, rw, K, h, w, H, W, rw_up, workspace);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(irn_max_final_kernel, dim3(1), dim3(64), 0, st, workspace, nb);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(irn_argmax_kernel, GRID1(n), dim3(256), 0, st, rw_up, K, n, bg_thres, workspace, nb, labels);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_irn_label_masks_u8(const int* labels, int K, long n, int base, unsigned char* masks, void* stream) {
  if (K <= 0) return 0;
  if (K > 65535) return (int)hipErrorInvalidValue;   // (K is the grid's y extent)
  hipLaunchKernelGGL(irn_label_masks_kernel, dim3(cdiv(n, 256), K), dim3(256), 0, (hipStream_t)stream, labels, n, base, masks);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_irn_fragments_f32(const int* frag_labels, const float* rw_up, const int* offsets, int K, long n, long min_area,
                                      int F, float* score, int* area, unsigned char* frag_masks, int* workspace, void* stream) {
  if (K <= 0 || F <= 0) return 0;
  if (K > 65535) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(area, 0, (size_t)F * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(workspace, 0, (size_t)F * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(frag_masks, 0, (size_t)F * n, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(irn_fragments_kernel, dim3(cdiv(n, 256), K), dim3(256), 0, st, frag_labels, rw_up, offsets, n, F, area,
                     workspace, frag_masks);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(irn_fragment_scores_kernel, GRID1(F), dim3(256), 0, st, area, workspace, F, min_area, score);
  TRIS_LAUNCH_CHECK();
  return 0;
}
