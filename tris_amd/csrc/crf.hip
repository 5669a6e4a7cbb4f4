// IRNet's dense-CRF label pass (IRNet/step_refer/cam_to_ir_label.py:45-76, IRNet/misc/imutils.py:169-183): the mean field of
// Kraehenbuehl & Koltun 2011 with both Potts terms filtered on the permutohedral lattice of Adams, Baek & Davis 2010.
//   lattice points (per pixel: d+1 vertices and barycentric weights)  ->  [torch.unique: the vertex set]  ->  neighbour table
//   ->  filter pass = splat (segmented sum per vertex, no atomics), d+1 blur steps, slice  ->  softmax update  ->  combine.
// The geometry is f32 with one rounding per operation in the order of DESIGN.md section 14 (no contraction): the vertex set is
// part of the result and must not depend on who computed it.  Values are plain f32.  One launch per step; every launch is
// bitwise reproducible.
#include "common.h"
#include "tris_hip.h"

namespace {

constexpr int kFieldBits = 12;                 // TRIS_CRF_FIELD_BITS
constexpr long kFieldBias = 1L << (kFieldBits - 1);
constexpr long kFieldMask = (1L << kFieldBits) - 1;

// ---------------------------------------------------------------------------------------------------------- lattice points
// One pixel: cf[i] = feature i times scale[i] -> the d+1 packed keys and barycentric weights.  Every array is indexed by fully
// unrolled loops only, and the two data-dependent slots of the barycentric accumulation are selected by comparison, so everything
// stays in registers (no scratch).  f32 division is correctly rounded (the compiler's default for HIP), as numpy's.
template <int D>
__host__ __device__ __forceinline__ void crf_point(const float* cf, long* kp, float* bp) {
#pragma clang fp contract(off)
  constexpr int D1 = D + 1;
  // elevate
  float E[D1];
  float sm = 0.f;
#pragma unroll
  for (int j = D; j >= 1; --j) {
    E[j] = sm - (float)j * cf[j - 1];
    sm = sm + cf[j - 1];
  }
  E[0] = sm;
  // nearest zero-remainder point, the rank of the differences
  float rem0[D1];
  int rank[D1];
  int S = 0;
#pragma unroll
  for (int i = 0; i < D1; ++i) {
    float rd = roundf(E[i] / (float)D1);
    rem0[i] = rd * (float)D1;
    S += (int)rd;
    rank[i] = 0;
  }
#pragma unroll
  for (int i = 0; i < D1; ++i) {
#pragma unroll
    for (int j = i + 1; j < D1; ++j) {
      if (E[i] - rem0[i] < E[j] - rem0[j]) rank[i]++; else rank[j]++;
    }
  }
  if (S > 0) {
#pragma unroll
    for (int i = 0; i < D1; ++i) {
      if (rank[i] >= D1 - S) { rem0[i] = rem0[i] - (float)D1; rank[i] += S - D1; } else rank[i] += S;
    }
  } else if (S < 0) {
#pragma unroll
    for (int i = 0; i < D1; ++i) {
      if (rank[i] < -S) { rem0[i] = rem0[i] + (float)D1; rank[i] += S + D1; } else rank[i] += S;
    }
  }
  // barycentric weights
  float b[D + 2];
#pragma unroll
  for (int s = 0; s < D + 2; ++s) b[s] = 0.f;
#pragma unroll
  for (int i = 0; i < D1; ++i) {
    const float v = (E[i] - rem0[i]) / (float)D1;
    const int lo = D - rank[i];
#pragma unroll
    for (int s = 0; s < D + 2; ++s) {
      if (s == lo) b[s] = b[s] + v;
      if (s == lo + 1) b[s] = b[s] - v;
    }
  }
  b[0] = b[0] + (1.f + b[D1]);
  // the d+1 vertices: key[k] = rem0[k] + canon[r][rank[k]], packed with coordinate 0 in the highest field
#pragma unroll
  for (int r = 0; r < D1; ++r) {
    long packed = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const int c = (int)rem0[k] + (rank[k] <= D - r ? r : r - D1);
      packed = (packed << kFieldBits) | (((long)c + kFieldBias) & kFieldMask);
    }
    kp[r] = packed;
    bp[r] = b[r];
  }
}

// One thread per pixel: look the features up, scale them (one rounding), place the point.
template <int D>
__global__ __launch_bounds__(256) void crf_points_kernel(const unsigned char* __restrict__ img, const float* __restrict__ tx,
                                                         const float* __restrict__ ty, const float* __restrict__ tc,
                                                         const float* __restrict__ scale, int H, int W,
                                                         long* __restrict__ keys, float* __restrict__ bary) {
#pragma clang fp contract(off)
  constexpr int D1 = D + 1;
  const int N = H * W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  const int y = p / W, x = p - y * W;
  float cf[D];
  cf[0] = tx[x] * scale[0];
  cf[1] = ty[y] * scale[1];
  if constexpr (D == 5) {
    const unsigned char* px = img + 3L * p;
    cf[2] = tc[px[0]] * scale[2];
    cf[3] = tc[px[1]] * scale[3];
    cf[4] = tc[px[2]] * scale[4];
  }
  long k[D1];
  float b[D1];
  crf_point<D>(cf, k, b);
#pragma unroll
  for (int r = 0; r < D1; ++r) {
    keys[(long)p * D1 + r] = k[r];
    bary[(long)p * D1 + r] = b[r];
  }
}

// ---------------------------------------------------------------------------------------------------------- neighbour table
// One thread per (vertex, axis).  n1 = key - 1 in every coordinate except +d at the axis, n2 the opposite; axis d moves only the
// implied last coordinate.  A neighbour outside the packed field cannot be in the set.
template <int D>
__device__ __forceinline__ int crf_find(const long* __restrict__ uniq, int M, const int* c, int axis, int sign) {
  long q = 0;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    int v = c[k] + sign - (k == axis ? sign * (D + 1) : 0);
    ok = ok && v >= -(int)kFieldBias && v < (int)kFieldBias;
    q = (q << kFieldBits) | (((long)v + kFieldBias) & kFieldMask);
  }
  if (!ok) return -1;
  int lo = 0, hi = M;                       // first index with uniq[i] >= q
  while (lo < hi) {
    int mid = lo + ((hi - lo) >> 1);
    if (uniq[mid] < q) lo = mid + 1; else hi = mid;
  }
  return (lo < M && uniq[lo] == q) ? lo : -1;
}

template <int D>
__global__ __launch_bounds__(256) void crf_neighbours_kernel(const long* __restrict__ uniq, int M, int* __restrict__ nbr) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  const int axis = blockIdx.y;
  if (v >= M) return;
  long packed = uniq[v];
  int c[D];
#pragma unroll
  for (int k = D - 1; k >= 0; --k) {
    c[k] = (int)(packed & kFieldMask) - (int)kFieldBias;
    packed >>= kFieldBits;
  }
  nbr[((long)axis * 2 + 0) * M + v] = crf_find<D>(uniq, M, c, axis, -1);
  nbr[((long)axis * 2 + 1) * M + v] = crf_find<D>(uniq, M, c, axis, +1);
}

// -------------------------------------------------------------------------------------------------------------- filter pass
template <int C> struct Vec;
template <> struct Vec<1> { typedef float T; };
template <> struct Vec<2> { typedef float2 T; };
template <> struct Vec<4> { typedef float4 T; };

template <int C>
__device__ __forceinline__ void vload(float* r, const float* p) {
  typename Vec<C>::T v = *reinterpret_cast<const typename Vec<C>::T*>(p);
  const float* f = reinterpret_cast<const float*>(&v);
#pragma unroll
  for (int c = 0; c < C; ++c) r[c] = f[c];
}
template <int C>
__device__ __forceinline__ void vstore(float* p, const float* r) {
  typename Vec<C>::T v;
  float* f = reinterpret_cast<float*>(&v);
#pragma unroll
  for (int c = 0; c < C; ++c) f[c] = r[c];
  *reinterpret_cast<typename Vec<C>::T*>(p) = v;
}

// splat: val[v] = sum over the vertex's list, in list order, of bary[e] * norm[p] * x[p]; e = p (d+1) + r
template <int C>
__global__ __launch_bounds__(256) void crf_splat_kernel(const float* __restrict__ x, const float* __restrict__ norm,
                                                        const float* __restrict__ bary, const int* __restrict__ order,
                                                        const int* __restrict__ off, int M, int d1, float* __restrict__ val) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= M) return;
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  const int e1 = off[v + 1];
  for (int i = off[v]; i < e1; ++i) {
    const int e = order[i];
    const int p = e / d1;
    float w = bary[e];
    if (norm) w *= norm[p];
    float xv[C];
    vload<C>(xv, x + (long)p * C);
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] += w * xv[c];
  }
  vstore<C>(val + (long)v * C, acc);
}

// one blur axis: dst[v] = src[v] + 0.5 (src[n1] + src[n2]), absent neighbours contribute 0
template <int C>
__global__ __launch_bounds__(256) void crf_blur_kernel(const float* __restrict__ src, const int* __restrict__ n1,
                                                       const int* __restrict__ n2, int M, float* __restrict__ dst) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= M) return;
  float a[C], l[C], r[C];
  vload<C>(a, src + (long)v * C);
  const int i1 = n1[v], i2 = n2[v];
#pragma unroll
  for (int c = 0; c < C; ++c) l[c] = r[c] = 0.f;
  if (i1 >= 0) vload<C>(l, src + (long)i1 * C);
  if (i2 >= 0) vload<C>(r, src + (long)i2 * C);
#pragma unroll
  for (int c = 0; c < C; ++c) a[c] = a[c] + 0.5f * (l[c] + r[c]);
  vstore<C>(dst + (long)v * C, a);
}

// slice: out[p] = norm[p] alpha sum_r bary[p][r] val[inv[p][r]]
template <int C>
__global__ __launch_bounds__(256) void crf_slice_kernel(const float* __restrict__ val, const float* __restrict__ norm,
                                                        const float* __restrict__ bary, const int* __restrict__ inv, int N,
                                                        int d1, float alpha, float* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  for (int r = 0; r < d1; ++r) {
    const long e = (long)p * d1 + r;
    const float w = bary[e];
    float vv[C];
    vload<C>(vv, val + (long)inv[e] * C);
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] += w * vv[c];
  }
  const float s = norm ? alpha * norm[p] : alpha;
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] *= s;
  vstore<C>(out + (long)p * C, acc);
}

template <int C>
int crf_filter_launch(const float* x, float* out, int N, int d, int M, const float* bary, const int* inv, const int* order,
                      const int* off, const int* nbr, const float* norm, float* ws, hipStream_t st) {
  const int d1 = d + 1;
  float* a = ws;
  float* b = ws + (long)M * C;
  crf_splat_kernel<C><<<cdiv(M, 256), 256, 0, st>>>(x, norm, bary, order, off, M, d1, a);
  TRIS_LAUNCH_CHECK();
  for (int j = 0; j < d1; ++j) {
    crf_blur_kernel<C><<<cdiv(M, 256), 256, 0, st>>>(a, nbr + ((long)j * 2 + 0) * M, nbr + ((long)j * 2 + 1) * M, M, b);
    TRIS_LAUNCH_CHECK();
    float* t = a; a = b; b = t;
  }
  const float alpha = 1.f / (1.f + ldexpf(1.f, -d));
  crf_slice_kernel<C><<<cdiv(N, 256), 256, 0, st>>>(a, norm, bary, inv, N, d1, alpha, out);
  TRIS_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------- pointwise kernels
__global__ __launch_bounds__(256) void crf_norm_kernel(const float* __restrict__ k1, int N, float* __restrict__ norm) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < N) norm[p] = 1.f / sqrtf(k1[p] + 1e-20f);
}

// softmax over the two labels with the maximum subtracted
__device__ __forceinline__ void softmax2(float a0, float a1, float* q) {
  const float m = fmaxf(a0, a1);
  const float e0 = expf(a0 - m), e1 = expf(a1 - m);
  const float s = e0 + e1;
  q[0] = e0 / s;
  q[1] = e1 / s;
}

// unary and first Q of R label maps at once; lab = the r-th label of pixel p
__device__ __forceinline__ void crf_unary_store(int lab, float e_same, float e_diff, float* U, float* Q) {
  U[0] = lab == 0 ? e_same : e_diff;
  U[1] = lab == 1 ? e_same : e_diff;
  softmax2(-U[0], -U[1], Q);
}

__global__ __launch_bounds__(256) void crf_unary_cam_kernel(const float* __restrict__ cam, int N, float thr_fg, float thr_bg,
                                                            float e_same, float e_diff, float* __restrict__ U,
                                                            float* __restrict__ Q) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  float c = cam[p];
  if (c < 0.f) c = 0.f;                                   // cams[cams < 0] = 0; a NaN stays and compares false
  float u[4], q[4];
  crf_unary_store(c > thr_fg ? 1 : 0, e_same, e_diff, u, q);           // strict: argmax of [thr, cam], a tie gives 0
  crf_unary_store(c > thr_bg ? 1 : 0, e_same, e_diff, u + 2, q + 2);
  vstore<4>(U + 4L * p, u);
  vstore<4>(Q + 4L * p, q);
}

__global__ __launch_bounds__(256) void crf_unary_labels_kernel(const unsigned char* __restrict__ labels, int R, int N,
                                                               float e_same, float e_diff, float* __restrict__ U,
                                                               float* __restrict__ Q) {
  const int i = blockIdx.x * 256 + threadIdx.x;          // i = p R + r
  if (i >= N * R) return;
  const int p = i / R, r = i - p * R;
  float u[2], q[2];
  crf_unary_store(labels[(long)r * N + p] != 0 ? 1 : 0, e_same, e_diff, u, q);
  vstore<2>(U + 2L * i, u);
  vstore<2>(Q + 2L * i, q);
}

__global__ __launch_bounds__(256) void crf_update_kernel(const float* __restrict__ U, const float* __restrict__ g,
                                                         const float* __restrict__ b, float wg, float wb, int n,
                                                         float* __restrict__ Q) {
  const int i = blockIdx.x * 256 + threadIdx.x;          // one (pixel, CRF) pair
  if (i >= n) return;
  float u[2], gv[2], bv[2], q[2];
  vload<2>(u, U + 2L * i);
  vload<2>(gv, g + 2L * i);
  vload<2>(bv, b + 2L * i);
  softmax2(-u[0] + wg * gv[0] + wb * bv[0], -u[1] + wg * gv[1] + wb * bv[1], q);
  vstore<2>(Q + 2L * i, q);
}

__global__ __launch_bounds__(256) void crf_combine_kernel(const float* __restrict__ Q, int N, unsigned char* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  float q[4];
  vload<4>(q, Q + 4L * p);
  const int fg = q[1] > q[0] ? 1 : 0;                    // argmax, the first on a tie
  const int bg = q[3] > q[2] ? 1 : 0;
  int conf = fg;
  if (fg == 0) conf = 255;
  if (bg + fg == 0) conf = 0;
  out[p] = (unsigned char)conf;
}

}  // namespace

extern "C" {

int tris_crf_lattice_points_f32(const unsigned char* img, const float* tx, const float* ty, const float* tc, const float* scale,
                                int H, int W, int d, long* keys, float* bary, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (H <= 0 || W <= 0 || (long)H * W * 6 > 2147483647L) return (int)hipErrorInvalidValue;
  const int N = H * W;
  if (d == 2) {
    crf_points_kernel<2><<<cdiv(N, 256), 256, 0, st>>>(nullptr, tx, ty, nullptr, scale, H, W, keys, bary);
  } else if (d == 5) {
    if (!img || !tc) return (int)hipErrorInvalidValue;
    crf_points_kernel<5><<<cdiv(N, 256), 256, 0, st>>>(img, tx, ty, tc, scale, H, W, keys, bary);
  } else {
    return (int)hipErrorInvalidValue;
  }
  TRIS_LAUNCH_CHECK();
  return 0;
}

int tris_crf_neighbours_i64(const long* uniq, int M, int d, int* nbr, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (M <= 0) return (int)hipErrorInvalidValue;
  dim3 grid(cdiv(M, 256), d + 1);
  if (d == 2) crf_neighbours_kernel<2><<<grid, 256, 0, st>>>(uniq, M, nbr);
  else if (d == 5) crf_neighbours_kernel<5><<<grid, 256, 0, st>>>(uniq, M, nbr);
  else return (int)hipErrorInvalidValue;
  TRIS_LAUNCH_CHECK();
  return 0;
}

long tris_crf_filter_workspace_bytes(int M, int C) { return (M > 0 && C > 0) ? 2L * M * C * (long)sizeof(float) : 0; }

int tris_crf_filter_f32(const float* x, float* out, int N, int C, int d, int M, const float* bary, const int* inv,
                        const int* order, const int* off, const int* nbr, const float* norm, float* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (N <= 0 || M <= 0 || d < 1 || !workspace) return (int)hipErrorInvalidValue;
  switch (C) {
    case 1: return crf_filter_launch<1>(x, out, N, d, M, bary, inv, order, off, nbr, norm, workspace, st);
    case 2: return crf_filter_launch<2>(x, out, N, d, M, bary, inv, order, off, nbr, norm, workspace, st);
    case 4: return crf_filter_launch<4>(x, out, N, d, M, bary, inv, order, off, nbr, norm, workspace, st);
    default: return (int)hipErrorInvalidValue;
  }
}

int tris_crf_norm_f32(const float* k1, int N, float* norm, void* stream) {
  crf_norm_kernel<<<cdiv(N, 256), 256, 0, (hipStream_t)stream>>>(k1, N, norm);
  TRIS_LAUNCH_CHECK();
  return 0;
}

int tris_crf_unary_cam_f32(const float* cam, int N, float thr_fg, float thr_bg, float e_same, float e_diff, float* U, float* Q,
                           void* stream) {
  crf_unary_cam_kernel<<<cdiv(N, 256), 256, 0, (hipStream_t)stream>>>(cam, N, thr_fg, thr_bg, e_same, e_diff, U, Q);
  TRIS_LAUNCH_CHECK();
  return 0;
}

int tris_crf_unary_labels_u8(const unsigned char* labels, int R, int N, float e_same, float e_diff, float* U, float* Q,
                             void* stream) {
  if (R != 1 && R != 2) return (int)hipErrorInvalidValue;
  crf_unary_labels_kernel<<<cdiv((long)N * R, 256), 256, 0, (hipStream_t)stream>>>(labels, R, N, e_same, e_diff, U, Q);
  TRIS_LAUNCH_CHECK();
  return 0;
}

int tris_crf_update_f32(const float* U, const float* g, const float* b, float wg, float wb, int N, int R, float* Q, void* stream) {
  crf_update_kernel<<<cdiv((long)N * R, 256), 256, 0, (hipStream_t)stream>>>(U, g, b, wg, wb, N * R, Q);
  TRIS_LAUNCH_CHECK();
  return 0;
}

int tris_crf_combine_u8(const float* Q, int N, unsigned char* out, void* stream) {
  crf_combine_kernel<<<cdiv(N, 256), 256, 0, (hipStream_t)stream>>>(Q, N, out);
  TRIS_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
