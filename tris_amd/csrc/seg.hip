// Stage-2 decoder kernels (gfx950): the pseudo-mask decoder of model/model_stage2.py on channels-last activations.
//   * BatchNorm (statistics from the conv epilogue / bn_finalize) + one-slope PReLU: apply, backward reduce, backward apply
//   * bilinear upsample (align_corners=False) with the skip add of the top-down path, and its gather-form backward
//   * the one-channel 1x1 heads (C -> 1) and their backward
//   * binary cross-entropy with logits of the four heads against the int64 pseudo target (or an fp32 one)
//   * signed evaluation post-processing (validate.py:179-191 on maps that may be negative)
// Every reduction is a fixed-order two-stage one (per-block fp64 partials -> one finalize), no atomics: a step is bitwise
// reproducible.  Scalars that change during training (the PReLU slope, the loss gradients) are read from device memory.
#include "common.h"
#include "tris_hip.h"
#include "bilinear.h"

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

constexpr int SEG_BLOCKS = 512;   // partial rows of a column reduction (fixed for a shape: the sums are reproducible)

inline int seg_grid(long n) {
  long g = (n + 255) / 256;
  return (int)(g < 4096 ? (g < 1 ? 1 : g) : 4096);
}
inline int red_blocks(long M) {
  long nb = (M + 63) / 64;
  return (int)(nb < SEG_BLOCKS ? (nb < 1 ? 1 : nb) : SEG_BLOCKS);
}

// ------------------------------------------------------------------------------------------------ BatchNorm + PReLU
// z = (x - mean) * (invstd * gamma) + beta  (bn_apply_kernel's expression, csrc/norm.hip);  y = z > 0 ? z : a * z  (nn.PReLU)
__global__ __launch_bounds__(256) void bn_prelu_fwd_kernel(const float* __restrict__ X, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ slope,
                                                           float* __restrict__ Y, long n4, int C4) {
  const float a = slope[0];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C4) * 4;
    const float4 mu = ld4(mean + c), is = ld4(invstd + c), g = ld4(gamma + c), b = ld4(beta + c);
    const float4 x = ld4(X + i * 4);
    float4 z;
    z.x = (x.x - mu.x) * (is.x * g.x) + b.x;
    z.y = (x.y - mu.y) * (is.y * g.y) + b.y;
    z.z = (x.z - mu.z) * (is.z * g.z) + b.z;
    z.w = (x.w - mu.w) * (is.w * g.w) + b.w;
    z.x = z.x > 0.f ? z.x : a * z.x;
    z.y = z.y > 0.f ? z.y : a * z.y;
    z.z = z.z > 0.f ? z.z : a * z.z;
    z.w = z.w > 0.f ? z.w : a * z.w;
    st4(Y + i * 4, z);
  }
}

// Partials of the backward sums.  Block = 256 threads = RS rows x CV channel vectors (C <= 1024, 1024 % C == 0), rows
// [rbeg, rend).  part[blk] = [sum dz (C) | sum dz*xhat (C) | slope term (1)], fp64.
__global__ __launch_bounds__(256) void bn_prelu_bwd_partial_kernel(const float* __restrict__ dY, const float* __restrict__ X,
                                                                   const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   const float* __restrict__ slope, long M, int C, long rpb,
                                                                   double* __restrict__ part) {
  __shared__ double s0[256][4];
  __shared__ double s1[256][4];
  __shared__ double s2[256];
  const int CV = C >> 2, RS = 256 / CV, tid = threadIdx.x;
  const int cv = tid % CV, ro = tid / CV, c = cv * 4;
  const float a = slope[0];
  const float4 mu = ld4(mean + c), is = ld4(invstd + c), g = ld4(gamma + c), b = ld4(beta + c);
  const float4 sc = make_float4(is.x * g.x, is.y * g.y, is.z * g.z, is.w * g.w);
  double d0[4] = {0, 0, 0, 0}, d1[4] = {0, 0, 0, 0}, ds = 0.0;
  const long rbeg = (long)blockIdx.x * rpb, rend = min(M, rbeg + rpb);
  for (long r = rbeg + ro; r < rend; r += RS) {
    const float4 x = ld4(X + r * C + c), dy = ld4(dY + r * C + c);
    const float xv[4] = {x.x, x.y, x.z, x.w}, gv[4] = {dy.x, dy.y, dy.z, dy.w};
    const float muv[4] = {mu.x, mu.y, mu.z, mu.w}, isv[4] = {is.x, is.y, is.z, is.w};
    const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float z = (xv[k] - muv[k]) * scv[k] + bv[k];
      const bool pos = z > 0.f;
      const float dz = pos ? gv[k] : a * gv[k];
      const float xh = (xv[k] - muv[k]) * isv[k];
      d0[k] += (double)dz;
      d1[k] += (double)dz * (double)xh;
      if (!pos) ds += (double)gv[k] * (double)z;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { s0[tid][k] = d0[k]; s1[tid][k] = d1[k]; }
  s2[tid] = ds;
  __syncthreads();
  double* out = part + (long)blockIdx.x * (2 * C + 1);
  if (ro == 0) {
    double t0[4] = {0, 0, 0, 0}, t1[4] = {0, 0, 0, 0};
    for (int q = 0; q < RS; ++q)
#pragma unroll
      for (int k = 0; k < 4; ++k) { t0[k] += s0[q * CV + cv][k]; t1[k] += s1[q * CV + cv][k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) { out[c + k] = t0[k]; out[C + c + k] = t1[k]; }
  }
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s2[tid] += s2[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[2 * C] = s2[0];
}

// per channel (and the slope) sum of the partial rows in block order
__global__ __launch_bounds__(256) void seg_part_finalize_kernel(const double* __restrict__ part, int nb, int C, int W,
                                                                float* __restrict__ out0, float* __restrict__ out1,
                                                                float* __restrict__ out2) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= W) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += part[(long)b * W + j];
  if (j < C) out0[j] = (float)s;
  else if (j < 2 * C) out1[j - C] = (float)s;
  else out2[j - 2 * C] = (float)s;
}

// dx = gamma*invstd * (dz - sum_dz/cnt - xhat * sum_dzx/cnt)   (bn_bwd_apply_kernel's expression), dz = dy * (z > 0 ? 1 : a)
__global__ __launch_bounds__(256) void bn_prelu_bwd_apply_kernel(const float* __restrict__ dY, const float* __restrict__ X,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const float* __restrict__ slope, const float* __restrict__ sum_dz,
                                                                 const float* __restrict__ sum_dzx, float inv_cnt,
                                                                 float* __restrict__ dX, long n4, int C4) {
  const float a = slope[0];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C4) * 4;
    const float4 mu = ld4(mean + c), is = ld4(invstd + c), ga = ld4(gamma + c), be = ld4(beta + c);
    const float4 s_a = ld4(sum_dz + c), s_b = ld4(sum_dzx + c);
    const float4 x = ld4(X + i * 4), dy = ld4(dY + i * 4);
    const float xv[4] = {x.x, x.y, x.z, x.w}, gv[4] = {dy.x, dy.y, dy.z, dy.w};
    const float muv[4] = {mu.x, mu.y, mu.z, mu.w}, isv[4] = {is.x, is.y, is.z, is.w}, gav[4] = {ga.x, ga.y, ga.z, ga.w};
    const float bev[4] = {be.x, be.y, be.z, be.w}, av[4] = {s_a.x, s_a.y, s_a.z, s_a.w}, bv[4] = {s_b.x, s_b.y, s_b.z, s_b.w};
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float k1 = gav[k] * isv[k], k2 = av[k] * inv_cnt, k3 = isv[k] * bv[k] * inv_cnt;
      const float z = (xv[k] - muv[k]) * k1 + bev[k];
      const float dz = z > 0.f ? gv[k] : a * gv[k];
      o[k] = k1 * (dz - k2 - (xv[k] - muv[k]) * k3);
    }
    st4(dX + i * 4, make_float4(o[0], o[1], o[2], o[3]));
  }
}

// ------------------------------------------------------------------------------------------------ upsample (+ skip)
// Up[b,oy,ox,:] = bilinear(X)  (resize_fwd_kernel's expression per channel, csrc/heads.hip);  Sum = Up + Skip
__global__ __launch_bounds__(256) void upsample_nhwc_fwd_kernel(const float* __restrict__ X, const float* __restrict__ Skip,
                                                                float* __restrict__ Up, float* __restrict__ Sum, int B, int Hi,
                                                                int Wi, int Ho, int Wo, int C4) {
  const long n = (long)B * Ho * Wo * C4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int cv = (int)(i % C4);
    long t = i / C4;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho);
    const long b = t / Ho;
    const Lerp ly = lerp_of(oy, Hi, Ho, 0), lx = lerp_of(ox, Wi, Wo, 0);
    const float* p = X + b * Hi * Wi * (long)C4 * 4 + cv * 4;
    const long C = (long)C4 * 4;
    const float4 v00 = ld4(p + ((long)ly.i0 * Wi + lx.i0) * C), v01 = ld4(p + ((long)ly.i0 * Wi + lx.i1) * C);
    const float4 v10 = ld4(p + ((long)ly.i1 * Wi + lx.i0) * C), v11 = ld4(p + ((long)ly.i1 * Wi + lx.i1) * C);
    float4 top, bot, y;
    top.x = v00.x + lx.w1 * (v01.x - v00.x); bot.x = v10.x + lx.w1 * (v11.x - v10.x); y.x = top.x + ly.w1 * (bot.x - top.x);
    top.y = v00.y + lx.w1 * (v01.y - v00.y); bot.y = v10.y + lx.w1 * (v11.y - v10.y); y.y = top.y + ly.w1 * (bot.y - top.y);
    top.z = v00.z + lx.w1 * (v01.z - v00.z); bot.z = v10.z + lx.w1 * (v11.z - v10.z); y.z = top.z + ly.w1 * (bot.z - top.z);
    top.w = v00.w + lx.w1 * (v01.w - v00.w); bot.w = v10.w + lx.w1 * (v11.w - v10.w); y.w = top.w + ly.w1 * (bot.w - top.w);
    if (Up) st4(Up + i * 4, y);
    if (Sum) {
      const float4 s = ld4(Skip + i * 4);
      st4(Sum + i * 4, make_float4(y.x + s.x, y.y + s.y, y.z + s.z, y.w + s.w));
    }
  }
}
// gather form: one thread per INPUT pixel and channel vector sums the output window that samples it (resize_bwd_kernel's
// loop order); the incoming gradient of an output pixel is dUp + dSum (either may be absent)
__global__ __launch_bounds__(256) void upsample_nhwc_bwd_kernel(const float* __restrict__ dUp, const float* __restrict__ dSum,
                                                                float* __restrict__ dX, int B, int Hi, int Wi, int Ho, int Wo,
                                                                int C4) {
  const long n = (long)B * Hi * Wi * C4;
  const long C = (long)C4 * 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int cv = (int)(i % C4);
    long t = i / C4;
    const int x = (int)(t % Wi);
    t /= Wi;
    const int y = (int)(t % Hi);
    const long b = t / Hi;
    int ylo, yhi, xlo, xhi;
    window(y, Hi, Ho, 0, ylo, yhi);
    window(x, Wi, Wo, 0, xlo, xhi);
    const long base = b * Ho * Wo * C + cv * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int oy = ylo; oy <= yhi; ++oy) {
      const float wy = contrib(oy, Hi, Ho, 0, y);
      if (wy == 0.f) continue;
      float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int ox = xlo; ox <= xhi; ++ox) {
        const float wx = contrib(ox, Wi, Wo, 0, x);
        const long o = base + ((long)oy * Wo + ox) * C;
        float4 g = dUp ? ld4(dUp + o) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (dSum) {
          const float4 s = ld4(dSum + o);
          g = dUp ? make_float4(g.x + s.x, g.y + s.y, g.z + s.z, g.w + s.w) : s;
        }
        row.x += wx * g.x; row.y += wx * g.y; row.z += wx * g.z; row.w += wx * g.w;
      }
      acc.x += wy * row.x; acc.y += wy * row.y; acc.z += wy * row.z; acc.w += wy * row.w;
    }
    st4(dX + i * 4, acc);
  }
}

// ------------------------------------------------------------------------------------------------ 1x1 head, C -> 1
// 8 lanes per row (C % 32 == 0): lane l holds channels [4l, 4l+4) + 32 k; butterfly sum over the 8 lanes (fixed order)
__global__ __launch_bounds__(256) void head1_fwd_kernel(const float* __restrict__ X, const float* __restrict__ w,
                                                        float* __restrict__ Y, long M, int C) {
  const int l = threadIdx.x & 7;
  for (long r = ((long)blockIdx.x * 256 + threadIdx.x) >> 3; r < M; r += ((long)gridDim.x * 256) >> 3) {
    float s = 0.f;
    for (int c = l * 4; c < C; c += 32) {
      const float4 x = ld4(X + r * C + c), ww = ld4(w + c);
      s += x.x * ww.x + x.y * ww.y + x.z * ww.z + x.w * ww.w;
    }
    s += __shfl_xor(s, 1, 8);
    s += __shfl_xor(s, 2, 8);
    s += __shfl_xor(s, 4, 8);
    if (l == 0) Y[r] = s;
  }
}
// dX = g (x) w; partial column sums of g * X (the weight gradient), layout part[blk][C]
__global__ __launch_bounds__(256) void head1_bwd_kernel(const float* __restrict__ G, const float* __restrict__ X,
                                                        const float* __restrict__ w, float* __restrict__ dX, long M, int C,
                                                        long rpb, double* __restrict__ part) {
  __shared__ double s0[256][4];
  const int CV = C >> 2, RS = 256 / CV, tid = threadIdx.x;
  const int cv = tid % CV, ro = tid / CV, c = cv * 4;
  const float4 ww = ld4(w + c);
  double d[4] = {0, 0, 0, 0};
  const long rbeg = (long)blockIdx.x * rpb, rend = min(M, rbeg + rpb);
  for (long r = rbeg + ro; r < rend; r += RS) {
    const float g = G[r];
    const float4 x = ld4(X + r * C + c);
    st4(dX + r * C + c, make_float4(g * ww.x, g * ww.y, g * ww.z, g * ww.w));
    d[0] += (double)g * x.x; d[1] += (double)g * x.y; d[2] += (double)g * x.z; d[3] += (double)g * x.w;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) s0[tid][k] = d[k];
  __syncthreads();
  if (ro == 0) {
    double t[4] = {0, 0, 0, 0};
    for (int q = 0; q < RS; ++q)
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] += s0[q * CV + cv][k];
#pragma unroll
    for (int k = 0; k < 4; ++k) part[(long)blockIdx.x * C + c + k] = t[k];
  }
}

// ------------------------------------------------------------------------------------------------ BCE with logits, 4 heads
struct Heads4 { const float* x[4]; };
struct Grads4 { float* d[4]; };
__device__ __forceinline__ float target_at(const void* __restrict__ T, int t_f32, long i) {
  return t_f32 ? reinterpret_cast<const float*>(T)[i] : (float)reinterpret_cast<const long*>(T)[i];
}
// blockIdx.y = head; part[head][blk] = fp64 sum over the block's elements of max(x,0) - x t + log1p(exp(-|x|)) (0 for an absent head)
__global__ __launch_bounds__(256) void bce4_fwd_kernel(Heads4 h, const void* __restrict__ T, int t_f32, long n, double* __restrict__ part) {
  __shared__ double red[256];
  const float* __restrict__ X = h.x[blockIdx.y];
  double s = 0.0;
  if (X != nullptr)
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
      const float x = X[i], t = target_at(T, t_f32, i);
      s += (double)(fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x))));
    }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}
// losses = {l1 + l2 + l3 + l4, l1, l2, l3, l4}  (train_stage2.py:314-319; the means of criterion, model_stage2.py:139-141)
__global__ void bce4_finalize_kernel(const double* __restrict__ part, int nb, long n, float* __restrict__ losses) {
  if (threadIdx.x != 0) return;
  float l[4];
  for (int k = 0; k < 4; ++k) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[(long)k * nb + b];
    l[k] = (float)(s / (double)n);
    losses[1 + k] = l[k];
  }
  losses[0] = ((l[0] + l[1]) + l[2]) + l[3];
}
// dX_k = (sigmoid(x) - t) * (g[0] + g[1 + k]) / n  (absent heads skipped)
__global__ __launch_bounds__(256) void bce4_bwd_kernel(Heads4 h, Grads4 d, const void* __restrict__ T, int t_f32,
                                                       const float* __restrict__ g, long n) {
  const int k = blockIdx.y;
  const float* __restrict__ X = h.x[k];
  float* __restrict__ D = d.d[k];
  if (X == nullptr || D == nullptr) return;
  const float gk = (g[0] + g[1 + k]) / (float)n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float x = X[i];
    D[i] = (1.0f / (1.0f + expf(-x)) - target_at(T, t_f32, i)) * gk;
  }
}

// ------------------------------------------------------------------------------------------------ BCE + EMA consistency, 4 heads
// One pass over x_k, the teacher map e_k and the target.  A thread owns whole quads (elements 4q .. 4q+3); VEC reads a quad as
// one 16-byte word, !VEC (a base pointer that is not 16-byte aligned) as four 4-byte words: the element order, and with it every
// sum, is the same.  The n % 4 last elements go to the first threads of block 0.
template <bool VEC>
__device__ __forceinline__ void quad_f32(const float* __restrict__ p, long q, float (&v)[4]) {
  if (VEC) {
    const float4 t = ld4(p + q * 4);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = p[q * 4 + j];
  }
}
template <bool VEC>
__device__ __forceinline__ void quad_target(const void* __restrict__ T, int t_f32, long q, float (&v)[4]) {
  if (t_f32) {
    quad_f32<VEC>(reinterpret_cast<const float*>(T), q, v);
  } else if (VEC) {
    const longlong2* p = reinterpret_cast<const longlong2*>(T) + q * 2;
    const longlong2 a = p[0], b = p[1];
    v[0] = (float)a.x; v[1] = (float)a.y; v[2] = (float)b.x; v[3] = (float)b.y;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (float)reinterpret_cast<const long*>(T)[q * 4 + j];
  }
}
__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }   // (bce4_bwd_kernel's expression)
__device__ __forceinline__ void loss5_elem(float x, float e, float t, double& bce, double& mse) {
  bce += (double)(fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x))));    // (bce4_fwd_kernel's expression)
  const double d = (double)sigmoid_f32(x) - (double)sigmoid_f32(e);
  mse += d * d;
}
// blockIdx.y = head; part[2 * head + {0: BCE, 1: consistency}][blk] = fp64 sums over the block's elements (0 for an absent head)
template <bool VEC>
__global__ __launch_bounds__(256) void loss5_fwd_kernel(Heads4 h, Heads4 ema, const void* __restrict__ T, int t_f32, long n,
                                                        double* __restrict__ part) {
  __shared__ double red0[256], red1[256];
  const float* __restrict__ X = h.x[blockIdx.y];
  const float* __restrict__ E = ema.x[blockIdx.y];
  double s0 = 0.0, s1 = 0.0;
  if (X != nullptr) {
    const long n4 = n >> 2;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long)gridDim.x * 256) {
      float x[4], e[4], t[4];
      quad_f32<VEC>(X, q, x);
      quad_f32<VEC>(E, q, e);
      quad_target<VEC>(T, t_f32, q, t);
#pragma unroll
      for (int j = 0; j < 4; ++j) loss5_elem(x[j], e[j], t[j], s0, s1);
    }
    const long i = n4 * 4 + threadIdx.x;
    if (blockIdx.x == 0 && i < n) loss5_elem(X[i], E[i], target_at(T, t_f32, i), s0, s1);
  }
  red0[threadIdx.x] = s0;
  red1[threadIdx.x] = s1;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red0[threadIdx.x] += red0[threadIdx.x + o];
      red1[threadIdx.x] += red1[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[(long)(2 * blockIdx.y) * gridDim.x + blockIdx.x] = red0[0];
    part[(long)(2 * blockIdx.y + 1) * gridDim.x + blockIdx.x] = red1[0];
  }
}
// losses = {l1 + l2 + l3 + l4 + l5, l1, l2, l3, l4, l5}, l5 = the four consistency means summed (train_stage2.py:305-319)
__global__ void loss5_finalize_kernel(const double* __restrict__ part, int nb, long n, float* __restrict__ losses) {
  if (threadIdx.x != 0) return;
  float l[4], m[4];
  for (int k = 0; k < 4; ++k) {
    double s = 0.0, c = 0.0;
    for (int b = 0; b < nb; ++b) { s += part[(long)(2 * k) * nb + b]; c += part[(long)(2 * k + 1) * nb + b]; }
    l[k] = (float)(s / (double)n);
    m[k] = (float)(c / (double)n);
    losses[1 + k] = l[k];
  }
  const float l5 = ((m[0] + m[1]) + m[2]) + m[3];
  losses[5] = l5;
  losses[0] = (((l[0] + l[1]) + l[2]) + l[3]) + l5;
}
// dX_k = (sigmoid(x) - t) * (g[0] + g[1 + k]) / n  [bce4_bwd_kernel's value]  + 2 (s - sigmoid(e)) s (1 - s) * (g[0] + g[5]) / n
__device__ __forceinline__ float loss5_grad(float x, float e, float t, float gk, float gc) {
#pragma clang fp contract(off)   // (the sum is not fused into the product before it: with e == x it is the BCE term's bits)
  const float s = sigmoid_f32(x);
  const float bce = (s - t) * gk;
  const float c = ((2.0f * (s - sigmoid_f32(e))) * (s * (1.0f - s))) * gc;
  return bce + c;
}
template <bool VEC>
__global__ __launch_bounds__(256) void loss5_bwd_kernel(Heads4 h, Heads4 ema, Grads4 d, const void* __restrict__ T, int t_f32,
                                                        const float* __restrict__ g, long n) {
  const int k = blockIdx.y;
  const float* __restrict__ X = h.x[k];
  const float* __restrict__ E = ema.x[k];
  float* __restrict__ D = d.d[k];
  if (X == nullptr || D == nullptr) return;
  const float gk = (g[0] + g[1 + k]) / (float)n, gc = (g[0] + g[5]) / (float)n;
  const long n4 = n >> 2;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long)gridDim.x * 256) {
    float x[4], e[4], t[4], o[4];
    quad_f32<VEC>(X, q, x);
    quad_f32<VEC>(E, q, e);
    quad_target<VEC>(T, t_f32, q, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = loss5_grad(x[j], e[j], t[j], gk, gc);
    if (VEC) {
      st4(D + q * 4, make_float4(o[0], o[1], o[2], o[3]));
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) D[q * 4 + j] = o[j];
    }
  }
  const long i = n4 * 4 + threadIdx.x;
  if (blockIdx.x == 0 && i < n) D[i] = loss5_grad(X[i], E[i], target_at(T, t_f32, i), gk, gc);
}

inline int loss5_blocks(long n) {      // quads per block: 64 at least, 512 blocks per head at most
  const long nb = ((n >> 2) + 63) / 64;
  return (int)(nb < SEG_BLOCKS ? (nb < 1 ? 1 : nb) : SEG_BLOCKS);
}
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ------------------------------------------------------------------------------------------------ lerp (the mean teacher's update)
// torch's lerp in fp32, each operation rounded on its own; w == 0 / w == 1 return an operand untouched (signed zeros included)
__device__ __forceinline__ float lerp_f32(float a, float b, float w) {
#pragma clang fp contract(off)
  if (w == 0.f) return a;
  if (w == 1.f) return b;
  const float d = b - a;
  return w < 0.5f ? a + w * d : b - d * (1.0f - w);
}
// dst[0, n) by threads tid, tid + nt, ...: where dst and src sit at the same offset inside a 16-byte line, the elements up to
// the next line are peeled, the body goes in 16-byte words and the rest one by one; otherwise everything goes one by one
__device__ __forceinline__ void lerp_range(float* __restrict__ dst, const float* __restrict__ src, long n, float w, long tid,
                                           long nt) {
  const unsigned od = (unsigned)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3), os = (unsigned)((reinterpret_cast<uintptr_t>(src) >> 2) & 3);
  if (od != os) {
    for (long i = tid; i < n; i += nt) dst[i] = lerp_f32(dst[i], src[i], w);
    return;
  }
  long head = (4 - od) & 3;
  if (head > n) head = n;
  const long n4 = (n - head) >> 2, tail = head + n4 * 4;
  for (long q = tid; q < n4; q += nt) {
    const float4 a = ld4(dst + head + q * 4), b = ld4(src + head + q * 4);
    st4(dst + head + q * 4, make_float4(lerp_f32(a.x, b.x, w), lerp_f32(a.y, b.y, w), lerp_f32(a.z, b.z, w), lerp_f32(a.w, b.w, w)));
  }
  if (tid < head) dst[tid] = lerp_f32(dst[tid], src[tid], w);
  for (long i = tail + tid; i < n; i += nt) dst[i] = lerp_f32(dst[i], src[i], w);
}
__global__ __launch_bounds__(256) void lerp_kernel(float* __restrict__ dst, const float* __restrict__ src, long n, float w) {
  lerp_range(dst, src, n, w, (long)blockIdx.x * 256 + threadIdx.x, (long)gridDim.x * 256);
}
struct LerpRec { float* dst; const float* src; long n; };
__global__ __launch_bounds__(256) void lerp_table_kernel(const LerpRec* __restrict__ table, int count, float w) {
  for (int r = blockIdx.x; r < count; r += gridDim.x) {
    const LerpRec rec = table[r];
    lerp_range(rec.dst, rec.src, rec.n, w, threadIdx.x, 256);
  }
}

// ------------------------------------------------------------------------------------------------ signed evaluation
// validate.py:179-191 as written: pred = bilinear_ac(map); pred /= max(pred) + 1e-5 (whatever its sign); mask = pred > 1e-9;
// hit point = first arg-max of the NORMALISED map (np.argmax).  ws layout (floats): [0, 2*1024) max partials | [2048] max |
// [2049 ..) per-block {I, U, best value, best index} of the count pass.
__global__ __launch_bounds__(256) void seval_max_kernel(const float* __restrict__ m, int S, int oH, int oW, float* __restrict__ ws) {
  __shared__ float sv[256];
  const long n = (long)oH * oW;
  float best = -INFINITY;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    best = fmaxf(best, sample_ac(m, S, oH, oW, (int)(i / oW), (int)(i % oW)));
  sv[threadIdx.x] = best;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sv[threadIdx.x] = fmaxf(sv[threadIdx.x], sv[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) ws[blockIdx.x] = sv[0];
}
__global__ void seval_max_final_kernel(float* __restrict__ ws, int nb) {
  if (threadIdx.x != 0) return;
  float best = -INFINITY;
  for (int b = 0; b < nb; ++b) best = fmaxf(best, ws[b]);
  ws[2048] = best;
}
__global__ __launch_bounds__(256) void seval_count_kernel(const float* __restrict__ m, int S, const unsigned char* __restrict__ target,
                                                          int oH, int oW, float* __restrict__ cam, float* __restrict__ ws) {
  __shared__ int ri[256], ru[256], bi[256];
  __shared__ float bv[256];
  const float denom = ws[2048] + 1e-5f;
  const long n = (long)oH * oW;
  int I = 0, U = 0, besti = 0x7fffffff;
  float best = -INFINITY;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = sample_ac(m, S, oH, oW, (int)(i / oW), (int)(i % oW)) / denom;
    if (cam) cam[i] = v;
    const bool p = v > 1e-9f, t = target[i] != 0;
    I += (p && t) ? 1 : 0;
    U += (p || t) ? 1 : 0;
    if (v > best) { best = v; besti = (int)i; }   // (increasing i: the first index of the thread's maximum)
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
    float* o = ws + 2049 + 4 * blockIdx.x;
    o[0] = __int_as_float(ri[0]);
    o[1] = __int_as_float(ru[0]);
    o[2] = bv[0];
    o[3] = __int_as_float(bi[0]);
  }
}
__global__ void seval_final_kernel(const float* __restrict__ ws, int nb, long* __restrict__ out_iu) {
  if (threadIdx.x != 0) return;
  long I = 0, U = 0;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int b = 0; b < nb; ++b) {
    const float* o = ws + 2049 + 4 * b;
    I += __float_as_int(o[0]);
    U += __float_as_int(o[1]);
    const int i = __float_as_int(o[3]);
    if (o[2] > best || (o[2] == best && i < bi)) { best = o[2]; bi = i; }
  }
  out_iu[0] = I;
  out_iu[1] = U;
  out_iu[2] = bi == 0x7fffffff ? 0 : bi;   // (an all-NaN map: index 0, as np.argmax)
}

inline bool seg_c_ok(int C) { return C >= 4 && C <= 1024 && 1024 % C == 0; }

}  // namespace

extern "C" long tris_seg_workspace_bytes(long M, int C) {
  return (long)red_blocks(M) * (2L * C + 1) * (long)sizeof(double);
}

extern "C" int tris_bn_prelu_fwd_f32(const float* X, const float* mean, const float* invstd, const float* gamma, const float* beta,
                                     const float* slope, float* Y, long M, int C, void* stream) {
  if (C % 4) return (int)hipErrorInvalidValue;
  const long n4 = M * C / 4;
  hipLaunchKernelGGL(bn_prelu_fwd_kernel, dim3(seg_grid(n4)), dim3(256), 0, (hipStream_t)stream, X, mean, invstd, gamma, beta, slope,
                     Y, n4, C / 4);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_bn_prelu_bwd_reduce_f32(const float* dY, const float* X, const float* mean, const float* invstd,
                                            const float* gamma, const float* beta, const float* slope, long M, int C, float* sum_dz,
                                            float* sum_dzx, float* dslope, double* workspace, void* stream) {
  if (!seg_c_ok(C) || M < 1) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int nb = red_blocks(M);
  const long rpb = (M + nb - 1) / nb;
  hipLaunchKernelGGL(bn_prelu_bwd_partial_kernel, dim3(nb), dim3(256), 0, st, dY, X, mean, invstd, gamma, beta, slope, M, C, rpb,
                     workspace);
  TRIS_LAUNCH_CHECK();
  const int W = 2 * C + 1;
  hipLaunchKernelGGL(seg_part_finalize_kernel, dim3(cdiv(W, 256)), dim3(256), 0, st, (const double*)workspace, nb, C, W, sum_dz,
                     sum_dzx, dslope);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_bn_prelu_bwd_apply_f32(const float* dY, const float* X, const float* mean, const float* invstd, const float* gamma,
                                           const float* beta, const float* slope, const float* sum_dz, const float* sum_dzx,
                                           float inv_count, float* dX, long M, int C, void* stream) {
  if (C % 4) return (int)hipErrorInvalidValue;
  const long n4 = M * C / 4;
  hipLaunchKernelGGL(bn_prelu_bwd_apply_kernel, dim3(seg_grid(n4)), dim3(256), 0, (hipStream_t)stream, dY, X, mean, invstd, gamma,
                     beta, slope, sum_dz, sum_dzx, inv_count, dX, n4, C / 4);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_upsample_nhwc_fwd_f32(const float* X, const float* skip, float* up, float* sum, int B, int Hi, int Wi, int Ho,
                                          int Wo, int C, void* stream) {
  if (C % 4 || (up == nullptr && sum == nullptr) || ((sum == nullptr) != (skip == nullptr)) || Hi < 1 || Wi < 1)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(upsample_nhwc_fwd_kernel, dim3(seg_grid((long)B * Ho * Wo * (C / 4))), dim3(256), 0, (hipStream_t)stream, X, skip,
                     up, sum, B, Hi, Wi, Ho, Wo, C / 4);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_upsample_nhwc_bwd_f32(const float* d_up, const float* d_sum, float* dX, int B, int Hi, int Wi, int Ho, int Wo,
                                          int C, void* stream) {
  if (C % 4 || (d_up == nullptr && d_sum == nullptr) || Ho < Hi || Wo < Wi) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(upsample_nhwc_bwd_kernel, dim3(seg_grid((long)B * Hi * Wi * (C / 4))), dim3(256), 0, (hipStream_t)stream, d_up,
                     d_sum, dX, B, Hi, Wi, Ho, Wo, C / 4);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_head1_fwd_f32(const float* X, const float* w, float* Y, long M, int C, void* stream) {
  if (C % 32 || !seg_c_ok(C)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(head1_fwd_kernel, dim3(seg_grid(M * 8)), dim3(256), 0, (hipStream_t)stream, X, w, Y, M, C);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_head1_bwd_f32(const float* g, const float* X, const float* w, float* dX, float* dw, long M, int C,
                                  double* workspace, void* stream) {
  if (C % 32 || !seg_c_ok(C) || M < 1) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int nb = red_blocks(M);
  const long rpb = (M + nb - 1) / nb;
  hipLaunchKernelGGL(head1_bwd_kernel, dim3(nb), dim3(256), 0, st, g, X, w, dX, M, C, rpb, workspace);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_part_finalize_kernel, dim3(cdiv(C, 256)), dim3(256), 0, st, (const double*)workspace, nb, C, C, dw, nullptr,
                     nullptr);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" long tris_bce4_workspace_bytes(long n) { return 4L * red_blocks(n) * (long)sizeof(double); }

extern "C" int tris_bce4_fwd_f32(const float* x1, const float* x2, const float* x3, const float* x4, const void* target, int target_f32,
                                 long n, float* losses, double* workspace, void* stream) {
  if (n < 1 || x1 == nullptr) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  Heads4 h = {{x1, x2, x3, x4}};
  const int nb = red_blocks(n);
  hipLaunchKernelGGL(bce4_fwd_kernel, dim3(nb, 4), dim3(256), 0, st, h, target, target_f32, n, workspace);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(bce4_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)workspace, nb, n, losses);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_bce4_bwd_f32(const float* x1, const float* x2, const float* x3, const float* x4, const void* target,
                                 int target_f32, const float* g, float* d1, float* d2, float* d3, float* d4, long n, void* stream) {
  if (n < 1) return (int)hipErrorInvalidValue;
  Heads4 h = {{x1, x2, x3, x4}};
  Grads4 d = {{d1, d2, d3, d4}};
  hipLaunchKernelGGL(bce4_bwd_kernel, dim3(seg_grid(n), 4), dim3(256), 0, (hipStream_t)stream, h, d, target, target_f32, g, n);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" long tris_seg_loss5_workspace_bytes(long n) { return 8L * loss5_blocks(n) * (long)sizeof(double); }

extern "C" int tris_seg_loss5_fwd_f32(const float* x1, const float* x2, const float* x3, const float* x4, const float* e1,
                                      const float* e2, const float* e3, const float* e4, const void* target, int target_f32, long n,
                                      float* losses, double* workspace, void* stream) {
  if (n < 1 || x1 == nullptr || target == nullptr) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  Heads4 h = {{x1, x2, x3, x4}}, ema = {{e1, e2, e3, e4}};
  bool vec = aligned16(target);
  for (int k = 0; k < 4; ++k) {
    if ((h.x[k] == nullptr) != (ema.x[k] == nullptr)) return (int)hipErrorInvalidValue;
    vec = vec && aligned16(h.x[k]) && aligned16(ema.x[k]);
  }
  const int nb = loss5_blocks(n);
  if (vec) hipLaunchKernelGGL(loss5_fwd_kernel<true>, dim3(nb, 4), dim3(256), 0, st, h, ema, target, target_f32, n, workspace);
  else hipLaunchKernelGGL(loss5_fwd_kernel<false>, dim3(nb, 4), dim3(256), 0, st, h, ema, target, target_f32, n, workspace);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss5_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)workspace, nb, n, losses);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_seg_loss5_bwd_f32(const float* x1, const float* x2, const float* x3, const float* x4, const float* e1,
                                      const float* e2, const float* e3, const float* e4, const void* target, int target_f32,
                                      const float* g, float* d1, float* d2, float* d3, float* d4, long n, void* stream) {
  if (n < 1 || target == nullptr || g == nullptr) return (int)hipErrorInvalidValue;
  Heads4 h = {{x1, x2, x3, x4}}, ema = {{e1, e2, e3, e4}};
  Grads4 d = {{d1, d2, d3, d4}};
  bool vec = aligned16(target);
  for (int k = 0; k < 4; ++k) {
    if (h.x[k] != nullptr && ema.x[k] == nullptr) return (int)hipErrorInvalidValue;
    vec = vec && aligned16(h.x[k]) && aligned16(ema.x[k]) && aligned16(d.d[k]);
  }
  const dim3 grid(loss5_blocks(n), 4);
  if (vec) hipLaunchKernelGGL(loss5_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, h, ema, d, target, target_f32, g, n);
  else hipLaunchKernelGGL(loss5_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, h, ema, d, target, target_f32, g, n);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_lerp_f32(float* dst, const float* src, long n, float w, void* stream) {
  if (n < 0 || (n > 0 && (dst == nullptr || src == nullptr || dst == src))) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const long g = (n / 4 + 255) / 256;        // one 16-byte word per thread, 2048 blocks at most
  hipLaunchKernelGGL(lerp_kernel, dim3((unsigned)(g < 1 ? 1 : (g < 2048 ? g : 2048))), dim3(256), 0, (hipStream_t)stream, dst, src, n, w);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_lerp_table_f32(const long* table, int count, float w, void* stream) {
  if (count < 0 || (count > 0 && table == nullptr)) return (int)hipErrorInvalidValue;
  if (count == 0) return 0;
  hipLaunchKernelGGL(lerp_table_kernel, dim3((unsigned)(count < 2048 ? count : 2048)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const LerpRec*>(table), count, w);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_eval_post_signed_f32(const float* map, int S, const unsigned char* target, int oH, int oW, float* cam,
                                         long* out_iu, float* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const long n = (long)oH * oW;
  if (n < 1 || S < 1) return (int)hipErrorInvalidValue;
  int nb = (int)((n + 255) / 256);
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(seval_max_kernel, dim3(nb), dim3(256), 0, st, map, S, oH, oW, workspace);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(seval_max_final_kernel, dim3(1), dim3(64), 0, st, workspace, nb);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(seval_count_kernel, dim3(nb), dim3(256), 0, st, map, S, target, oH, oW, cam, workspace);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(seval_final_kernel, dim3(1), dim3(64), 0, st, (const float*)workspace, nb, out_iu);
  TRIS_LAUNCH_CHECK();
  return 0;
}
