// IRNet edge / displacement heads, training (gfx950): the backward of what irnnet.hip computes for the two branches of
// IRNet/net/resnet50_irn.py.  The trunk is frozen and its taps are detached there (:117-121), so only the branches need one:
//   * GroupNorm -> bilinear upsample (x1 / x2 / x4) -> crop -> ReLU, the adjoint of gn_apply_up_kernel: pass A gathers the masked
//     output gradient through the adjoint of the blend (an input pixel collects from at most 2 * scale outputs per axis; outputs
//     beyond the crop do not exist) and leaves fp64 partial sums per (image, row block, channel) in gn_partial_kernel's block layout;
//     a finalize sums them in index order into dgamma, dbeta and the two means of every (image, group); pass B forms the gradient of
//     the GroupNorm input in place
//   * the narrow heads (C -> 1 | 2): the data gradient over the whole concatenation buffer, weight and bias gradients from fp64
//     block partials summed in index order
// The 1x1 products' weight and data gradients run on the GEMM paths (gemm_conv.hip).  No atomics: every launch is bitwise reproducible.
#include "common.h"
#include "tris_hip.h"
#include "bilinear.h"
#include "irn_gn.h"

namespace {

// ------------------------------------------------------------------------------------------ GroupNorm + upsample, backward
// Pass A.  grid (row blocks, B); 256 threads = RS rows x CV channel vectors of the INPUT map T [B][Hi*Wi][C].
// dU[b][r][c] = sum over the outputs (oy < Ho, ox < Wo) that blend input pixel r of wy wx (Y > 0 ? dY : 0);
// part[((b * nblk + blk) * C + c) * 2] = {sum dU, sum dU xhat} over the block's rows, xhat = (T - mean) invstd.
__global__ __launch_bounds__(256) void gn_up_bwd_gather_kernel(const float* __restrict__ dY, const float* __restrict__ Y, long ldy,
                                                               const float* __restrict__ T, const float* __restrict__ stats,
                                                               float* __restrict__ dT, float* __restrict__ dU, int Hi, int Wi, int C,
                                                               int G, int scale, int Ho, int Wo, long rpb, double* __restrict__ part) {
  __shared__ double sh[8][256];
  const int CV = C >> 2, RS = 256 / CV, tid = threadIdx.x;
  const int cv = tid % CV, ro = tid / CV;
  const long b = blockIdx.y, HW = (long)Hi * Wi;
  const long rbeg = (long)blockIdx.x * rpb, rend = min(HW, rbeg + rpb);
  const float* st = stats + (b * G + (cv * 4) / (C / G)) * 2;
  const float mean = st[0], is = st[1];
  const float* yb = Y + b * Ho * Wo * ldy + cv * 4;
  const float* gb = dY + b * Ho * Wo * ldy + cv * 4;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
  for (long r = rbeg + ro; r < rend; r += RS) {
    const int iy = (int)(r / Wi), ix = (int)(r - (long)iy * Wi);
    float4 du = make_float4(0.f, 0.f, 0.f, 0.f);
    if (scale == 1) {
      if (iy < Ho && ix < Wo) {
        const long o = ((long)iy * Wo + ix) * ldy;
        const float4 y = ld4(yb + o), g = ld4(gb + o);
        du.x = y.x > 0.f ? g.x : 0.f; du.y = y.y > 0.f ? g.y : 0.f; du.z = y.z > 0.f ? g.z : 0.f; du.w = y.w > 0.f ? g.w : 0.f;
      }
    } else {
      // src = (dst + 0.5) / scale - 0.5 lies in [i - 1, i + 1) for dst in [scale i - scale / 2, scale i + 3 scale / 2): exact for
      // scale = 2 | 4; the clamp at 0 adds nothing outside it.  contrib() is the forward's lerp_of: a pixel outside gets weight 0.
      const int ylo = max(scale * iy - scale / 2, 0), yhi = min(scale * iy + 3 * scale / 2 - 1, Ho - 1);
      const int xlo = max(scale * ix - scale / 2, 0), xhi = min(scale * ix + 3 * scale / 2 - 1, Wo - 1);
      for (int oy = ylo; oy <= yhi; ++oy) {
        const float wy = contrib(oy, Hi, Hi * scale, 0, iy);
        if (wy == 0.f) continue;
        for (int ox = xlo; ox <= xhi; ++ox) {
          const float wgt = wy * contrib(ox, Wi, Wi * scale, 0, ix);
          const long o = ((long)oy * Wo + ox) * ldy;
          const float4 y = ld4(yb + o), g = ld4(gb + o);
          du.x = y.x > 0.f ? fmaf(wgt, g.x, du.x) : du.x;
          du.y = y.y > 0.f ? fmaf(wgt, g.y, du.y) : du.y;
          du.z = y.z > 0.f ? fmaf(wgt, g.z, du.z) : du.z;
          du.w = y.w > 0.f ? fmaf(wgt, g.w, du.w) : du.w;
        }
      }
    }
    const long e = (b * HW + r) * C + cv * 4;
    st4(dT + e, du);
    if (dU) st4(dU + e, du);
    const float4 x = ld4(T + e);
    a0 += du.x; a1 += du.y; a2 += du.z; a3 += du.w;
    q0 += (double)du.x * (double)((x.x - mean) * is);
    q1 += (double)du.y * (double)((x.y - mean) * is);
    q2 += (double)du.z * (double)((x.z - mean) * is);
    q3 += (double)du.w * (double)((x.w - mean) * is);
  }
  sh[0][tid] = a0; sh[1][tid] = a1; sh[2][tid] = a2; sh[3][tid] = a3;
  sh[4][tid] = q0; sh[5][tid] = q1; sh[6][tid] = q2; sh[7][tid] = q3;
  __syncthreads();
  if (tid < CV) {
    double* o = part + ((b * gridDim.x + blockIdx.x) * C + tid * 4) * 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = 0.0, q = 0.0;
      for (int r = 0; r < RS; ++r) {
        s += sh[j][r * CV + tid];
        q += sh[4 + j][r * CV + tid];
      }
      o[j * 2] = s;
      o[j * 2 + 1] = q;
    }
  }
}

// grid B.  S[(b * C + c) * 2] = the block partials of (image, channel) summed in block order; means[(b * G + g) * 2] =
// {sum_c gamma_c S_du, sum_c gamma_c S_dux} / count over the group's channels in index order (the group sums of gamma dU and
// gamma dU xhat are linear in the channel sums: they are formed here, in fp64, not accumulated a second time in pass A).
__global__ __launch_bounds__(256) void gn_up_bwd_finalize_kernel(const double* __restrict__ part, int nblk, int C, int G,
                                                                 const float* __restrict__ gamma, double count,
                                                                 double* __restrict__ S, float* __restrict__ means) {
  __shared__ double sS[2 * 1024];
  const long b = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += 256) {
    double s = 0.0, q = 0.0;
    for (int k = 0; k < nblk; ++k) {
      const double* p = part + ((b * nblk + k) * C + c) * 2;
      s += p[0];
      q += p[1];
    }
    sS[2 * c] = s;
    sS[2 * c + 1] = q;
    S[(b * C + c) * 2] = s;
    S[(b * C + c) * 2 + 1] = q;
  }
  __syncthreads();
  const int cpg = C / G;
  for (int g = threadIdx.x; g < G; g += 256) {
    double m1 = 0.0, m2 = 0.0;
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
      m1 += (double)gamma[c] * sS[2 * c];
      m2 += (double)gamma[c] * sS[2 * c + 1];
    }
    means[(b * G + g) * 2] = (float)(m1 / count);
    means[(b * G + g) * 2 + 1] = (float)(m2 / count);
  }
}

// dgamma[c] = sum_b S_dux[b][c], dbeta[c] = sum_b S_du[b][c], images in index order
__global__ __launch_bounds__(256) void gn_up_bwd_params_kernel(const double* __restrict__ S, int B, int C, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int b = 0; b < B; ++b) {
    s += S[((long)b * C + c) * 2];
    q += S[((long)b * C + c) * 2 + 1];
  }
  dbeta[c] = (float)s;
  dgamma[c] = (float)q;
}

// Pass B, in place over dT = dU: dT = invstd (gamma dU - m1 - xhat m2)
__global__ __launch_bounds__(256) void gn_up_bwd_apply_kernel(float* __restrict__ dT, const float* __restrict__ T,
                                                              const float* __restrict__ stats, const float* __restrict__ gamma,
                                                              const float* __restrict__ means, long B, long HW, int C4, int G) {
  const long n = B * HW * C4;
  const int cpg = C4 * 4 / G;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int cv = (int)(i % C4);
    const long b = (i / C4) / HW;
    const long j = (b * G + (cv * 4) / cpg) * 2;
    const float mean = stats[j], is = stats[j + 1], m1 = means[j], m2 = means[j + 1];
    const float4 g = ld4(gamma + cv * 4), x = ld4(T + i * 4), du = ld4(dT + i * 4);
    float4 d;
    d.x = is * (g.x * du.x - m1 - ((x.x - mean) * is) * m2);
    d.y = is * (g.y * du.y - m1 - ((x.y - mean) * is) * m2);
    d.z = is * (g.z * du.z - m1 - ((x.z - mean) * is) * m2);
    d.w = is * (g.w * du.w - m1 - ((x.w - mean) * is) * m2);
    st4(dT + i * 4, d);
  }
}

// ------------------------------------------------------------------------------------------------ narrow heads, backward
constexpr int HEAD_BLOCKS = 1024;   // row blocks at most (fixed for a row count)

inline int head_blocks(long M) {
  long nb = (M + 63) / 64;
  return (int)(nb < HEAD_BLOCKS ? (nb < 1 ? 1 : nb) : HEAD_BLOCKS);
}

// dX[r][c] = sum_n g[r][n] w[n][c] (pitch C); part[blk][n * C + c] = sum over the block's rows of g[r][n] X[r][c],
// part[blk][N * C + n] = sum of g[r][n].  256 threads = RS rows x CV channel vectors, CV = C / 4 <= 64 (threads past RS * CV idle).
template <int N>
__global__ __launch_bounds__(256) void irn_head_bwd_kernel(const float* __restrict__ g, const float* __restrict__ X, long ldx,
                                                           const float* __restrict__ w, float* __restrict__ dX, long M, int C,
                                                           long rpb, double* __restrict__ part) {
  __shared__ double sh[N * 5][256];
  const int CV = C >> 2, RS = 256 / CV, tid = threadIdx.x;
  const int cv = tid % CV, ro = tid / CV;
  const long rbeg = (long)blockIdx.x * rpb, rend = min(M, rbeg + rpb);
  float4 wv[N];
  double a[N][4], bs[N];
#pragma unroll
  for (int n = 0; n < N; ++n) {
    wv[n] = ld4(w + n * C + cv * 4);
    a[n][0] = a[n][1] = a[n][2] = a[n][3] = bs[n] = 0.0;
  }
  if (ro < RS)
    for (long r = rbeg + ro; r < rend; r += RS) {
      const float4 x = ld4(X + r * ldx + cv * 4);
      float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int n = 0; n < N; ++n) {
        const float gn = g[r * N + n];
        d.x = fmaf(gn, wv[n].x, d.x); d.y = fmaf(gn, wv[n].y, d.y); d.z = fmaf(gn, wv[n].z, d.z); d.w = fmaf(gn, wv[n].w, d.w);
        a[n][0] += (double)gn * x.x; a[n][1] += (double)gn * x.y; a[n][2] += (double)gn * x.z; a[n][3] += (double)gn * x.w;
        bs[n] += gn;
      }
      st4(dX + r * C + cv * 4, d);
    }
#pragma unroll
  for (int n = 0; n < N; ++n) {
#pragma unroll
    for (int j = 0; j < 4; ++j) sh[n * 5 + j][tid] = a[n][j];
    sh[n * 5 + 4][tid] = bs[n];
  }
  __syncthreads();
  double* o = part + (long)blockIdx.x * (N * C + N);
  if (tid < CV) {
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double s = 0.0;
        for (int r = 0; r < RS; ++r) s += sh[n * 5 + j][r * CV + tid];
        o[n * C + tid * 4 + j] = s;
      }
  }
  if (tid < N) {   // the bias sums, from the threads of channel vector 0
    double s = 0.0;
    for (int r = 0; r < RS; ++r) s += sh[tid * 5 + 4][r * CV];
    o[N * C + tid] = s;
  }
}

// out[o] = sum over the blocks, in index order; o < n_w: dw, else db (may be NULL)
__global__ __launch_bounds__(256) void irn_head_bwd_finalize_kernel(const double* __restrict__ part, int nblk, int n_w, int n_b,
                                                                    float* __restrict__ dw, float* __restrict__ db) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= n_w + n_b) return;
  double s = 0.0;
  for (int k = 0; k < nblk; ++k) s += part[(long)k * (n_w + n_b) + o];
  if (o < n_w)
    dw[o] = (float)s;
  else if (db)
    db[o - n_w] = (float)s;
}

}  // namespace

extern "C" {

long tris_gn_up_bwd_workspace_bytes(int B, long HW, int C, int G) {
  if (B < 1 || HW < 1 || !gn_shape_ok(C, G)) return 0;
  // partials [B][nblk][C][2] fp64, channel sums [B][C][2] fp64, group means [B][G][2] fp32
  return ((long)B * gn_blocks(HW) * C * 2 + (long)B * C * 2) * (long)sizeof(double) + (long)B * G * 2 * (long)sizeof(float);
}

int tris_gn_up_bwd_f32(const float* dY, const float* Y, long ldy, const float* T, const float* stats, const float* gamma, float* dT,
                       float* dU, float* dgamma, float* dbeta, int B, int Hi, int Wi, int C, int G, int scale, int Ho, int Wo,
                       void* workspace, void* stream) {
  if (!gn_shape_ok(C, G) || ldy % 4 || ldy < C || (scale != 1 && scale != 2 && scale != 4) || B < 1 || B > 65535 || Hi < 1 || Wi < 1 ||
      Ho < 1 || Wo < 1 || Ho > Hi * scale || Wo > Wi * scale)
    return (int)hipErrorInvalidValue;
  if (!dY || !Y || !T || !stats || !gamma || !dT || !dgamma || !dbeta || !workspace) return (int)hipErrorInvalidValue;
  const long HW = (long)Hi * Wi;
  const int nblk = gn_blocks(HW);
  const long rpb = (HW + nblk - 1) / nblk;
  double* part = (double*)workspace;
  double* S = part + (long)B * nblk * C * 2;
  float* means = (float*)(S + (long)B * C * 2);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gn_up_bwd_gather_kernel, dim3(nblk, B), dim3(256), 0, st, dY, Y, ldy, T, stats, dT, dU, Hi, Wi, C, G, scale, Ho,
                     Wo, rpb, part);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_up_bwd_finalize_kernel, dim3(B), dim3(256), 0, st, part, nblk, C, G, gamma, (double)HW * (double)(C / G), S,
                     means);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_up_bwd_params_kernel, dim3(cdiv(C, 256)), dim3(256), 0, st, S, B, C, dgamma, dbeta);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_up_bwd_apply_kernel, dim3(ew_grid((long)B * HW * (C / 4))), dim3(256), 0, st, dT, T, stats, gamma, means,
                     (long)B, HW, C / 4, G);
  TRIS_LAUNCH_CHECK();
  return 0;
}

long tris_irn_head_bwd_workspace_bytes(long M, int C, int N) {
  if (M < 1 || C < 4 || (N != 1 && N != 2)) return 0;
  return (long)head_blocks(M) * (N * C + N) * (long)sizeof(double);
}

int tris_irn_head_bwd_f32(const float* g, const float* X, long ldx, const float* w, float* dX, float* dw, float* db, long M, int C,
                          int N, void* workspace, void* stream) {
  if (C % 32 || C > 256 || ldx % 4 || ldx < C || M < 1 || (N != 1 && N != 2)) return (int)hipErrorInvalidValue;
  if (!g || !X || !w || !dX || !dw || !workspace) return (int)hipErrorInvalidValue;
  const int nblk = head_blocks(M);
  const long rpb = (M + nblk - 1) / nblk;
  double* part = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (N == 1)
    hipLaunchKernelGGL(irn_head_bwd_kernel<1>, dim3(nblk), dim3(256), 0, st, g, X, ldx, w, dX, M, C, rpb, part);
  else
    hipLaunchKernelGGL(irn_head_bwd_kernel<2>, dim3(nblk), dim3(256), 0, st, g, X, ldx, w, dX, M, C, rpb, part);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(irn_head_bwd_finalize_kernel, dim3(cdiv(N * C + N, 256)), dim3(256), 0, st, part, nblk, N * C, N, dw, db);
  TRIS_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
