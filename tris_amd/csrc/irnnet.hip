// IRNet edge / displacement network, inference (gfx950): what the ResNet-50 trunk and the two branches of
// IRNet/net/resnet50_irn.py need beyond the dense products (those run on the GEMM / conv3x3 paths of gemm_conv.hip) and the frozen
// BatchNorm (tris_bn_apply_f32).  Channels-last activations throughout.
//   * stem: uint8 image -> normalise (256-entry table per channel) -> both flip rows -> 7x7 stride-2 pad-3 convolution 3 -> 64 ->
//     frozen BatchNorm -> ReLU, one direct vector-ALU kernel (K = 147 fits no MFMA K block, fp32 FMAs need no operand split, and
//     the layer is 2 % of the network's work: DESIGN.md section 10)
//   * MaxPool 3x3 stride 2 pad 1, row subsample (the strided 1x1 downsample's gather)
//   * GroupNorm: fixed-order fp64 partials per (image, row block, group) -> finalize -> apply, the apply fused with the bilinear
//     upsample (bilinear.h lerp_of), the crop, the ReLU and the write into a channel slice of the concatenation buffer
//   * the two narrow heads (C -> 1 with bias, C -> 2 with the mean shift as a bias) and the flip-average + sigmoid
// No atomics anywhere: every launch is bitwise reproducible.
#include "common.h"
#include "tris_hip.h"
#include "bilinear.h"
#include "irn_gn.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------ stem
constexpr int ST = 16;                 // output tile edge: 256 threads, one output pixel (64 channels) each
constexpr int SP = 2 * ST + 5;         // input patch edge
constexpr int SPW = SP * 3 + 1;        // patch row pitch in floats

// T = unsigned char: img uint8 [H][W][3]; lut [3][256]; Y [2][Ho][Wo][64], row 1 = the image flipped along W.
// T = float: img [B][H][W][3], already normalised (lut unused); Y [B][Ho][Wo][64], no flip row.  Wk [7][7][3][64].
template <typename T>
__global__ __launch_bounds__(256) void irn_stem_kernel(const T* __restrict__ img, const float* __restrict__ lut,
                                                       const float* __restrict__ Wk, const float* __restrict__ mean,
                                                       const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ Y, int H, int W,
                                                       int Ho, int Wo) {
  __shared__ float sw[147 * 64];
  __shared__ float sp[SP * SPW];
  const int tid = threadIdx.x, b = blockIdx.z;
  const int oy0 = blockIdx.y * ST, ox0 = blockIdx.x * ST;
  const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
  for (int i = tid; i < 147 * 16; i += 256) st4(sw + i * 4, ld4(Wk + i * 4));
  for (int i = tid; i < SP * SP; i += 256) {
    const int py = i / SP, px = i - py * SP;
    const int iy = iy0 + py, ix = ix0 + px;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
      if constexpr (sizeof(T) == 1) {
        const unsigned char* p = img + ((long)iy * W + (b ? W - 1 - ix : ix)) * 3;
        v0 = lut[p[0]];
        v1 = lut[256 + p[1]];
        v2 = lut[512 + p[2]];
      } else {
        const float* p = img + (((long)b * H + iy) * W + ix) * 3;
        v0 = p[0];
        v1 = p[1];
        v2 = p[2];
      }
    }
    float* d = sp + py * SPW + px * 3;
    d[0] = v0; d[1] = v1; d[2] = v2;
  }
  __syncthreads();
  const int ty = tid >> 4, tx = tid & 15;
  float4 acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
  for (int ky = 0; ky < 7; ++ky) {
    const float* prow = sp + (2 * ty + ky) * SPW + 2 * tx * 3;
#pragma unroll 1
    for (int kx = 0; kx < 7; ++kx) {
#pragma unroll
      for (int ci = 0; ci < 3; ++ci) {
        const float x = prow[kx * 3 + ci];
        const float* wr = sw + ((ky * 7 + kx) * 3 + ci) * 64;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float4 w = ld4(wr + j * 4);
          acc[j].x = fmaf(x, w.x, acc[j].x);
          acc[j].y = fmaf(x, w.y, acc[j].y);
          acc[j].z = fmaf(x, w.z, acc[j].z);
          acc[j].w = fmaf(x, w.w, acc[j].w);
        }
      }
    }
  }
  const int oy = oy0 + ty, ox = ox0 + tx;
  if (oy >= Ho || ox >= Wo) return;
  float* out = Y + (((long)b * Ho + oy) * Wo + ox) * 64;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float4 mu = ld4(mean + j * 4), is = ld4(invstd + j * 4), g = ld4(gamma + j * 4), be = ld4(beta + j * 4);
    float4 y;   // tris_bn_apply_f32's expression
    y.x = fmaxf((acc[j].x - mu.x) * (is.x * g.x) + be.x, 0.f);
    y.y = fmaxf((acc[j].y - mu.y) * (is.y * g.y) + be.y, 0.f);
    y.z = fmaxf((acc[j].z - mu.z) * (is.z * g.z) + be.z, 0.f);
    y.w = fmaxf((acc[j].w - mu.w) * (is.w * g.w) + be.w, 0.f);
    st4(out + j * 4, y);
  }
}

// --------------------------------------------------------------------------------------------------- MaxPool, subsample
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float* __restrict__ X, float* __restrict__ Y, int B, int H, int W,
                                                         int Ho, int Wo, int C4) {
  const long n = (long)B * Ho * Wo * C4;
  const long C = (long)C4 * 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int cv = (int)(i % C4);
    long t = i / C4;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho);
    const long b = t / Ho;
    const float ninf = -__builtin_huge_valf();
    float4 m = make_float4(ninf, ninf, ninf, ninf);
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = 2 * oy - 1 + ky;
      if (iy < 0 || iy >= H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = 2 * ox - 1 + kx;
        if (ix < 0 || ix >= W) continue;
        const float4 v = ld4(X + ((b * H + iy) * W + ix) * C + cv * 4);
        m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
      }
    }
    st4(Y + i * 4, m);
  }
}

__global__ __launch_bounds__(256) void subsample2_kernel(const float* __restrict__ X, float* __restrict__ Y, int B, int H, int W,
                                                         int Ho, int Wo, int C4) {
  const long n = (long)B * Ho * Wo * C4;
  const long C = (long)C4 * 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int cv = (int)(i % C4);
    long t = i / C4;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho);
    const long b = t / Ho;
    st4(Y + i * 4, ld4(X + ((b * H + 2 * oy) * W + 2 * ox) * C + cv * 4));
  }
}

// ------------------------------------------------------------------------------------------------------------ GroupNorm
// part[((b * nblk + blk) * G + g) * 2] = {sum, sum of squares} of the block's rows, fp64.  256 threads = RS rows x CV channel vectors.
__global__ __launch_bounds__(256) void gn_partial_kernel(const float* __restrict__ X, long HW, int C, int G, long rpb,
                                                         double* __restrict__ part) {
  __shared__ double s0[256];
  __shared__ double s1[256];
  const int CV = C >> 2, RS = 256 / CV, tid = threadIdx.x;
  const int cv = tid % CV, ro = tid / CV;
  const float* xb = X + (long)blockIdx.y * HW * C + cv * 4;
  const long rbeg = (long)blockIdx.x * rpb, rend = min(HW, rbeg + rpb);
  double a = 0.0, q = 0.0;
  for (long r = rbeg + ro; r < rend; r += RS) {
    const float4 x = ld4(xb + r * C);
    a += ((double)x.x + (double)x.y) + ((double)x.z + (double)x.w);
    q += ((double)x.x * x.x + (double)x.y * x.y) + ((double)x.z * x.z + (double)x.w * x.w);
  }
  s0[tid] = a;
  s1[tid] = q;
  __syncthreads();
  if (tid < G) {
    const int gv = CV / G;   // channel vectors per group
    double t0 = 0.0, t1 = 0.0;
    for (int r = 0; r < RS; ++r)
      for (int j = 0; j < gv; ++j) {
        t0 += s0[r * CV + tid * gv + j];
        t1 += s1[r * CV + tid * gv + j];
      }
    double* o = part + (((long)blockIdx.y * gridDim.x + blockIdx.x) * G + tid) * 2;
    o[0] = t0;
    o[1] = t1;
  }
}

// stats[(b * G + g) * 2] = {mean, 1 / sqrt(biased variance + eps)}.  One wave per (image, group): lane l sums the row blocks
// l, l + 64, ... in order, then a butterfly over the lanes -- a fixed order for a shape, so the statistics are reproducible
__global__ __launch_bounds__(64) void gn_finalize_kernel(const double* __restrict__ part, int nblk, int G, double count, double eps,
                                                         float* __restrict__ stats) {
  const int j = blockIdx.x, b = j / G, g = j - b * G;
  double s = 0.0, ss = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 64) {
    const double* p = part + (((long)b * nblk + k) * G + g) * 2;
    s += p[0];
    ss += p[1];
  }
  s = wave_sum_f64(s);
  ss = wave_sum_f64(ss);
  if (threadIdx.x != 0) return;
  const double mean = s / count;
  double var = ss / count - mean * mean;
  if (var < 0.0) var = 0.0;
  stats[j * 2] = (float)mean;
  stats[j * 2 + 1] = (float)(1.0 / sqrt(var + eps));
}

struct GnCoef { float4 mu, sc, be; };
__device__ __forceinline__ float4 gn_one(const float4 x, const GnCoef& k) {
  return make_float4((x.x - k.mu.x) * k.sc.x + k.be.x, (x.y - k.mu.y) * k.sc.y + k.be.y, (x.z - k.mu.z) * k.sc.z + k.be.z,
                     (x.w - k.mu.w) * k.sc.w + k.be.w);
}

// Y[b, oy, ox, c] (pixel pitch ldy) = relu?(bilinear x`scale` of groupnorm(X))[oy, ox] for oy < Ho, ox < Wo: the crop is the
// output range, the blend is upsample_nhwc_fwd_kernel's.  stats == NULL: no normalisation (the plain upsample + crop).
__global__ __launch_bounds__(256) void gn_apply_up_kernel(const float* __restrict__ X, const float* __restrict__ stats,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* __restrict__ Y, int B, int Hi, int Wi, int C4, int G, int scale,
                                                          int Ho, int Wo, long ldy, int relu) {
  const long n = (long)B * Ho * Wo * C4;
  const long C = (long)C4 * 4;
  const int cpg = stats ? (int)(C / G) : 1;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int cv = (int)(i % C4);
    long t = i / C4;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho);
    const long b = t / Ho;
    GnCoef k;
    k.mu = make_float4(0.f, 0.f, 0.f, 0.f);
    k.sc = make_float4(1.f, 1.f, 1.f, 1.f);
    k.be = k.mu;
    if (stats) {
      const float* st = stats + (b * G + (cv * 4) / cpg) * 2;
      const float m = st[0], is = st[1];
      const float4 g = ld4(gamma + cv * 4);
      k.mu = make_float4(m, m, m, m);
      k.sc = make_float4(is * g.x, is * g.y, is * g.z, is * g.w);
      k.be = ld4(beta + cv * 4);
    }
    const float* p = X + b * Hi * Wi * C + cv * 4;
    float4 y;
    if (scale == 1) {
      y = ld4(p + ((long)oy * Wi + ox) * C);
      if (stats) y = gn_one(y, k);
    } else {
      const Lerp ly = lerp_of(oy, Hi, Hi * scale, 0), lx = lerp_of(ox, Wi, Wi * scale, 0);
      float4 v00 = ld4(p + ((long)ly.i0 * Wi + lx.i0) * C), v01 = ld4(p + ((long)ly.i0 * Wi + lx.i1) * C);
      float4 v10 = ld4(p + ((long)ly.i1 * Wi + lx.i0) * C), v11 = ld4(p + ((long)ly.i1 * Wi + lx.i1) * C);
      if (stats) { v00 = gn_one(v00, k); v01 = gn_one(v01, k); v10 = gn_one(v10, k); v11 = gn_one(v11, k); }
      float4 top, bot;
      top.x = v00.x + lx.w1 * (v01.x - v00.x); bot.x = v10.x + lx.w1 * (v11.x - v10.x); y.x = top.x + ly.w1 * (bot.x - top.x);
      top.y = v00.y + lx.w1 * (v01.y - v00.y); bot.y = v10.y + lx.w1 * (v11.y - v10.y); y.y = top.y + ly.w1 * (bot.y - top.y);
      top.z = v00.z + lx.w1 * (v01.z - v00.z); bot.z = v10.z + lx.w1 * (v11.z - v10.z); y.z = top.z + ly.w1 * (bot.z - top.z);
      top.w = v00.w + lx.w1 * (v01.w - v00.w); bot.w = v10.w + lx.w1 * (v11.w - v10.w); y.w = top.w + ly.w1 * (bot.w - top.w);
    }
    if (relu) { y.x = fmaxf(y.x, 0.f); y.y = fmaxf(y.y, 0.f); y.z = fmaxf(y.z, 0.f); y.w = fmaxf(y.w, 0.f); }
    st4(Y + ((b * Ho + oy) * Wo + ox) * ldy + cv * 4, y);
  }
}

// ---------------------------------------------------------------------------------------------------------- narrow heads
// Y[r][n] = sum_c X[r * ldx + c] w[n][c] + bias[n], N = 1 | 2.  8 lanes per row (C % 32 == 0), butterfly sum (fixed order).
template <int N>
__global__ __launch_bounds__(256) void irn_head_kernel(const float* __restrict__ X, long ldx, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ Y, long M, int C) {
  const int l = threadIdx.x & 7;
  const long Mr = (M + 7) & ~7L;   // (whole 8-lane groups stay together through the shuffles: rows past M compute and drop)
  for (long r = ((long)blockIdx.x * 256 + threadIdx.x) >> 3; r < Mr; r += ((long)gridDim.x * 256) >> 3) {
    float s[N];
#pragma unroll
    for (int n = 0; n < N; ++n) s[n] = 0.f;
    if (r < M)
      for (int c = l * 4; c < C; c += 32) {
        const float4 x = ld4(X + r * ldx + c);
#pragma unroll
        for (int n = 0; n < N; ++n) {
          const float4 ww = ld4(w + n * C + c);
          s[n] += x.x * ww.x + x.y * ww.y + x.z * ww.z + x.w * ww.w;
        }
      }
#pragma unroll
    for (int n = 0; n < N; ++n) {
      s[n] += __shfl_xor(s[n], 1, 8);
      s[n] += __shfl_xor(s[n], 2, 8);
      s[n] += __shfl_xor(s[n], 4, 8);
    }
    if (l == 0 && r < M) {
#pragma unroll
      for (int n = 0; n < N; ++n) Y[r * N + n] = s[n] + (bias ? bias[n] : 0.f);
    }
  }
}

// edge[y][x] = sigmoid(E[0][y][x] / 2 + E[1][y][w-1-x] / 2);  dp[c][y][x] = D[0][y][x][c]
__global__ __launch_bounds__(256) void irn_net_finish_kernel(const float* __restrict__ E, const float* __restrict__ D,
                                                         float* __restrict__ edge, float* __restrict__ dp, int h, int w) {
  const int n = h * w;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int y = i / w, x = i - y * w;
    const float z = E[i] / 2.f + E[n + y * w + (w - 1 - x)] / 2.f;
    edge[i] = 1.0f / (1.0f + expf(-z));
    dp[i] = D[2 * i];
    dp[n + i] = D[2 * i + 1];
  }
}

}  // namespace

extern "C" {

int tris_irn_stem_f32(const unsigned char* img, const float* lut, const float* Wk, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, float* Y, int H, int W, void* stream) {
  if (H < 1 || W < 1) return (int)hipErrorInvalidValue;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(irn_stem_kernel<unsigned char>, dim3(cdiv(Wo, ST), cdiv(Ho, ST), 2), dim3(256), 0, (hipStream_t)stream, img, lut,
                     Wk, mean, invstd, gamma, beta, Y, H, W, Ho, Wo);
  TRIS_LAUNCH_CHECK();
  return 0;
}

int tris_irn_stem_batch_f32(const float* img, const float* Wk, const float* mean, const float* invstd, const float* gamma,
                            const float* beta, float* Y, int B, int H, int W, void* stream) {
  if (B < 1 || B > 65535 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(irn_stem_kernel<float>, dim3(cdiv(Wo, ST), cdiv(Ho, ST), B), dim3(256), 0, (hipStream_t)stream, img,
                     (const float*)nullptr, Wk, mean, invstd, gamma, beta, Y, H, W, Ho, Wo);
  TRIS_LAUNCH_CHECK();
  return 0;
}

int tris_maxpool3s2_f32(const float* X, float* Y, int B, int H, int W, int C, void* stream) {
  if (C % 4 || B < 1 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(maxpool3s2_kernel, dim3(ew_grid((long)B * Ho * Wo * (C / 4))), dim3(256), 0, (hipStream_t)stream, X, Y, B, H,
                     W, Ho, Wo, C / 4);
  TRIS_LAUNCH_CHECK();
  return 0;
}

int tris_subsample2_f32(const float* X, float* Y, int B, int H, int W, int C, void* stream) {
  if (C % 4 || B < 1 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(subsample2_kernel, dim3(ew_grid((long)B * Ho * Wo * (C / 4))), dim3(256), 0, (hipStream_t)stream, X, Y, B, H,
                     W, Ho, Wo, C / 4);
  TRIS_LAUNCH_CHECK();
  return 0;
}

long tris_gn_workspace_bytes(int B, long HW, int G) { return (long)B * gn_blocks(HW) * G * 2 * (long)sizeof(double); }

int tris_gn_stats_f32(const float* X, int B, long HW, int C, int G, float eps, float* stats, double* workspace, void* stream) {
  if (!gn_shape_ok(C, G) || B < 1 || HW < 1) return (int)hipErrorInvalidValue;
  const int nblk = gn_blocks(HW);
  const long rpb = (HW + nblk - 1) / nblk;
  hipLaunchKernelGGL(gn_partial_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, X, HW, C, G, rpb, workspace);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(B * G), dim3(64), 0, (hipStream_t)stream, workspace, nblk, G,
                     (double)HW * (double)(C / G), (double)eps, stats);
  TRIS_LAUNCH_CHECK();
  return 0;
}

int tris_gn_apply_up_f32(const float* X, const float* stats, const float* gamma, const float* beta, float* Y, int B, int Hi, int Wi,
                         int C, int G, int scale, int Ho, int Wo, long ldy, int relu, void* stream) {
  if (C % 4 || ldy % 4 || ldy < C || scale < 1 || B < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || Ho > Hi * scale || Wo > Wi * scale)
    return (int)hipErrorInvalidValue;
  if (stats != nullptr && (!gn_shape_ok(C, G) || gamma == nullptr || beta == nullptr)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(gn_apply_up_kernel, dim3(ew_grid((long)B * Ho * Wo * (C / 4))), dim3(256), 0, (hipStream_t)stream, X, stats,
                     gamma, beta, Y, B, Hi, Wi, C / 4, G, scale, Ho, Wo, ldy, relu);
  TRIS_LAUNCH_CHECK();
  return 0;
}

int tris_irn_head_f32(const float* X, long ldx, const float* w, const float* bias, float* Y, long M, int C, int N, void* stream) {
  if (C % 32 || ldx % 4 || ldx < C || M < 1 || (N != 1 && N != 2)) return (int)hipErrorInvalidValue;
  const int grid = ew_grid(M * 8);
  if (N == 1)
    hipLaunchKernelGGL(irn_head_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, X, ldx, w, bias, Y, M, C);
  else
    hipLaunchKernelGGL(irn_head_kernel<2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, X, ldx, w, bias, Y, M, C);
  TRIS_LAUNCH_CHECK();
  return 0;
}

int tris_irn_net_finish_f32(const float* E, const float* D, float* edge, float* dp, int h, int w, void* stream) {
  if (h < 1 || w < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(irn_net_finish_kernel, dim3(ew_grid((long)h * w)), dim3(256), 0, (hipStream_t)stream, E, D, edge, dp, h, w);
  TRIS_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
