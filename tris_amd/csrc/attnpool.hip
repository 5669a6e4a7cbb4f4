// CLIP attention pooling for inference (CLIP/clip/model.py:58-104 AttentionPool2d).  Two memory streams:
//   tokens: c4 [B,h,w,C] + positional_embedding [S*S+1,C] -> T [B,hw+1,C] (mean row, pixel rows, resized positional grid) in one launch
//   pool:   the folded single-query attention of the global embedding -- scores of every token against a per-head vector U, softmax,
//           and the probability-weighted sum of the TOKENS (the K and V projections of the hw+1 tokens are never formed).
// 16-byte accesses along C, no atomics, every sum in index order: two launches on equal inputs give equal bytes.
#include "common.h"
#include "tris_hip.h"
#include "bilinear.h"

namespace {

constexpr int TOK_THREADS = 256;
constexpr int POOL_THREADS = 1024;     // 16 waves (one workgroup per CU: its LDS): pass 1 strides the keys by wave, pass 2 splits the heads
constexpr int POOL_WAVES = POOL_THREADS / 64;
constexpr int POOL_CH = 2048;          // channels of the group's U rows held in LDS at a time (8 heads x 2048 x 4 B = 64 KB)
constexpr int POOL_LDS_MAX = 128 * 1024;

// grid (pix_blocks + mean_blocks, B).  The first pix_blocks blocks own one (pixel, float4 of channels) per thread; the rest own one
// float4 of channels of the mean row and walk the hw pixels in order.
__global__ __launch_bounds__(TOK_THREADS) void attnpool_tokens_kernel(const float* __restrict__ x, const float* __restrict__ pos,
                                                                      float* __restrict__ T, int h, int w, int C, int S,
                                                                      int pix_blocks) {
  const int b = blockIdx.y, C4 = C >> 2, hw = h * w;
  const float4* xb = (const float4*)(x + (long)b * hw * C);
  float4* Tb = (float4*)(T + (long)b * (hw + 1) * C);
  const float4* p4 = (const float4*)pos;
  if ((int)blockIdx.x >= pix_blocks) {
    const int c = ((int)blockIdx.x - pix_blocks) * TOK_THREADS + threadIdx.x;
    if (c >= C4) return;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int i = 0; i < hw; ++i) {
      const float4 v = xb[(long)i * C4 + c];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const float n = (float)hw;
    const float4 p = p4[c];
    Tb[c] = make_float4(s.x / n + p.x, s.y / n + p.y, s.z / n + p.z, s.w / n + p.w);
    return;
  }
  const long idx = (long)blockIdx.x * TOK_THREADS + threadIdx.x;
  if (idx >= (long)hw * C4) return;
  const int i = (int)(idx / C4), c = (int)(idx - (long)i * C4);
  const int y = i / w, xx = i - y * w;
  const LerpQ ly = lerp_exact_of(y, S, h), lx = lerp_exact_of(xx, S, w);
  const float4* g = p4 + C4;           // the S x S grid: pos[1:]
  const float4 v00 = g[(long)(ly.i0 * S + lx.i0) * C4 + c], v01 = g[(long)(ly.i0 * S + lx.i1) * C4 + c];
  const float4 v10 = g[(long)(ly.i1 * S + lx.i0) * C4 + c], v11 = g[(long)(ly.i1 * S + lx.i1) * C4 + c];
  const float4 v = xb[idx];
  float4 o;
  // weighted form (not v0 + w (v1 - v0)): every rounding is relative to a w_k |v_k| term; weights 1 and 0 reproduce the value exactly
  o.x = v.x + (ly.w0 * (lx.w0 * v00.x + lx.w1 * v01.x) + ly.w1 * (lx.w0 * v10.x + lx.w1 * v11.x));
  o.y = v.y + (ly.w0 * (lx.w0 * v00.y + lx.w1 * v01.y) + ly.w1 * (lx.w0 * v10.y + lx.w1 * v11.y));
  o.z = v.z + (ly.w0 * (lx.w0 * v00.z + lx.w1 * v01.z) + ly.w1 * (lx.w0 * v10.z + lx.w1 * v11.z));
  o.w = v.w + (ly.w0 * (lx.w0 * v00.w + lx.w1 * v01.w) + ly.w1 * (lx.w0 * v10.w + lx.w1 * v11.w));
  Tb[(long)C4 + idx] = o;
}

// grid (B * heads / G).  LDS: su [G][CH] | ss [G][L] | sred [G], CH = min(C, POOL_CH).
template <int G>
__global__ __launch_bounds__(POOL_THREADS) void attnpool_pool_kernel(const float* __restrict__ T, const float* __restrict__ U,
                                                                      long sB, long sH, float scale, float* __restrict__ P,
                                                                      float* __restrict__ pooled, int L, int C, int heads) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int ngroups = heads / G;
  const int b = (int)blockIdx.x / ngroups, g0 = ((int)blockIdx.x - b * ngroups) * G;
  const int CH = C < POOL_CH ? C : POOL_CH;
  float* su = sm;
  float* ss = sm + G * CH;
  float* sred = ss + G * L;
  const float* Tb = T + (long)b * L * C;
  const float* Ub = U + (long)b * sB + (long)g0 * sH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // pass 1: ss[hd][j] = T[b][j] . U[b][g0 + hd], a chunk of channels at a time; key j belongs to wave j % 16 in every chunk
  for (int c0 = 0; c0 < C; c0 += CH) {
    const int cw4 = ((C - c0) < CH ? (C - c0) : CH) >> 2;
    __syncthreads();                                        // (the readers of the previous chunk are done)
    for (int i = tid; i < G * cw4; i += POOL_THREADS) {
      const int hd = i / cw4, c = i - hd * cw4;
      ((float4*)(su + hd * CH))[c] = *(const float4*)(Ub + (long)hd * sH + c0 + 4 * c);
    }
    __syncthreads();
    for (int j = wave; j < L; j += POOL_WAVES) {
      const float4* t4 = (const float4*)(Tb + (long)j * C + c0);
      float acc[G];
#pragma unroll
      for (int hd = 0; hd < G; ++hd) acc[hd] = 0.f;
#pragma unroll 8
      for (int c = lane; c < cw4; c += 64) {        // (C = 2048: the eight loads of a key are in flight together)
        const float4 t = t4[c];
#pragma unroll
        for (int hd = 0; hd < G; ++hd) {
          const float4 u = ((const float4*)(su + hd * CH))[c];
          acc[hd] = fmaf(t.w, u.w, fmaf(t.z, u.z, fmaf(t.y, u.y, fmaf(t.x, u.x, acc[hd]))));
        }
      }
#pragma unroll
      for (int hd = 0; hd < G; ++hd) acc[hd] = wave_sum(acc[hd]);
      if (lane == 0) {
#pragma unroll
        for (int hd = 0; hd < G; ++hd) ss[hd * L + j] = c0 == 0 ? acc[hd] : ss[hd * L + j] + acc[hd];
      }
    }
  }
  __syncthreads();

  // softmax of each row: wave hd takes the maximum and writes exp(s - m); one thread per row sums in key order
  if (wave < G) {
    float* row = ss + wave * L;
    float m = -INFINITY;
    for (int j = lane; j < L; j += 64) m = fmaxf(m, row[j] * scale);
    m = wave_max(m);
    for (int j = lane; j < L; j += 64) row[j] = expf(row[j] * scale - m);
  }
  __syncthreads();
  if (tid < G) {
    const float* row = ss + tid * L;
    float s = 0.f;
    for (int j = 0; j < L; ++j) s += row[j];
    sred[tid] = s;
  }
  __syncthreads();
  float* Pb = P + ((long)b * heads + g0) * L;               // rows g0 .. g0 + G - 1 of image b are contiguous: [G][L]
  for (int i = tid; i < G * L; i += POOL_THREADS) {
    const float p = ss[i] / sred[i / L];
    ss[i] = p;
    Pb[i] = p;
  }
  __syncthreads();

  // pass 2: pooled[hd][c] = sum_j P[hd][j] T[j][c], keys in order.  The threads split into NS slices of the group's heads (each slice
  // re-reads the token rows, from L1 / L2), a thread owns one float4 of channels and G / NS float4 accumulators.
  constexpr int NS = G >= 2 ? 2 : 1, GS = G / NS, TS = POOL_THREADS / NS;
  const int C4 = C >> 2, h0 = (tid / TS) * GS;
  float* Ob = pooled + (long)b * sB + (long)(g0 + h0) * sH;
  const float* sp = ss + h0 * L;
  for (int c = tid % TS; c < C4; c += TS) {
    const float4* t4 = (const float4*)Tb + c;
    float4 acc[GS];
#pragma unroll
    for (int hd = 0; hd < GS; ++hd) acc[hd] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
    for (int j = 0; j < L; ++j) {
      const float4 t = t4[(long)j * C4];
#pragma unroll
      for (int hd = 0; hd < GS; ++hd) {
        const float p = sp[hd * L + j];
        acc[hd].x = fmaf(p, t.x, acc[hd].x);
        acc[hd].y = fmaf(p, t.y, acc[hd].y);
        acc[hd].z = fmaf(p, t.z, acc[hd].z);
        acc[hd].w = fmaf(p, t.w, acc[hd].w);
      }
    }
#pragma unroll
    for (int hd = 0; hd < GS; ++hd) *(float4*)(Ob + (long)hd * sH + 4 * c) = acc[hd];
  }
}

template <int G>
int pool_launch(const float* T, const float* U, long sB, long sH, float scale, float* P, float* pooled, int B, int L, int C,
                int heads, hipStream_t st) {
  static int state = -1;               // the kernel needs more than the default 64 KB of dynamic LDS at C >= 2048
  if (state < 0)
    state = (int)hipFuncSetAttribute((const void*)attnpool_pool_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, POOL_LDS_MAX);
  if (state) return state;
  const int CH = C < POOL_CH ? C : POOL_CH;
  const size_t lds = ((size_t)G * CH + (size_t)G * L + 8) * sizeof(float);
  if (lds > (size_t)POOL_LDS_MAX) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(attnpool_pool_kernel<G>, dim3((unsigned)((long)B * (heads / G))), dim3(POOL_THREADS), lds, st, T, U, sB, sH,
                     scale, P, pooled, L, C, heads);
  TRIS_LAUNCH_CHECK();
  return 0;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int tris_attnpool_tokens_f32(const float* c4, const float* pos, float* T, int B, int h, int w, int C, int S,
                                        void* stream) {
  if (B < 1 || B > 65535 || h < 1 || w < 1 || S < 1 || S > 1024 || C < 4 || (C & 3) || (long)h * w + 1 > TRIS_ATTNPOOL_LMAX)
    return (int)hipErrorInvalidValue;
  if (!c4 || !pos || !T || !aligned16(c4) || !aligned16(pos) || !aligned16(T)) return (int)hipErrorInvalidValue;
  const int C4 = C >> 2;
  const int pix_blocks = cdiv((long)h * w * C4, TOK_THREADS), mean_blocks = cdiv(C4, TOK_THREADS);
  hipLaunchKernelGGL(attnpool_tokens_kernel, dim3(pix_blocks + mean_blocks, B), dim3(TOK_THREADS), 0, (hipStream_t)stream, c4, pos,
                     T, h, w, C, S, pix_blocks);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_attnpool_pool_f32(const float* T, const float* U, long strideB, long strideH, float scale, float* P,
                                      float* pooled, int B, int L, int C, int heads, void* stream) {
  if (B < 1 || heads < 1 || L < 1 || L > TRIS_ATTNPOOL_LMAX || C < 4 || (C & 3) || strideB < 0 || strideH < 0 || (strideB & 3) ||
      (strideH & 3))
    return (int)hipErrorInvalidValue;
  if (!T || !U || !P || !pooled || !aligned16(T) || !aligned16(U) || !aligned16(pooled)) return (int)hipErrorInvalidValue;
  const int G = heads % 8 == 0 ? 8 : heads % 4 == 0 ? 4 : heads % 2 == 0 ? 2 : 1;
  if ((long)B * (heads / G) > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  switch (G) {
    case 8: return pool_launch<8>(T, U, strideB, strideH, scale, P, pooled, B, L, C, heads, st);
    case 4: return pool_launch<4>(T, U, strideB, strideH, scale, P, pooled, B, L, C, heads, st);
    case 2: return pool_launch<2>(T, U, strideB, strideH, scale, P, pooled, B, L, C, heads, st);
    default: return pool_launch<1>(T, U, strideB, strideH, scale, P, pooled, B, L, C, heads, st);
  }
}
