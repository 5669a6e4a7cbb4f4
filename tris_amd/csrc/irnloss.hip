// IRNet's affinity / displacement training losses (IRNet/net/resnet50_irn.py:168-222 AffinityDisplacementLoss, the loss lines of
// IRNet/step_refer/train_irn.py:57-68, the pair labels of IRNet/voc12/dataloader.py:83-109), forward and backward, with nothing
// per pair in memory.
//   forward : one block = a 16 x 16 tile of SOURCE pixels of one image; sigmoid(edge), dp and the labels of the tile and its halo
//             (r columns on either side, r rows below) are staged in LDS; every thread walks the search directions and their path
//             cells (the host tables of irn.search_paths), keeps five fp64 sums and three counts in registers; one fixed-order
//             block reduction into a partials buffer; a one-block finish sums the partials in a fixed order.
//   backward: the gradient of a pair's path maximum goes to ONE cell, and at that cell aff = 1 - sigmoid(edge[cell]) whatever the
//             pair.  So d edge_out[q] needs only HOW MANY pairs of each class have their maximum at q: the forward counts them
//             (integer adds in LDS, flushed with integer adds to arg_count [B,3,h,w]; integer sums do not depend on arrival
//             order, so the result is bitwise repeatable) and the backward is elementwise in q.  d dp_out is sign(.) summed over
//             the pairs a pixel is the source or the destination of: an integer gather per pixel, times two fp64 scales.
// The arithmetic is fp64 on fp32 inputs (a pair costs one log; the op is far from any throughput limit): outputs are
// the correctly rounded fp64 results up to the order of the fp64 sums.
#include "common.h"
#include "tris_hip.h"

namespace {

constexpr int TS = 16;        // tile side: 16 x 16 = the 256 threads of a block
constexpr int R_MAX = 15;     // radius_floor the LDS layout is sized for (46 x 31 staged cells, 41 KB, at 15)
constexpr double AFF_EPS = 1e-5;

__device__ __forceinline__ double sigmoid_f64(float x) { return 1.0 / (1.0 + exp(-(double)x)); }
// dataloader.py:97-106: -1 invalid, 0 bg_pos, 1 fg_pos, 2 neg
__device__ __forceinline__ int pair_class(int a, int b) {
  if (a >= 21 || b >= 21) return -1;
  if (a != b) return 2;
  return a > 0 ? 1 : 0;
}
__device__ __forceinline__ int sgn(double t) { return (t > 0.0) - (t < 0.0); }   // torch's sign: sign(0) = 0

inline size_t fwd_lds_bytes(int r) {
  const size_t tn = (size_t)(TS + r) * (TS + 2 * r);
  return tn * (sizeof(double) + 2 * sizeof(float) + 3 * sizeof(int) + 1);
}
inline size_t bwd_lds_bytes(int r) {
  const size_t tn = (size_t)(TS + 2 * r) * (TS + 2 * r);
  return tn * (2 * sizeof(float) + 1);
}

// part_sum[blk][5] = sums over the block's pairs of {pos | bg, pos | fg, neg | neg, fg_0 + fg_1 | fg, bg_0 + bg_1 | bg};
// part_cnt[blk][3] = {N_bg, N_fg, N_neg}.  arg_cnt (may be NULL: no backward wanted) [B][3][h][w] += the pairs whose path
// maximum is at the cell, per class.
__global__ __launch_bounds__(256) void irn_loss_fwd_kernel(const float* __restrict__ edge, const float* __restrict__ dp,
                                                           const unsigned char* __restrict__ label, int h, int w, int r,
                                                           const int* __restrict__ dirs, const int* __restrict__ path_off,
                                                           const int* __restrict__ cells, int nd, int n_cells,
                                                           int* __restrict__ arg_cnt, double* __restrict__ part_sum,
                                                           long long* __restrict__ part_cnt) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ double red_s[4][5];
  __shared__ int red_n[4][3];
  const int TH = TS + r, TW = TS + 2 * r, TN = TH * TW;
  double* sig = reinterpret_cast<double*>(smem);
  float* d0 = reinterpret_cast<float*>(sig + TN);
  float* d1 = d0 + TN;
  int* cnt = reinterpret_cast<int*>(d1 + TN);                     // [3][TN]
  unsigned char* lab = reinterpret_cast<unsigned char*>(cnt + 3 * TN);
  const int tid = threadIdx.x, b = blockIdx.z;
  const long n = (long)h * w;
  const int y0 = blockIdx.y * TS, x0 = blockIdx.x * TS;          // map position of the staged region's corner
  for (int i = tid; i < TN; i += 256) {
    const int gy = y0 + i / TW, gx = x0 + i % TW;
    const bool in = gy < h && gx < w;
    const long q = (long)gy * w + gx;
    sig[i] = in ? sigmoid_f64(edge[b * n + q]) : 0.0;
    d0[i] = in ? dp[(2L * b) * n + q] : 0.f;
    d1[i] = in ? dp[(2L * b + 1) * n + q] : 0.f;
    lab[i] = in ? label[b * n + q] : (unsigned char)255;
    cnt[i] = 0;
    cnt[TN + i] = 0;
    cnt[2 * TN + i] = 0;
  }
  __syncthreads();
  const int ly = tid / TS, lx = tid % TS;
  const int s = ly * TW + lx + r;                                  // the source pixel (y0 + ly, x0 + r + lx) in the staged region
  const bool active = y0 + ly < h - r && x0 + r + lx < w - r;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  int num[3] = {0, 0, 0};
  if (active) {
    const int a = lab[s];
    const double s0 = (double)d0[s], s1 = (double)d1[s];
    for (int d = 0; d < nd; ++d) {
      const int dy = dirs[2 * d], dx = dirs[2 * d + 1];
      if (dy < 0 || dy > r || dx < -r || dx > r) continue;         // (a table of another radius: never leave the staged region)
      const int t = s + dy * TW + dx;
      const int cls = pair_class(a, lab[t]);
      if (cls < 0) continue;
      // the path maximum; among equal maxima the first in the reference's path order (indexing.py:48: larger |cy| + |cx| first,
      // then, the sort being stable, the scan order of the table)
      double best = -1.0;
      int best_l1 = -1, best_i = s;
      const int c0 = max(path_off[d], 0), c1 = min(path_off[d + 1], n_cells);
      for (int c = c0; c < c1; ++c) {
        const int cy = cells[2 * c], cx = cells[2 * c + 1];
        if (cy < 0 || cy > dy || cx < min(dx, 0) || cx > max(dx, 0)) continue;
        const int i = s + cy * TW + cx;
        const double v = sig[i];
        const int l1 = cy + abs(cx);
        if (v > best || (v == best && l1 > best_l1)) {
          best = v;
          best_l1 = l1;
          best_i = i;
        }
      }
      const double aff = 1.0 - best;
      if (cls == 2) {
        acc[2] += -log(1.0 + AFF_EPS - aff);
      } else {
        acc[cls] += -log(aff + AFF_EPS);
        const double p0 = s0 - (double)d0[t], p1 = s1 - (double)d1[t];
        if (cls == 1)
          acc[3] += fabs(p0 - (double)dy) + fabs(p1 - (double)dx);
        else
          acc[4] += fabs(p0) + fabs(p1);
      }
      ++num[cls];
      if (arg_cnt != nullptr) atomicAdd(&cnt[cls * TN + best_i], 1);
    }
  }
  // fixed-order block reduction: lanes by shuffle, the four waves in order
#pragma unroll
  for (int k = 0; k < 5; ++k) acc[k] = wave_sum_f64(acc[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) num[k] = wave_sum_i32(num[k]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) red_s[tid >> 6][k] = acc[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) red_n[tid >> 6][k] = num[k];
  }
  __syncthreads();
  const long blk = ((long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  if (tid < 5) part_sum[blk * 5 + tid] = ((red_s[0][tid] + red_s[1][tid]) + red_s[2][tid]) + red_s[3][tid];
  if (tid >= 64 && tid < 67) {
    const int k = tid - 64;
    part_cnt[blk * 3 + k] = (long long)red_n[0][k] + red_n[1][k] + red_n[2][k] + red_n[3][k];
  }
  if (arg_cnt != nullptr) {
    for (int i = tid; i < TN; i += 256) {
      const int gy = y0 + i / TW, gx = x0 + i % TW;
      if (gy >= h || gx >= w) continue;
      const long q = (long)gy * w + gx;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int v = cnt[k * TN + i];
        if (v != 0) atomicAdd(&arg_cnt[(3L * b + k) * n + q], v);   // integer: the sum does not depend on the order
      }
    }
  }
}

// train_irn.py:57-63.  norm[5] = {1/2 / (N_bg + eps), 1/2 / (N_fg + eps), 1 / (N_neg + eps), 1 / (2 N_fg + eps), 1 / (2 N_bg + eps)}:
// what the backward scales by, left on the device.
__global__ __launch_bounds__(256) void irn_loss_finish_kernel(const double* __restrict__ part_sum,
                                                              const long long* __restrict__ part_cnt, long nb,
                                                              float* __restrict__ losses, long* __restrict__ counts,
                                                              double* __restrict__ norm) {
  __shared__ double ss[5][256];
  __shared__ long long sc[3][256];
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double t = 0.0;
    for (long i = tid; i < nb; i += 256) t += part_sum[i * 5 + k];
    ss[k][tid] = t;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    long long t = 0;
    for (long i = tid; i < nb; i += 256) t += part_cnt[i * 3 + k];
    sc[k][tid] = t;
  }
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int k = 0; k < 5; ++k) ss[k][tid] += ss[k][tid + o];
#pragma unroll
      for (int k = 0; k < 3; ++k) sc[k][tid] += sc[k][tid + o];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const double n_bg = (double)sc[0][0], n_fg = (double)sc[1][0], n_neg = (double)sc[2][0];
  const double c[5] = {0.5 / (n_bg + AFF_EPS), 0.5 / (n_fg + AFF_EPS), 1.0 / (n_neg + AFF_EPS), 1.0 / (2.0 * n_fg + AFF_EPS),
                       1.0 / (2.0 * n_bg + AFF_EPS)};
  losses[0] = (float)(ss[0][0] * c[0] + ss[1][0] * c[1]);
  losses[1] = (float)(ss[2][0] * c[2]);
  losses[2] = (float)(ss[3][0] * c[3]);
  losses[3] = (float)(ss[4][0] * c[4]);
  for (int k = 0; k < 3; ++k) counts[k] = (long)sc[k][0];
  for (int k = 0; k < 5; ++k) norm[k] = c[k];
}

// One block = a 16 x 16 tile of MAP pixels of one image; dp and the labels of the tile and r cells around it in LDS.
__global__ __launch_bounds__(256) void irn_loss_bwd_kernel(const float* __restrict__ edge, const float* __restrict__ dp,
                                                           const unsigned char* __restrict__ label, int h, int w, int r,
                                                           const int* __restrict__ dirs, int nd, const int* __restrict__ arg_cnt,
                                                           const double* __restrict__ norm, const float* __restrict__ g,
                                                           float* __restrict__ d_edge, float* __restrict__ d_dp) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int TW = TS + 2 * r, TN = TW * TW;
  float* d0 = reinterpret_cast<float*>(smem);
  float* d1 = d0 + TN;
  unsigned char* lab = reinterpret_cast<unsigned char*>(d1 + TN);
  const int tid = threadIdx.x, b = blockIdx.z;
  const long n = (long)h * w;
  const int y0 = blockIdx.y * TS, x0 = blockIdx.x * TS;
  if (d_dp != nullptr) {
    for (int i = tid; i < TN; i += 256) {
      const int gy = y0 - r + i / TW, gx = x0 - r + i % TW;
      const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
      const long q = (long)gy * w + gx;
      d0[i] = in ? dp[(2L * b) * n + q] : 0.f;
      d1[i] = in ? dp[(2L * b + 1) * n + q] : 0.f;
      lab[i] = in ? label[b * n + q] : (unsigned char)255;
    }
  }
  __syncthreads();
  const int ly = tid / TS, lx = tid % TS;
  const int y = y0 + ly, x = x0 + lx;
  if (y >= h || x >= w) return;
  const long q = (long)y * w + x;
  if (d_dp != nullptr) {
    const int c = (ly + r) * TW + lx + r;
    const int a = lab[c];
    const double m0 = (double)d0[c], m1 = (double)d1[c];
    const int hs = h - r, xlo = r, xhi = w - r;                    // the source region: rows [0, hs), columns [xlo, xhi)
    const bool is_src = y < hs && x >= xlo && x < xhi;
    int fg0 = 0, fg1 = 0, bg0 = 0, bg1 = 0;
    for (int d = 0; d < nd; ++d) {
      const int dy = dirs[2 * d], dx = dirs[2 * d + 1];
      if (dy < 0 || dy > r || dx < -r || dx > r) continue;
      const int o = dy * TW + dx;
      if (is_src) {                                                // this pixel is the pair's source: + sign
        const int cls = pair_class(a, lab[c + o]);
        const double p0 = m0 - (double)d0[c + o], p1 = m1 - (double)d1[c + o];
        if (cls == 1) {
          fg0 += sgn(p0 - (double)dy);
          fg1 += sgn(p1 - (double)dx);
        } else if (cls == 0) {
          bg0 += sgn(p0);
          bg1 += sgn(p1);
        }
      }
      const int py = y - dy, px = x - dx;
      if (py >= 0 && py < hs && px >= xlo && px < xhi) {           // ... its destination: - sign
        const int cls = pair_class(lab[c - o], a);
        const double p0 = (double)d0[c - o] - m0, p1 = (double)d1[c - o] - m1;
        if (cls == 1) {
          fg0 -= sgn(p0 - (double)dy);
          fg1 -= sgn(p1 - (double)dx);
        } else if (cls == 0) {
          bg0 -= sgn(p0);
          bg1 -= sgn(p1);
        }
      }
    }
    const double c_fg = (double)g[2] * norm[3], c_bg = (double)g[3] * norm[4];
    d_dp[(2L * b) * n + q] = (float)(c_fg * (double)fg0 + c_bg * (double)bg0);
    d_dp[(2L * b + 1) * n + q] = (float)(c_fg * (double)fg1 + c_bg * (double)bg1);
  }
  if (d_edge != nullptr) {
    const int n_bg = arg_cnt[(3L * b) * n + q], n_fg = arg_cnt[(3L * b + 1) * n + q], n_neg = arg_cnt[(3L * b + 2) * n + q];
    float out = 0.f;
    if ((n_bg | n_fg | n_neg) != 0) {
      // every pair with its maximum here has aff = 1 - s: d pos / d s = 1 / (aff + eps), d neg / d s = -1 / (1 + eps - aff)
      const double s = sigmoid_f64(edge[b * n + q]);
      const double aff = 1.0 - s;
      const double pos = (double)g[0] * (norm[0] * (double)n_bg + norm[1] * (double)n_fg) / (aff + AFF_EPS);
      const double neg = (double)g[1] * norm[2] * (double)n_neg / (1.0 + AFF_EPS - aff);
      out = (float)(s * aff * (pos - neg));
    }
    d_edge[b * n + q] = out;
  }
}

inline bool shape_ok(int B, int h, int w, int radius) {
  const int r = radius - 1;
  return B >= 1 && B <= 65535 && r >= 1 && r <= R_MAX && h >= r + 1 && w >= 2 * r + 1;
}
inline long fwd_blocks(int B, int h, int w, int r) { return (long)B * cdiv(h - r, TS) * cdiv(w - 2 * r, TS); }

}  // namespace

extern "C" long tris_irn_loss_workspace_bytes(int B, int h, int w, int radius) {
  if (!shape_ok(B, h, w, radius)) return 0;
  return fwd_blocks(B, h, w, radius - 1) * (long)(5 * sizeof(double) + 3 * sizeof(long long));
}

extern "C" int tris_irn_loss_fwd_f32(const float* edge_out, const float* dp_out, const unsigned char* label, int B, int h, int w,
                                     int radius, const int* dirs, const int* path_off, const int* path_cells, int n_dirs, int n_cells,
                                     float* losses, long* counts, double* norm, int* arg_count, void* workspace, void* stream) {
  if (!shape_ok(B, h, w, radius) || n_dirs < 0 || n_cells < 0) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int r = radius - 1;
  const long nb = fwd_blocks(B, h, w, r);
  double* part_sum = reinterpret_cast<double*>(workspace);
  long long* part_cnt = reinterpret_cast<long long*>(part_sum + nb * 5);
  if (arg_count != nullptr) {
    hipError_t e = hipMemsetAsync(arg_count, 0, (size_t)B * 3 * h * w * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(irn_loss_fwd_kernel, dim3(cdiv(w - 2 * r, TS), cdiv(h - r, TS), B), dim3(256), fwd_lds_bytes(r), st, edge_out,
                     dp_out, label, h, w, r, dirs, path_off, path_cells, n_dirs, n_cells, arg_count, part_sum, part_cnt);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(irn_loss_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)part_sum, (const long long*)part_cnt, nb, losses,
                     counts, norm);
  TRIS_LAUNCH_CHECK();
  return 0;
}

extern "C" int tris_irn_loss_bwd_f32(const float* edge_out, const float* dp_out, const unsigned char* label, int B, int h, int w,
                                     int radius, const int* dirs, int n_dirs, const int* arg_count, const double* norm, const float* g,
                                     float* d_edge, float* d_dp, void* stream) {
  if (!shape_ok(B, h, w, radius) || n_dirs < 0 || (d_edge != nullptr && arg_count == nullptr)) return (int)hipErrorInvalidValue;
  if (d_edge == nullptr && d_dp == nullptr) return 0;
  const int r = radius - 1;
  hipLaunchKernelGGL(irn_loss_bwd_kernel, dim3(cdiv(w, TS), cdiv(h, TS), B), dim3(256), bwd_lds_bytes(r), (hipStream_t)stream,
                     edge_out, dp_out, label, h, w, r, dirs, n_dirs, arg_count, norm, g, d_edge, d_dp);
  TRIS_LAUNCH_CHECK();
  return 0;
}
