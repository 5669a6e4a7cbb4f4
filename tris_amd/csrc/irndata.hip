// IRNet's training input pipeline (irn_data.py): one launch turns a batch of decoded uint8 images and labels of different sizes,
// resident in HBM, into what IRNet/voc12/dataloader.py:222-285 ("dataloader.py") delivers per sample --
//   random_scale (IRNet/misc/imutils.py:48-55, "imutils.py"): Pillow BICUBIC for the image, NEAREST for the label
//   TorchvisionNormalize (dataloader.py:67-81) through the host's 3 x 256 table
//   random_lr_flip (imutils.py:57-66), random_crop / top_left_crop with fills 0 / 255 (imutils.py:68-130)
//   pil_rescale(label, 0.25, 0) (dataloader.py:281)
// Bit-exact against Pillow: the horizontal pass first, rounded and clamped to uint8, the vertical pass on that, both with 1 << 21
// rounding, >> 22 and a clamp (resample_pass_kernel of data.hip).  The host builds only the table entries the crop window needs,
// in the window's order (the flip is the order of the column entries); an axis whose size does not change has no table and its
// pass is the identity.
//
// One 256-thread block per 32 x 32 output tile per sample.  The source patch the tile's taps reach is staged in LDS with aligned
// dword loads (the row's byte misalignment is kept in LDS), the horizontal pass goes into a second LDS buffer, the vertical pass
// with the normalisation table writes 16-byte stores.  A tile wholly outside the pasted box only writes the fills.  No atomics and
// a fixed order of every sum: two runs give equal bytes.
#include "common.h"
#include "tris_hip.h"

namespace {

constexpr int TILE = TRIS_IRN_AUG_TILE;    // output tile edge
constexpr int PATCH = TRIS_IRN_AUG_PATCH;  // most source rows / columns a tile's taps may reach (host-checked)
constexpr int KMAX = TRIS_IRN_AUG_KMAX;    // most taps per output (host-checked)
constexpr int ND = TRIS_IRN_AUG_DESC;      // longs per sample descriptor
constexpr int PITCH = PATCH * 3 + 4;       // bytes per staged source row: 3 bytes of misalignment, rounded to a dword (61 dwords)
constexpr int TPITCH = TILE * 3;           // bytes per row of the horizontal pass's output

// descriptor fields (irn_data.py DESC_*)
enum { D_IMG = 0, D_LAB, D_H, D_W, D_HT, D_WT, D_CT, D_CB, D_CL, D_CR, D_IT, D_IB, D_IL, D_IR, D_FLAGS, D_KH, D_KV, D_COLB, D_COLK,
       D_ROWB, D_ROWK, D_XNN, D_YNN };

__device__ __forceinline__ int clamp_u8(int ss) {
  ss >>= 22;
  return ss < 0 ? 0 : (ss > 255 ? 255 : ss);
}

__global__ __launch_bounds__(256) void irn_augment_kernel(const unsigned char* __restrict__ img_arena,
                                                          const unsigned char* __restrict__ lab_arena,
                                                          const long* __restrict__ desc, const int* __restrict__ tables,
                                                          const float* __restrict__ lut, float* __restrict__ img,
                                                          unsigned char* __restrict__ label,
                                                          unsigned char* __restrict__ label_reduced, int crop, int ntx) {
  __shared__ __attribute__((aligned(16))) unsigned char s_patch[PATCH * PITCH];
  __shared__ __attribute__((aligned(16))) unsigned char s_tmp[PATCH * TPITCH];
  __shared__ float s_lut[768];
  __shared__ int s_cb[TILE][2], s_rb[TILE][2];   // {first source index, tap count} per column / row entry of the tile
  __shared__ int s_ck[TILE][KMAX], s_rk[TILE][KMAX];
  __shared__ int s_xnn[TILE], s_ynn[TILE];      // the label's source column / row per entry

  const int t = threadIdx.x;
  const int b = blockIdx.y;
  const int x0 = (blockIdx.x % ntx) * TILE, y0 = (blockIdx.x / ntx) * TILE;
  const int tw = min(TILE, crop - x0), th = min(TILE, crop - y0);
  const long* d = desc + (long)b * ND;
  // the pasted box inside this tile, in output coordinates
  const int bx0 = max(x0, (int)d[D_CL]), bx1 = min(x0 + tw, (int)d[D_CR]);
  const int by0 = max(y0, (int)d[D_CT]), by1 = min(y0 + th, (int)d[D_CB]);
  const bool inside = bx0 < bx1 && by0 < by1;   // block-uniform
  const int ni = bx1 - bx0, nj = by1 - by0;
  const int W = (int)d[D_W];
  const long crop2 = (long)crop * crop;

  if (inside) {
    const int flags = (int)d[D_FLAGS];
    const bool has_h = flags & 1, has_v = flags & 2, flip = flags & 4;
    const int i0 = bx0 - (int)d[D_CL], j0 = by0 - (int)d[D_CT];   // first column / row entry of the tile
    const int kh = (int)d[D_KH], kv = (int)d[D_KV];
    const int Wt = (int)d[D_WT];
    for (int q = t; q < 768; q += 256) s_lut[q] = lut[q];
    if (t < TILE) {
      const int e = t;
      if (e < ni) {
        if (has_h) {
          const int* p = tables + d[D_COLB] + 2 * (i0 + e);
          s_cb[e][0] = p[0];
          s_cb[e][1] = p[1];
        } else {   // the resized column is the source column
          const int xr = (int)d[D_IL] + i0 + e;
          s_cb[e][0] = flip ? Wt - 1 - xr : xr;
          s_cb[e][1] = 1;
        }
        s_xnn[e] = tables[d[D_XNN] + i0 + e];
      }
    } else if (t < 2 * TILE) {
      const int e = t - TILE;
      if (e < nj) {
        if (has_v) {
          const int* p = tables + d[D_ROWB] + 2 * (j0 + e);
          s_rb[e][0] = p[0];
          s_rb[e][1] = p[1];
        } else {
          s_rb[e][0] = (int)d[D_IT] + j0 + e;
          s_rb[e][1] = 1;
        }
        s_ynn[e] = tables[d[D_YNN] + j0 + e];
      }
    }
    for (int q = t; q < TILE * KMAX; q += 256) {
      const int e = q / KMAX, k = q - e * KMAX;
      int v = k == 0 ? (1 << 22) : 0;   // no table: one tap of 1.0, and (p << 22 + (1 << 21)) >> 22 == p
      if (has_h) v = (e < ni && k < kh) ? tables[d[D_COLK] + (long)(i0 + e) * kh + k] : 0;
      s_ck[e][k] = v;
      v = k == 0 ? (1 << 22) : 0;
      if (has_v) v = (e < nj && k < kv) ? tables[d[D_ROWK] + (long)(j0 + e) * kv + k] : 0;
      s_rk[e][k] = v;
    }
    __syncthreads();
    // source patch: the entries are monotone in the resized index (descending under a flip), so the ends give the extent
    const int x_lo = min(s_cb[0][0], s_cb[ni - 1][0]);
    const int x_hi = max(s_cb[0][0] + s_cb[0][1], s_cb[ni - 1][0] + s_cb[ni - 1][1]);
    const int y_lo = s_rb[0][0];
    const int y_hi = s_rb[nj - 1][0] + s_rb[nj - 1][1];
    const int pw = min(x_hi - x_lo, PATCH), ph = min(y_hi - y_lo, PATCH);   // (the host refuses what exceeds PATCH)
    const unsigned char* src = img_arena + d[D_IMG];
    {
      const int ndw_max = (pw * 3 + 6) >> 2;
      for (int q = t; q < ph * ndw_max; q += 256) {
        const int r = q / ndw_max, w = q - r * ndw_max;
        const long g = ((long)(y_lo + r) * W + x_lo) * 3;   // the image's offset in the arena is a multiple of 16
        const int sh = (int)(g & 3);
        if (w * 4 < sh + pw * 3)   // (the arena ends in 16 spare bytes: the last dword of the last row may reach past the image)
          *reinterpret_cast<unsigned*>(s_patch + r * PITCH + w * 4) = *reinterpret_cast<const unsigned*>(src + (g - sh) + w * 4);
      }
    }
    __syncthreads();
    // horizontal pass -> s_tmp [ph][ni][3]
    for (int q = t; q < ph * ni * 3; q += 256) {
      const int r = q / (ni * 3), ec = q - r * (ni * 3);
      const int e = ec / 3, c = ec - e * 3;
      const int sh = (int)((((long)(y_lo + r) * W + x_lo) * 3) & 3);
      const unsigned char* p = s_patch + r * PITCH + sh + (s_cb[e][0] - x_lo) * 3 + c;
      const int cnt = min(s_cb[e][1], KMAX);
      int ss = 1 << 21;
      for (int k = 0; k < cnt; ++k) ss += (int)p[k * 3] * s_ck[e][k];
      s_tmp[r * TPITCH + ec] = (unsigned char)clamp_u8(ss);
    }
    __syncthreads();
  }

  // vertical pass + normalisation, four floats per thread: a tile row is tw * 3 floats, a multiple of 4 (crop % 4 == 0)
  {
    const int nq = tw * 3 / 4;
    for (int q = t; q < th * nq; q += 256) {
      const int y = q / nq, f4 = q - y * nq;
      float r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int f = f4 * 4 + u;
        const int px = f / 3, c = f - px * 3;
        const int col = x0 + px, row = y0 + y;
        float v = 0.0f;
        if (inside && col >= bx0 && col < bx1 && row >= by0 && row < by1) {
          const int e = col - bx0, j = row - by0;
          const unsigned char* p = s_tmp + (s_rb[j][0] - s_rb[0][0]) * TPITCH + e * 3 + c;
          const int cnt = min(s_rb[j][1], KMAX);
          int ss = 1 << 21;
          for (int k = 0; k < cnt; ++k) ss += (int)p[k * TPITCH] * s_rk[j][k];
          v = s_lut[c * 256 + clamp_u8(ss)];
        }
        r[u] = v;
      }
      float* dst = img + ((long)b * crop2 + (long)(y0 + y) * crop + x0) * 3 + f4 * 4;
      *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
    }
  }
  // label: four bytes per thread
  const unsigned char* lab = lab_arena + d[D_LAB];
  {
    const int y = t >> 3, xq = (t & 7) * 4;
    if (y < th && xq < tw) {
      unsigned pack = 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int col = x0 + xq + u, row = y0 + y;
        unsigned v = 255;
        if (inside && col >= bx0 && col < bx1 && row >= by0 && row < by1) {
          const int xs = s_xnn[col - bx0], ys = s_ynn[row - by0];
          v = (xs < 0 || ys < 0) ? 0u : (unsigned)lab[(long)ys * W + xs];   // (Pillow leaves a pixel it cannot source at 0)
        }
        pack |= v << (8 * u);
      }
      *reinterpret_cast<unsigned*>(label + (long)b * crop2 + (long)(y0 + y) * crop + x0 + xq) = pack;
    }
  }
  // the reduced label: Pillow's NEAREST to a quarter of a size divisible by 4 picks index 4 x + 2
  if (t < 64) {
    const int ry = t >> 3, rx = t & 7;
    const int y = 4 * ry + 2, x = 4 * rx + 2;
    if (y < th && x < tw) {
      const int col = x0 + x, row = y0 + y;
      unsigned v = 255;
      if (inside && col >= bx0 && col < bx1 && row >= by0 && row < by1) {
        const int xs = s_xnn[col - bx0], ys = s_ynn[row - by0];
        v = (xs < 0 || ys < 0) ? 0u : (unsigned)lab[(long)ys * W + xs];
      }
      const int cr = crop / 4;
      label_reduced[(long)b * cr * cr + (long)(y0 / 4 + ry) * cr + (x0 / 4 + rx)] = (unsigned char)v;
    }
  }
}

}  // namespace

extern "C" int tris_irn_augment_batch_u8(const unsigned char* img_arena, const unsigned char* lab_arena, const long* desc,
                                         const int* tables, const float* lut, float* img, unsigned char* label,
                                         unsigned char* label_reduced, int B, int crop, void* stream) {
  if (B <= 0 || B > 65535 || crop <= 0 || crop % 4 || !img_arena || !lab_arena || !desc || !tables || !lut || !img || !label ||
      !label_reduced || (((uintptr_t)img_arena) & 15) || (((uintptr_t)img) & 15) || (((uintptr_t)label) & 3))
    return (int)hipErrorInvalidValue;
  const int nt = cdiv(crop, TILE);
  hipLaunchKernelGGL(irn_augment_kernel, dim3(nt * nt, B), dim3(256), 0, (hipStream_t)stream, img_arena, lab_arena, desc, tables,
                     lut, img, label, label_reduced, crop, nt);
  TRIS_LAUNCH_CHECK();
  return 0;
}
