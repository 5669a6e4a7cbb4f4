// Box metrics of one (image, sentence) prediction (validate.py:106-117, 191-208; utils/box_eval_utils.py:10-73): PointM (hitm),
// generate_bbox on the boolean mask cam > 1e-9 restated without cv2 / torchvision, bbox_hit, box_miou, box_acc.
//   proposals  = bounding rectangles of the 8-connected foreground components + of the holes (4-connected background components
//                that do not reach the frame) grown by one pixel, in raster order of each component's first pixel
//   confidence = foreground share of the rectangle, double, from an int32 summed-area table
//   NMS        = torchvision's CPU loop on the (x, y, w, h) rows read as (x1, y1, x2, y2), float32, threshold 0.05
// Both colours are labelled in ONE union-find over nodes 0..H*W: node 0 is the outside of the image, pixel p is node p + 1.  A
// parent is always a smaller node than its child (unionfind.h, shared with insseg.hip), so a root is its component's
// first raster pixel -- the project's tie key -- and every background component that touches the frame has root 0.
#include <limits.h>
#include "common.h"
#include "tris_hip.h"
#include "unionfind.h"

namespace {
struct BoxWs {
  double* conf;                                      // [N] proposal confidence
  int *parent, *minx, *miny, *maxx, *maxy;           // [N] union-find + per-root rectangle slots
  int* sat;                                          // [n] inclusive summed-area table of the mask
  int* tcount;                                       // [nb] roots per 256-node tile
  int *px, *py, *pw, *ph, *pcnt;                     // [N] proposals (x, y, w, h, foreground count)
  float* conf32;                                     // [N]
  int* state;                                        // [N] 0: still to visit, 1: visited or suppressed
  unsigned char* mask;                               // [n]
};
__host__ __device__ inline long align8(long v) { return (v + 7) & ~7L; }
inline long box_ws_layout(long n, BoxWs* w, char* base) {
  long N = n + 1, nb = (N + 255) / 256, o = 0;
  auto take = [&](long bytes) { char* p = base ? base + o : nullptr; o = align8(o + bytes); return p; };
  char* c = take(8 * N);
  char* ints[5];
  for (int i = 0; i < 5; ++i) ints[i] = take(4 * N);
  char* sat = take(4 * n);
  char* tc = take(4 * nb);
  char* pr[5];
  for (int i = 0; i < 5; ++i) pr[i] = take(4 * N);
  char* c32 = take(4 * N);
  char* stt = take(4 * N);
  char* m = take(n);
  if (w) {
    w->conf = (double*)c;
    w->parent = (int*)ints[0]; w->minx = (int*)ints[1]; w->miny = (int*)ints[2]; w->maxx = (int*)ints[3]; w->maxy = (int*)ints[4];
    w->sat = (int*)sat; w->tcount = (int*)tc;
    w->px = (int*)pr[0]; w->py = (int*)pr[1]; w->pw = (int*)pr[2]; w->ph = (int*)pr[3]; w->pcnt = (int*)pr[4];
    w->conf32 = (float*)c32; w->state = (int*)stt; w->mask = (unsigned char*)m;
  }
  return o;
}

// mask = cam > 1e-9; every pixel starts linked to its upper neighbour of the same colour, else to its left one, else to itself;
// a background pixel of the first row / column starts linked to the outside node
__global__ __launch_bounds__(256) void bx_init_kernel(const float* __restrict__ cam, int H, int W, BoxWs w) {
  int n = H * W;
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  int y = p / W, x = p - y * W;
  bool c = cam[p] > 1e-9f;
  w.mask[p] = c ? 1 : 0;
  int node = p + 1, v = node;
  bool up = y > 0 && ((cam[p - W] > 1e-9f) == c), left = x > 0 && ((cam[p - 1] > 1e-9f) == c);
  if (!c && (y == 0 || x == 0)) v = 0;
  else if (up) v = node - W;
  else if (left) v = node - 1;
  w.parent[node] = v;
  w.minx[node] = INT_MAX; w.miny[node] = INT_MAX; w.maxx[node] = -1; w.maxy[node] = -1;
  if (p == 0) { w.parent[0] = 0; w.minx[0] = INT_MAX; w.miny[0] = INT_MAX; w.maxx[0] = -1; w.maxy[0] = -1; }
}
// parent[i] <- the root of i
__global__ __launch_bounds__(256) void bx_compress_kernel(int* parent, int N) {
  int i = blockIdx.x * 256 + threadIdx.x + 1;
  if (i >= N) return;
  int a = uf_load(parent, i);
  if (a == i) return;
  __atomic_store_n(&parent[i], uf_root(parent, a), __ATOMIC_RELAXED);
}
// the adjacencies the initial links do not cover: foreground 8-connected, background 4-connected + the frame
__global__ __launch_bounds__(256) void bx_merge_kernel(int H, int W, BoxWs w) {
  int n = H * W;
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  int y = p / W, x = p - y * W, node = p + 1;
  const unsigned char* m = w.mask;
  unsigned char c = m[p];
  bool U = y > 0 && m[p - W] == c, L = x > 0 && m[p - 1] == c;
  if (c) {
    if (U && L) uf_unite(w.parent, node, node - 1);
    if (!U && y > 0) {   // (with an upper neighbour both diagonals are 4-adjacent to it)
      if (x > 0 && !L && m[p - W - 1]) uf_unite(w.parent, node, node - W - 1);
      if (x < W - 1 && m[p - W + 1]) uf_unite(w.parent, node, node - W + 1);
    }
  } else {
    if (y == 0 || x == 0) return;
    if (U && L) uf_unite(w.parent, node, node - 1);
    if (y == H - 1 || x == W - 1) uf_unite(w.parent, node, 0);
  }
}
// inclusive row sums of the mask: one block per row
__global__ __launch_bounds__(256) void bx_rowscan_kernel(int W, BoxWs w) {
  __shared__ int wsum[4];
  const long base = (long)blockIdx.x * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int x0 = 0; x0 < W; x0 += 256) {
    int x = x0 + threadIdx.x;
    int v = x < W ? w.mask[base + x] : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      int t = __shfl_up(v, o, 64);
      if (lane >= o) v += t;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    int add = carry;
    for (int k = 0; k < wave; ++k) add += wsum[k];
    if (x < W) w.sat[base + x] = v + add;
    carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
}
// column sums of the row sums: one thread per column, eight rows in flight
__global__ __launch_bounds__(256) void bx_colscan_kernel(int H, int W, BoxWs w) {
  int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= W) return;
  int* s = w.sat + x;
  int acc = 0, y = 0;
  for (; y + 8 <= H; y += 8) {
    int v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = s[(long)(y + k) * W];
#pragma unroll
    for (int k = 0; k < 8; ++k) { acc += v[k]; s[(long)(y + k) * W] = acc; }
  }
  for (; y < H; ++y) { acc += s[(long)y * W]; s[(long)y * W] = acc; }
}
__device__ __forceinline__ bool bx_degenerate(const BoxWs& w, int n) {   // all zero / all one: nothing survives the reference's threshold
  int tot = w.sat[n - 1];
  return tot == 0 || tot == n;
}
// rectangles of the roots (only pixels with a differing neighbour on a side can be extreme on that side) + roots per tile
__global__ __launch_bounds__(256) void bx_rect_kernel(int H, int W, BoxWs w) {
  int n = H * W, N = n + 1;
  int i = blockIdx.x * 256 + threadIdx.x;
  bool isroot = false;
  if (i >= 1 && i < N) {
    int p = i - 1, y = p / W, x = p - y * W;
    const unsigned char* m = w.mask;
    unsigned char c = m[p];
    bool bl = x == 0 || m[p - 1] != c, br = x == W - 1 || m[p + 1] != c;
    bool bu = y == 0 || m[p - W] != c, bd = y == H - 1 || m[p + W] != c;
    isroot = uf_load(w.parent, i) == i;
    if (bl || br || bu || bd) {
      int r = uf_root(w.parent, i);
      if (r != 0) {
        if (bl) atomicMin(&w.minx[r], x);
        if (br) atomicMax(&w.maxx[r], x);
        if (bu) atomicMin(&w.miny[r], y);
        if (bd) atomicMax(&w.maxy[r], y);
      }
    }
  }
  if (bx_degenerate(w, n)) isroot = false;
  int cnt = __syncthreads_count(isroot);
  if (threadIdx.x == 0) w.tcount[blockIdx.x] = cnt;
}
__device__ __forceinline__ int bx_sat(const int* sat, int W, int y, int x) { return (y < 0 || x < 0) ? 0 : sat[(long)y * W + x]; }
// roots -> proposals in raster order, with their counts and confidences
__global__ __launch_bounds__(256) void bx_emit_kernel(int H, int W, BoxWs w) {
  __shared__ int red[4], wcnt[4];
  int n = H * W, N = n + 1;
  int part = 0;
  for (int j = threadIdx.x; j < (int)blockIdx.x; j += 256) part += w.tcount[j];
  const int off = block_isum_256(part, red);
  if (w.tcount[blockIdx.x] == 0) return;   // (uniform: also every tile of a degenerate mask)
  int i = blockIdx.x * 256 + threadIdx.x;
  bool isroot = i >= 1 && i < N && uf_load(w.parent, i) == i;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long b = __ballot(isroot);
  if (lane == 0) wcnt[wave] = __popcll(b);
  __syncthreads();
  if (!isroot) return;
  int k = off + __popcll(b & ((1ull << lane) - 1ull));
  for (int q = 0; q < wave; ++q) k += wcnt[q];
  int x = w.minx[i], y = w.miny[i], bw = w.maxx[i] - x + 1, bh = w.maxy[i] - y + 1;
  if (!w.mask[i - 1]) { x -= 1; y -= 1; bw += 2; bh += 2; }   // a hole's border runs on the foreground around it
  int x2 = x + bw - 1, y2 = y + bh - 1;
  int cnt = bx_sat(w.sat, W, y2, x2) - bx_sat(w.sat, W, y - 1, x2) - bx_sat(w.sat, W, y2, x - 1) + bx_sat(w.sat, W, y - 1, x - 1);
  // numpy: uint8 slice .mean() / 255 = float64(255 * cnt) / float64(w * h) / 255
  double conf = __ddiv_rn(__ddiv_rn((double)(255LL * cnt), (double)((long long)bw * bh)), 255.0);
  w.px[k] = x; w.py[k] = y; w.pw[k] = bw; w.ph[k] = bh; w.pcnt[k] = cnt;
  w.conf[k] = conf;
  w.conf32[k] = __double2float_rn(conf);
  w.state[k] = 0;
}
// utils/box_utils.box_iou of one float32 box against the one int64 ground-truth box (promoted to float32)
__device__ float bx_iou_gt(int x1, int y1, int x2, int y2, const int* g) {
  float a1 = __fmul_rn((float)(x2 - x1), (float)(y2 - y1));
  float a2 = (float)((long long)(g[2] - g[0]) * (long long)(g[3] - g[1]));
  float lx = fmaxf((float)x1, (float)g[0]), ly = fmaxf((float)y1, (float)g[1]);
  float rx = fminf((float)x2, (float)g[2]), ry = fminf((float)y2, (float)g[3]);
  float ww = fmaxf(__fsub_rn(rx, lx), 0.f), hh = fmaxf(__fsub_rn(ry, ly), 0.f);
  float inter = __fmul_rn(ww, hh);
  float uni = __fsub_rn(__fadd_rn(a1, a2), inter);
  return __fdiv_rn(inter, uni);
}
// The ordered greedy NMS as "take the best proposal still standing, strike what it overlaps" (= torchvision's loop over the
// sorted list), the kept filter and the per-sentence results.  One workgroup.
__global__ __launch_bounds__(256) void bx_nms_kernel(const unsigned char* __restrict__ target, int H, int W,
                                                     const int* __restrict__ gt, const long* __restrict__ iu, BoxWs w,
                                                     int* __restrict__ record, int* __restrict__ boxes_out) {
  __shared__ int red[4];
  __shared__ double dred[4];
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ int s_cur;
  const int n = H * W, nb = (n + 1 + 255) / 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int part = 0;
  for (int j = threadIdx.x; j < nb; j += 256) part += w.tcount[j];
  const int P = block_isum_256(part, red);
  double dm = 0.0;
  for (int j = threadIdx.x; j < P; j += 256) dm = fmax(dm, w.conf[j]);
  dm = wave_max_f64(dm);
  if (lane == 0) dred[wave] = dm;
  __syncthreads();
  const double cmax = fmax(fmax(dred[0], dred[1]), fmax(dred[2], dred[3]));
  long am = iu[2];
  if (am < 0 || am >= n) am = 0;
  const int my = (int)(am / W), mx = (int)(am - (long)my * W);
  // thread 0's running results
  int nnms = 0, nkept = 0, acc = 0;
  int hx1 = 0, hy1 = 0, hx2 = 1, hy2 = 1;   // the reference's default box
  int cur = -1;
  float cx1 = 0.f, cy1 = 0.f, cx2 = 0.f, cy2 = 0.f, carea = 0.f;
  while (true) {
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int j = threadIdx.x; j < P; j += 256) {
      if (w.state[j]) continue;
      if (j == cur) { w.state[j] = 1; continue; }
      float x1 = (float)w.px[j], y1 = (float)w.py[j], x2 = (float)w.pw[j], y2 = (float)w.ph[j];
      if (cur >= 0) {
        float area = __fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1));
        float iw = fmaxf(0.f, __fsub_rn(fminf(cx2, x2), fmaxf(cx1, x1)));
        float ih = fmaxf(0.f, __fsub_rn(fminf(cy2, y2), fmaxf(cy1, y1)));
        float inter = __fmul_rn(iw, ih);
        float ovr = __fdiv_rn(inter, __fsub_rn(__fadd_rn(carea, area), inter));
        if ((double)ovr > 0.05) { w.state[j] = 1; continue; }
      }
      float v = w.conf32[j];
      if (v > bv) { bv = v; bi = j; }   // (j ascends: the first of equal confidences stays)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      float ov = __shfl_xor(bv, o, 64);
      int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    __syncthreads();   // (s_cur / sv / si of the round before have been read)
    if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int q = 1; q < 4; ++q)
        if (sv[q] > bv || (sv[q] == bv && si[q] < bi)) { bv = sv[q]; bi = si[q]; }
      s_cur = bi;
    }
    __syncthreads();
    cur = s_cur;
    if (cur == INT_MAX) break;
    const int x = w.px[cur], y = w.py[cur], bw = w.pw[cur], bh = w.ph[cur];
    cx1 = (float)x; cy1 = (float)y; cx2 = (float)bw; cy2 = (float)bh;   // the (x, y, w, h) row read as (x1, y1, x2, y2)
    carea = __fmul_rn(__fsub_rn(cx2, cx1), __fsub_rn(cy2, cy1));
    if (threadIdx.x == 0) {
      ++nnms;
      if (w.conf[cur] > 0.5 * cmax) {
        int* row = boxes_out + 5L * nkept;
        row[0] = x; row[1] = y; row[2] = bw; row[3] = bh; row[4] = w.pcnt[cur];
        const int x2 = x + bw, y2 = y + bh;
        if (bx_iou_gt(x, y, x2, y2, gt) > 0.5f) acc = 1;
        if (nkept == 0 || (x <= mx && mx <= x2 && y <= my && my <= y2)) { hx1 = x; hy1 = y; hx2 = x2; hy2 = y2; }
        ++nkept;
      }
    }
  }
  if (threadIdx.x == 0) {
    const float miou = bx_iou_gt(hx1, hy1, hx2, hy2, gt);
    if (nkept == 0 && miou > 0.5f) acc = 1;   // the default list
    record[0] = target[am] != 0 ? 1 : 0;
    record[1] = P; record[2] = nnms; record[3] = nkept;
    record[4] = hx1; record[5] = hy1; record[6] = hx2; record[7] = hy2;
    record[8] = acc;
    record[9] = __float_as_int(miou);
    const long long cb = __double_as_longlong(cmax);
    record[10] = (int)(cb & 0xffffffffLL);
    record[11] = (int)(cb >> 32);
    record[12] = 0; record[13] = 0; record[14] = 0; record[15] = 0;
  }
}
}  // namespace

extern "C" long tris_eval_boxes_workspace_bytes(int H, int W) {
  if (H <= 0 || W <= 0 || (long)H * W > (1L << 24)) return -1;
  return box_ws_layout((long)H * W, nullptr, nullptr);
}

extern "C" int tris_eval_boxes_f32(const float* cam, const unsigned char* target, int H, int W, const int* gt_box, const long* iu,
                                   int* record, int* boxes_out, void* workspace, void* stream) {
  if (H <= 0 || W <= 0 || (long)H * W > (1L << 24)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)workspace & 7) != 0) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int n = H * W, N = n + 1;
  BoxWs w;
  box_ws_layout(n, &w, (char*)workspace);
  const int gp = cdiv(n, 256), gn = cdiv(N, 256);
  hipLaunchKernelGGL(bx_init_kernel, dim3(gp), dim3(256), 0, st, cam, H, W, w);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(bx_rowscan_kernel, dim3(H), dim3(256), 0, st, W, w);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(bx_colscan_kernel, dim3(cdiv(W, 256)), dim3(256), 0, st, H, W, w);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(bx_compress_kernel, dim3(gp), dim3(256), 0, st, w.parent, N);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(bx_merge_kernel, dim3(gp), dim3(256), 0, st, H, W, w);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(bx_rect_kernel, dim3(gn), dim3(256), 0, st, H, W, w);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(bx_emit_kernel, dim3(gn), dim3(256), 0, st, H, W, w);
  TRIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(bx_nms_kernel, dim3(1), dim3(256), 0, st, target, H, W, gt_box, iu, w, record, boxes_out);
  TRIS_LAUNCH_CHECK();
  return 0;
}
