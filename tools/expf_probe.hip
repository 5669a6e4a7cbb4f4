// Accuracy of the __expf the flash attention kernels call (csrc/attn_mfma.hip, csrc/attn_h2.hip), against fp64: the constant C_EXP of
// tests/oracle_mha.py.  __expf(x) is exp2(fl(log2e_f32 * x)) on the hardware exp2; the product's rounding and the constant's own
// error put 1.22 u |x| (u = 2^-24) on the result, which the oracle charges as 1.25 u |x|; what is left after taking that off is the
// instruction's own error.  Sweeps 2^24 arguments over [-87, 0] (the results stay normal numbers).
//   hipcc -O2 --offload-arch=gfx950 tools/expf_probe.hip -o expf_probe && ./expf_probe
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

__global__ void probe(float* x, float* y, int n, float lo) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float v = lo * ((float)i / (float)(n - 1));
    x[i] = v;
    y[i] = __expf(v);
  }
}

int main() {
  const int n = 1 << 24;
  float *dx, *dy;
  if (hipMalloc(&dx, n * sizeof(float)) != hipSuccess || hipMalloc(&dy, n * sizeof(float)) != hipSuccess) return 1;
  hipLaunchKernelGGL(probe, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, n, -87.0f);
  std::vector<float> x(n), y(n);
  if (hipMemcpy(x.data(), dx, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  if (hipMemcpy(y.data(), dy, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  const double u = std::ldexp(1.0, -24);
  double worst_raw = 0, worst_left = 0, worst_small = 0, at_raw = 0, at_left = 0;
  for (int i = 0; i < n; ++i) {
    const double e = std::exp((double)x[i]);
    const double rel = std::fabs((double)y[i] - e) / e / u;
    const double left = rel - 1.25 * std::fabs((double)x[i]);
    if (rel > worst_raw) { worst_raw = rel; at_raw = x[i]; }
    if (left > worst_left) { worst_left = left; at_left = x[i]; }
    if (x[i] > -1.0f && rel > worst_small) worst_small = rel;
  }
  std::printf("__expf against fp64 over [-87, 0], %d arguments, in units of u = 2^-24\n", n);
  std::printf("largest relative error                         %.3f u  (x = %.4f)\n", worst_raw, at_raw);
  std::printf("largest relative error for x in (-1, 0]        %.3f u\n", worst_small);
  std::printf("largest (relative error - 1.25 u |x|)          %.3f u  (x = %.4f)\n", worst_left, at_left);
  hipFree(dx);
  hipFree(dy);
  return 0;
}
