// Accuracy of the rsqrtf the row normalisations call (csrc/norm.hip: layernorm_fwd_kernel, instnorm_fwd_kernel), against fp64: the
// constant C_RSQ of tests/oracle_rownorm.py.  The compiler's HIP math header defines rsqrtf as a device-library call whose accuracy
// it does not state.  Sweeps 2^24 arguments, log-uniform over [2^-30, 2^30]; the error is relative, in units of u = 2^-24, and
// holds the rounding of the result to float32 (0.5 u for a correctly rounded function).  For comparison: 1.0f / sqrtf(x) (two
// correctly rounded operations) and sqrtf alone.
//   hipcc -O3 --offload-arch=gfx950 tools/rsqrtf_probe.hip -o rsqrtf_probe && ./rsqrtf_probe
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

__global__ void probe(float* x, float* y, float* z, float* w, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float v = exp2f(-30.0f + 60.0f * ((float)i / (float)(n - 1)));
    x[i] = v;
    y[i] = rsqrtf(v);
    z[i] = 1.0f / sqrtf(v);
    w[i] = sqrtf(v);
  }
}

int main() {
  const int n = 1 << 24;
  float* d[4];
  for (auto& p : d)
    if (hipMalloc(&p, n * sizeof(float)) != hipSuccess) return 1;
  hipLaunchKernelGGL(probe, dim3((n + 255) / 256), dim3(256), 0, 0, d[0], d[1], d[2], d[3], n);
  std::vector<float> h[4];
  for (int k = 0; k < 4; ++k) {
    h[k].resize(n);
    if (hipMemcpy(h[k].data(), d[k], n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  }
  const double u = std::ldexp(1.0, -24);
  double worst[3] = {0, 0, 0}, at[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const double v = (double)h[0][i];
    const double ref[3] = {1.0 / std::sqrt(v), 1.0 / std::sqrt(v), std::sqrt(v)};
    for (int k = 0; k < 3; ++k) {
      const double rel = std::fabs((double)h[k + 1][i] - ref[k]) / ref[k] / u;
      if (rel > worst[k]) { worst[k] = rel; at[k] = v; }
    }
  }
  std::printf("rsqrtf against fp64, %d arguments log-uniform over [2^-30, 2^30], relative error in units of u = 2^-24\n", n);
  std::printf("rsqrtf(x)          largest %.3f u  (x = %.6g)\n", worst[0], at[0]);
  std::printf("1.0f / sqrtf(x)    largest %.3f u  (x = %.6g)\n", worst[1], at[1]);
  std::printf("sqrtf(x)           largest %.3f u  (x = %.6g)\n", worst[2], at[2]);
  for (auto p : d) (void)hipFree(p);
  return 0;
}
