// Accuracy of the logf and log1pf the loss kernels call, against fp64: the constants C_LOGF and C_LOG1PF of tests/oracle_update.py.
// logf: csrc/heads.hip clip_loss_fwd_kernel takes -logf(clamp(cos, 1e-4, 0.9999)) and -logf(1 - cos), arguments in (1e-4, 2).
// log1pf: csrc/heads.hip log_sigmoid and csrc/seg.hip bce4_fwd_kernel take log1pf(expf(-|x|)), arguments in (0, 1].
// The compiler's HIP math header makes both device-library calls whose accuracy it does not state.  Each sweep is 2^24 arguments,
// log-uniform over its range; the error is relative to the fp64 value, in units of u = 2^-24, and holds the rounding of the
// result to float32 (0.5 u for a correctly rounded function).  logf has two sweeps: (1e-4, 1], the range of the two clamped
// cosines, and (1, 2], where 1 - cos of a negative cosine lands.  log1pf's range starts at 2^-126: below it the argument, an
// expf, is subnormal or zero.
//   hipcc -O3 --offload-arch=gfx950 tools/logf_probe.hip -o logf_probe && ./logf_probe
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

// x = lo * (hi / lo)^(i / (n - 1)), formed in double and rounded once
__global__ void probe(float* x, float* y, double lo, double hi, int which, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float v = (float)(lo * exp(log(hi / lo) * ((double)i / (double)(n - 1))));
    x[i] = v;
    y[i] = which == 0 ? logf(v) : log1pf(v);
  }
}

int main() {
  const int n = 1 << 24;
  float *dx, *dy;
  if (hipMalloc(&dx, n * sizeof(float)) != hipSuccess || hipMalloc(&dy, n * sizeof(float)) != hipSuccess) return 1;
  std::vector<float> hx(n), hy(n);
  const double u = std::ldexp(1.0, -24);
  struct Sweep { const char* name; int which; double lo, hi; };
  const Sweep sweeps[3] = {{"logf(x)   x in (1e-4, 1]    ", 0, 1e-4, 1.0},
                           {"logf(x)   x in (1, 2]       ", 0, 1.0, 2.0},
                           {"log1pf(x) x in [2^-126, 1]  ", 1, std::ldexp(1.0, -126), 1.0}};
  std::printf("logf and log1pf against fp64, %d arguments log-uniform over each range, relative error in units of u = 2^-24\n", n);
  for (const Sweep& s : sweeps) {
    hipLaunchKernelGGL(probe, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, s.lo, s.hi, s.which, n);
    if (hipMemcpy(hx.data(), dx, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    if (hipMemcpy(hy.data(), dy, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    double worst = 0, at = 0;
    long counted = 0;
    for (int i = 0; i < n; ++i) {
      const double v = (double)hx[i];
      const double ref = s.which == 0 ? std::log(v) : std::log1p(v);
      if (ref == 0.0) continue;  // logf(1) = 0: exact or not, checked below
      const double rel = std::fabs((double)hy[i] - ref) / std::fabs(ref) / u;
      ++counted;
      if (rel > worst) { worst = rel; at = v; }
    }
    std::printf("%s largest %.3f u  (x = %.9g, %ld arguments)\n", s.name, worst, at, counted);
  }
  // the end points the kernels can reach exactly
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dx, dy, 1.0, 1.0, 0, 2);
  if (hipMemcpy(hy.data(), dy, 2 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  std::printf("logf(1) = %g\n", (double)hy[0]);
  (void)hipFree(dx);
  (void)hipFree(dy);
  return 0;
}
