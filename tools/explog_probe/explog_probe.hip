// __expf / __logf of gfx950 on given fp32 arguments, one call per element, for measuring the
// intrinsics' error against fp64 (tools/explog_probe/measure.py; the constants K_EXP / K_LOG of
// tests/test_gpu_swav.py come from it). Reads raw fp32 from IN, writes raw fp32 to OUT.
//
// hipcc --offload-arch=gfx950 -O3 -ffp-contract=fast -Xclang -target-feature -Xclang -packed-fp32-ops \
//       -o explog_probe tools/explog_probe/explog_probe.hip      (the flags of csrc/kernels/swav.hip)
// ./explog_probe exp|log IN OUT
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x)                                                                   \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      std::exit(1);                                                                \
    }                                                                              \
  } while (0)

template <bool LOG>
__global__ __launch_bounds__(256) void probe_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = LOG ? __logf(x[i]) : __expf(x[i]);
}

int main(int argc, char** argv) {
  if (argc != 4 || (std::strcmp(argv[1], "exp") && std::strcmp(argv[1], "log"))) {
    std::fprintf(stderr, "usage: explog_probe exp|log IN OUT\n");
    return 2;
  }
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  const size_t n = (size_t)std::ftell(f) / sizeof(float);
  std::fseek(f, 0, SEEK_SET);
  std::vector<float> h(n);
  if (n == 0 || std::fread(h.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);
  float *dx, *dy;
  CHECK(hipMalloc(&dx, n * sizeof(float)));
  CHECK(hipMalloc(&dy, n * sizeof(float)));
  CHECK(hipMemcpy(dx, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
  const dim3 grid((unsigned)((n + 255) / 256));
  if (!std::strcmp(argv[1], "log"))
    hipLaunchKernelGGL(probe_kernel<true>, grid, dim3(256), 0, 0, dx, dy, n);
  else
    hipLaunchKernelGGL(probe_kernel<false>, grid, dim3(256), 0, 0, dx, dy, n);
  CHECK(hipGetLastError());
  CHECK(hipMemcpy(h.data(), dy, n * sizeof(float), hipMemcpyDeviceToHost));
  CHECK(hipFree(dx));
  CHECK(hipFree(dy));
  f = std::fopen(argv[3], "wb");
  if (!f || std::fwrite(h.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);
  return 0;
}
