// Split-K reduction of the weight-gradient kernels (igemm_wgrad.hip, wgrad1x1.hip,
// wgrad3x3.hip): dW = Σ_split partial[split] in fp32, deterministic order, one launch per
// tensor or, deferred, one launch for a residual block's tensors.
#include "common.h"
#include "launchers.h"

using namespace sdx;

namespace {

// dW = Σ_split partial[split] (fp32); optional accumulate into dW. A block owns 64 float4
// columns; its 4 thread rows sum interleaved splits with 4 independent accumulators each
// (many loads in flight), then combine through LDS — deterministic order.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int splits, long n4,
                                                            float* __restrict__ out, int accumulate) {
  __shared__ float4 red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long e = (long)blockIdx.x * 64 + tx;
  const float4* P = reinterpret_cast<const float4*>(part);
  float4 a[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) a[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (e < n4) {
    int k = ty;
    for (; k + 12 < splits; k += 16) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint4 u = ld16s<SDX_NT_PART != 0>(P + (size_t)(k + 4 * q) * n4 + e);
        const float4 v = make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
        a[q].x += v.x; a[q].y += v.y; a[q].z += v.z; a[q].w += v.w;
      }
    }
    for (; k < splits; k += 4) {
      const uint4 u = ld16s<SDX_NT_PART != 0>(P + (size_t)k * n4 + e);
      const float4 v = make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
      a[0].x += v.x; a[0].y += v.y; a[0].z += v.z; a[0].w += v.w;
    }
  }
  float4 s = a[0];
#pragma unroll
  for (int q = 1; q < 4; ++q) { s.x += a[q].x; s.y += a[q].y; s.z += a[q].z; s.w += a[q].w; }
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && e < n4) {
    float4 t = accumulate ? reinterpret_cast<const float4*>(out)[e] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < 4; ++q) { t.x += red[q][tx].x; t.y += red[q][tx].y; t.z += red[q][tx].z; t.w += red[q][tx].w; }
    reinterpret_cast<float4*>(out)[e] = t;
  }
}

}  // namespace

// Deferred split-K reductions (SplitkDefer, launchers.h): while a stream is registered, the
// reductions launched on it are queued and later issued as ONE multi-tensor launch
// (splitk_flush), block b of which serves job j = the first with b < tiles_end[j] — a
// residual block's 3-4 weight gradients become one reduction launch instead of 3-4.
namespace {
constexpr int kMaxSplitkJobs = 16;
struct SplitkJobs {
  const float* part[kMaxSplitkJobs];
  float* dw[kMaxSplitkJobs];
  long n4[kMaxSplitkJobs];
  int splits[kMaxSplitkJobs];
  int acc[kMaxSplitkJobs];
  int tiles_end[kMaxSplitkJobs];
  int n;
};
thread_local hipStream_t g_defer_stream = nullptr;
thread_local SplitkJobs g_jobs{};

// The body of splitk_reduce_kernel for job j (plain loads of the partials). A second copy on
// purpose: one shared inline body changes the register allocation of both kernels
// (tools/isa_digest.py), and their code is pinned.
__global__ __launch_bounds__(256) void splitk_reduce_multi_kernel(SplitkJobs jobs) {
  int j = 0;
  while (j + 1 < jobs.n && (int)blockIdx.x >= jobs.tiles_end[j]) ++j;
  const int b = blockIdx.x - (j ? jobs.tiles_end[j - 1] : 0);
  __shared__ float4 red[4][64];
  const float* __restrict__ part = jobs.part[j];
  const long n4 = jobs.n4[j];
  const int splits = jobs.splits[j];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long e = (long)b * 64 + tx;
  const float4* P = reinterpret_cast<const float4*>(part);
  float4 a[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) a[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (e < n4) {
    int k = ty;
    for (; k + 12 < splits; k += 16) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = P[(size_t)(k + 4 * q) * n4 + e];
        a[q].x += v.x; a[q].y += v.y; a[q].z += v.z; a[q].w += v.w;
      }
    }
    for (; k < splits; k += 4) {
      const float4 v = P[(size_t)k * n4 + e];
      a[0].x += v.x; a[0].y += v.y; a[0].z += v.z; a[0].w += v.w;
    }
  }
  float4 sm = a[0];
#pragma unroll
  for (int q = 1; q < 4; ++q) { sm.x += a[q].x; sm.y += a[q].y; sm.z += a[q].z; sm.w += a[q].w; }
  red[ty][tx] = sm;
  __syncthreads();
  if (ty == 0 && e < n4) {
    float4* out = reinterpret_cast<float4*>(jobs.dw[j]);
    float4 t = jobs.acc[j] ? out[e] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < 4; ++q) { t.x += red[q][tx].x; t.y += red[q][tx].y; t.z += red[q][tx].z; t.w += red[q][tx].w; }
    out[e] = t;
  }
}
}  // namespace

void splitk_defer_begin(hipStream_t s) {
  g_defer_stream = s;
  g_jobs.n = 0;
}

bool splitk_deferring(hipStream_t s) { return g_defer_stream != nullptr && s == g_defer_stream; }

void splitk_defer_cancel() {
  g_defer_stream = nullptr;
  g_jobs.n = 0;
}

hipError_t splitk_flush() {
  hipStream_t s = g_defer_stream;
  g_defer_stream = nullptr;
  if (g_jobs.n == 0) return hipSuccess;
  const int grid = g_jobs.tiles_end[g_jobs.n - 1];
  hipLaunchKernelGGL(splitk_reduce_multi_kernel, dim3(grid), dim3(256), 0, s, g_jobs);
  g_jobs.n = 0;
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_splitk_reduce(const float* partial, int splits, long n4, float* dw, int accumulate, hipStream_t s) {
  if (splitk_deferring(s)) {
    // the queued jobs run unordered in one launch: a second job into the same sink would race
    // its read-modify-write with the first (a shared or tied weight) — issue the queue first
    bool dup = false;
    for (int i = 0; i < g_jobs.n; ++i) dup = dup || g_jobs.dw[i] == dw;
    if (g_jobs.n == kMaxSplitkJobs || dup) {
      // queue full: issue what is queued and keep deferring
      hipStream_t keep = g_defer_stream;
      const hipError_t e = splitk_flush();
      if (e != hipSuccess) return e;
      splitk_defer_begin(keep);
    }
    const int i = g_jobs.n++;
    g_jobs.part[i] = partial;
    g_jobs.dw[i] = dw;
    g_jobs.n4[i] = n4;
    g_jobs.splits[i] = splits;
    g_jobs.acc[i] = accumulate;
    g_jobs.tiles_end[i] = (i ? g_jobs.tiles_end[i - 1] : 0) + (int)((n4 + 63) / 64);
    return hipSuccess;
  }
  const long grid = (n4 + 63) / 64;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(grid), dim3(256), 0, s, partial, splits, n4, dw, accumulate);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}
