// Fused optimizer kernels over the flat fp32 parameter / gradient / momentum buffers.
//
// The reference steps torch.optim.SGD over 163 separate tensors (util.py:79-84,
// main_supcon.py:323-325). Here all parameters live in ONE flat buffer (views handed to
// the modules), so an SGD step is a single streaming kernel (16-B accesses) that also
// folds in the data-parallel gradient averaging (grad_scale = 1/W) and reads the
// learning rate from device memory (no host sync, graph-replayable when the lr
// changes). LARS (config 5) adds one segmented-norm pass per step.
#include "common.h"
#include "launchers.h"

using namespace sdx;

namespace {

// torch SGD semantics (dampening 0): d = s·g + wd·p; buf = m·buf + d; p -= lr·(nesterov ? d + m·buf : buf)
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ buf, long n4, const float* __restrict__ lr_ptr,
                                                  float momentum, float wd, float gscale, int nesterov) {
  const float lr = lr_ptr[0];
  float4* P = reinterpret_cast<float4*>(p);
  const float4* G = reinterpret_cast<const float4*>(g);
  float4* Bf = reinterpret_cast<float4*>(buf);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 pv = P[i];
    const float4 gv = G[i];
    float4 bv = Bf[i];
    float* pp = reinterpret_cast<float*>(&pv);
    const float* gg = reinterpret_cast<const float*>(&gv);
    float* bb = reinterpret_cast<float*>(&bv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = gscale * gg[k] + wd * pp[k];
      bb[k] = momentum * bb[k] + d;
      const float step = nesterov ? d + momentum * bb[k] : bb[k];
      pp[k] -= lr * step;
    }
    P[i] = pv;
    Bf[i] = bv;
  }
}

__device__ __forceinline__ int find_seg(const long* __restrict__ off, int nseg, long e) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// block-wide sum in a fixed order: xor butterfly inside each wave, then the four wave sums in
// wave order. Every thread returns the same value. `red` holds 4 floats.
__device__ __forceinline__ float block_sum_ordered(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();   // `red` may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// per-block partial sums: part[2*blk] = Σp², part[2*blk+1] = Σ(s·g + wd·p)² (wd only on adapted
// segments) over the block's 4096 elements. No atomics: every block owns its slot, and the sum
// inside a block has a fixed order (16 terms per thread, butterfly, 4 waves), so the norms are
// bit-reproducible from run to run and from rank to rank.
__global__ __launch_bounds__(256) void seg_norms_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                        const long* __restrict__ off, const int* __restrict__ adapt,
                                                        int nseg, long n, float wd, float gscale,
                                                        float* __restrict__ part) {
  __shared__ float red[4];
  // each block handles a contiguous chunk of 4096 elements; chunks never straddle segments
  // because every segment is padded to a multiple of 4096 by the flat-buffer allocator.
  const long base = (long)blockIdx.x * 4096;
  if (base >= n) return;
  const int seg = find_seg(off, nseg, base);
  const float w = adapt[seg] ? wd : 0.f;
  float sp = 0.f, sd = 0.f;
  for (long e = base + threadIdx.x; e < base + 4096 && e < n; e += 256) {
    const float pv = p[e];
    const float d = gscale * g[e] + w * pv;
    sp += pv * pv;
    sd += d * d;
  }
  sp = block_sum_ordered(sp, red);
  sd = block_sum_ordered(sd, red);
  if (threadIdx.x == 0) *reinterpret_cast<float2*>(part + 2 * (long)blockIdx.x) = make_float2(sp, sd);
}

// LARS: d = s·g + wd·p (adapted) | s·g; trust = eta·||p||/||d|| (adapted, both > 0) | 1;
// buf = m·buf + lr·trust·d; p -= buf
// Every block sums the partials of its own segment in index order (thread t takes blocks
// t, t+256, ... of the segment, then the fixed-order block sum): all blocks of a segment get
// the same bits, and the segment's first block stores them to norms[2*seg], norms[2*seg+1].
__global__ __launch_bounds__(256) void lars_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ buf, const long* __restrict__ off,
                                                   const int* __restrict__ adapt, const float* __restrict__ part,
                                                   float* __restrict__ norms, int nseg, long n,
                                                   const float* __restrict__ lr_ptr, float momentum, float wd,
                                                   float gscale, float eta) {
  __shared__ float red[4];
  const float lr = lr_ptr[0];
  const long base = (long)blockIdx.x * 4096;
  if (base >= n) return;
  const int seg = find_seg(off, nseg, base);
  // clamped to the scratch's n/4096 slots whatever the table holds
  const long blk0 = max(off[seg], 0L) / 4096;
  const long blk1 = min(seg + 1 < nseg ? off[seg + 1] : n, n) / 4096;
  float sp = 0.f, sd = 0.f;
  for (long b = blk0 + threadIdx.x; b < blk1; b += 256) {
    const float2 v = *reinterpret_cast<const float2*>(part + 2 * b);
    sp += v.x;
    sd += v.y;
  }
  sp = block_sum_ordered(sp, red);
  sd = block_sum_ordered(sd, red);
  if (blockIdx.x == blk0 && threadIdx.x == 0) {
    norms[2 * seg] = sp;
    norms[2 * seg + 1] = sd;
  }
  const bool ad = adapt[seg] != 0;
  float trust = 1.f;
  if (ad) {
    const float pn = sqrtf(sp), dn = sqrtf(sd);
    if (pn > 0.f && dn > 0.f) trust = eta * pn / dn;
  }
  const float w = ad ? wd : 0.f;
  const float scale = lr * trust;
  for (long e = base + threadIdx.x; e < base + 4096 && e < n; e += 256) {
    const float pv = p[e];
    const float d = gscale * g[e] + w * pv;
    const float b = momentum * buf[e] + scale * d;
    buf[e] = b;
    p[e] = pv - b;
  }
}

}  // namespace

hipError_t launch_sgd(float* p, const float* g, float* buf, long n, const float* lr, float momentum, float wd,
                      float gscale, int nesterov, hipStream_t s, int max_blocks) {
  if (n % 4 != 0) return hipErrorInvalidValue;
  const long n4 = n / 4;
  long grid = (n4 + 255) / 256;
  if (grid > 4096) grid = 4096;
  // a capped grid (grid-stride loop) trickles an early per-bucket update along beside the
  // backward instead of taking every CU for a short burst
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(sgd_kernel, dim3(grid), dim3(256), 0, s, p, g, buf, n4, lr, momentum, wd, gscale, nesterov);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

// n and every seg_off entry are multiples of 4096 (checked by the binding); part holds
// 2 * n/4096 floats, norms 2 * nseg. Both are fully overwritten, nothing needs zeroing.
hipError_t launch_lars(float* p, const float* g, float* buf, const long* seg_off, const int* adapt, int nseg, long n,
                       const float* lr, float momentum, float wd, float gscale, float eta, float* norms, float* part,
                       hipStream_t s) {
  if (n % 4096 != 0 || nseg < 1) return hipErrorInvalidValue;
  const long blocks = n / 4096;
  if (blocks < 1) return hipSuccess;
  hipLaunchKernelGGL(seg_norms_kernel, dim3(blocks), dim3(256), 0, s, p, g, seg_off, adapt, nseg, n, wd, gscale,
                     part);
  SDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(lars_kernel, dim3(blocks), dim3(256), 0, s, p, g, buf, seg_off, adapt, part, norms, nseg, n, lr,
                     momentum, wd, gscale, eta);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}
