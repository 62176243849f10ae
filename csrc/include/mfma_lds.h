// Device primitives shared by the MFMA GEMM kernels that stage operands in LDS
// (igemm_kernel.h, wgrad1x1.hip, wgrad3x3.hip). Everything here has internal linkage: each
// including unit gets its own zero page (no -fgpu-rdc, a device global cannot be shared).
#pragma once

#include "common.h"

namespace {

typedef __attribute__((address_space(3))) sdx::bf16x4 lds_bf16x4;

// K-outer image: [BK][COLS] bf16; chunk swizzle keeps the transposed reads of a 32-lane
// half (8 rows x 2 chunks) on distinct banks.
template <int COLS>
__device__ __forceinline__ int kout_swz(int row) {
  if (COLS >= 128) return ((row & 3) | (((row >> 3) & 1) << 2)) << 1;
  return (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1;
}

// 16 zero bytes in global memory: out-of-bounds operand chunks (padding taps, tail rows,
// K tail) load from here instead of being skipped, so every staging load is unconditional.
// A predicated load makes hipcc branch around it and drain the whole load queue
// (vmcnt(0)) before the LDS write, which defeats any prefetch depth.
__device__ __attribute__((aligned(16))) uint16_t g_zero16[8];
// g_zero16's address in an SGPR pair the compiler cannot rematerialise: otherwise it re-runs
// s_getpc + a GOT s_load + s_waitcnt lgkmcnt(0) before every zero-page select of the K loop
typedef const __attribute__((address_space(1))) uint16_t* gptr16;
__device__ __forceinline__ gptr16 opaque_zero() {
  gptr16 z = (gptr16)g_zero16;
  asm volatile("" : "+s"(z));
  return z;
}

// s_waitcnt vmcnt(N) alone (expcnt / lgkmcnt at their maxima); gfx9 encoding: vmcnt in
// bits [3:0] + [15:14], expcnt [6:4], lgkmcnt [11:8]
template <int N>
__device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
  asm volatile("" ::: "memory");
}

// raw workgroup barrier: this wave's LDS reads complete first; LDS-DMA stays in flight
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

}  // namespace
