// What the dedicated weight-gradient kernels (wgrad1x1.hip, wgrad3x3.hip) share around their
// operand loaders and pipelines: the block -> (tile, K-split) decode, the lane decomposition,
// the transposed fragment read, the D = Bᵀ·Aᵀ MFMA nest and the fp32 partial-slab stores.
// Internal linkage, as mfma_lds.h; only those two units include it.
#pragma once

#include <type_traits>

#include "common.h"
#include "mfma_lds.h"

namespace {

// Split-K geometry both parameter structs embed (after their pointers, which stay first and
// aligned for the kernel-argument loads): 32-pixel steps, output tiles, splits
struct WgSplit {
  int steps_total;      // dy pixels (3x3 pad kernels: pixel slots) / 32
  int steps_per_split;
  int k_tiles, c_tiles, splits;
};

struct WgTile {
  int k0, c0;           // first output channel (dW row) and input channel of the block's tile
  int split;
  int s_begin, s_end;   // the split's steps
};

// tile / split of this block (split-major: an XCD's co-resident blocks share one pixel range)
template <int BM, int BN>
__device__ __forceinline__ WgTile wg_tile(const WgSplit& g) {
  const int tiles = g.k_tiles * g.c_tiles;
  const int lin = sdx::xcd_remap(blockIdx.x, gridDim.x);
  const int tile = lin % tiles, split = lin / tiles;
  const int s_begin = split * g.steps_per_split;
  return {(tile / g.c_tiles) * BM, (tile % g.c_tiles) * BN, split, s_begin,
          min(g.steps_total, s_begin + g.steps_per_split)};
}

// 512 threads = 8 waves, 2 (output rows, wm) x 4 (output columns, wn). Fragment addressing:
// lane (h4, c16 = 4q + pp) reads K rows (pixels) p_lo = 8h4 + q and p_lo + 4, columns
// col0 + 4pp .. +3 (ds_read_b64_tr_b16 transposes across the 4 q-lanes); in the accumulators
// it holds output row c16, columns 4h4 .. +3 of each 16 x 16 tile
struct WgLane {
  int lane, wv, h4, c16, wm, wn, q, pp, p_lo;
  __device__ __forceinline__ explicit WgLane(int tid)
      : lane(tid & 63), wv(tid >> 6), h4(lane >> 4), c16(lane & 15), wm(wv >> 2), wn(wv & 3), q(c16 >> 2),
        pp(c16 & 3), p_lo(8 * h4 + q) {}
};

// One MFMA operand fragment: the transposed halves of pixel rows p_lo and p_lo + 4
__device__ __forceinline__ sdx::bf16x8 wg_frag_at(const unsigned char* lo_p, const unsigned char* hi_p) {
  const sdx::bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)lo_p);
  const sdx::bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)hi_p);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ sdx::bf16x8 wg_frag(const unsigned char* base, int o_lo, int o_hi) {
  return wg_frag_at(base + o_lo, base + o_hi);
}
// the half of row p_lo + 4 a constant HI bytes further (an immediate ds_read offset): images
// whose swizzle ignores row bit 2
template <int HI>
__device__ __forceinline__ sdx::bf16x8 wg_frag(const unsigned char* base, int o) {
  return wg_frag_at(base + o, base + o + HI);
}

template <int TM, int TN>
__device__ __forceinline__ void wg_zero(sdx::f32x4 (&acc)[TM][TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = sdx::f32x4{0.f, 0.f, 0.f, 0.f};
}

// The MFMA is issued as D = Bᵀ·Aᵀ (igemm_kernel.h's convention), so each lane holds 4
// consecutive output columns of one output row
template <int TM, int TN>
__device__ __forceinline__ void wg_mfma(const sdx::bf16x8 (&fa)[TM], const sdx::bf16x8 (&fb)[TN],
                                        sdx::f32x4 (&acc)[TM][TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
}

// ---- epilogues: fp32 partial rows, 4 consecutive columns per lane; a wave owns 16·TM rows ----
__device__ __forceinline__ void wg_st4(float* o, const sdx::f32x4& a) {
  st16<SDX_NT_PART != 0>(o, make_uint4(__float_as_uint(a[0]), __float_as_uint(a[1]), __float_as_uint(a[2]),
                                       __float_as_uint(a[3])));
}

// 1x1: part = [splits][K][C]; the wave's columns are c0 + wn·16·TN ..
template <int TM, int TN>
__device__ __forceinline__ void wg_store_1x1(const sdx::f32x4 (&acc)[TM][TN], float* part, int K, int C,
                                             const WgTile& t, const WgLane& L) {
  float* out = part + (size_t)t.split * K * C;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = t.k0 + L.wm * (16 * TM) + 16 * i + L.c16;
    float* row = out + (size_t)m * C;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = t.c0 + L.wn * (16 * TN) + 16 * j + 4 * L.h4;
      wg_st4(row + n, acc[i][j]);
    }
  }
}

// 1x1 over the pixel-pair view: the diagonal blocks only: row m of dy half e = m / K0, column
// n of x half n / C0 (4 consecutive columns never straddle C0, a multiple of 64), into slices
// 2·split + e of a [2·splits][K0][C0] slab
template <int TM, int TN>
__device__ __forceinline__ void wg_store_pairs(const sdx::f32x4 (&acc)[TM][TN], float* part, int K0, int C0,
                                               const WgTile& t, const WgLane& L) {
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = t.k0 + L.wm * (16 * TM) + 16 * i + L.c16;
    const int e = m >= K0;
    float* row = part + ((size_t)(2 * t.split + e) * K0 + (m - e * K0)) * C0;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = t.c0 + L.wn * (16 * TN) + 16 * j + 4 * L.h4;
      if ((n >= C0) != e) continue;
      wg_st4(row + (n - e * C0), acc[i][j]);
    }
  }
}

// 3x3: part = [splits][K][9·C], tap-major columns; the wave's 144 of the tile's 576 columns
// are 9 tiles of (one tap n >> 6, 16 channels): 4 consecutive columns share a tap
__device__ __forceinline__ void wg_store_3x3(const sdx::f32x4 (&acc)[2][9], float* part, int K, int C,
                                             const WgTile& t, const WgLane& L) {
  const int Ncol = 9 * C;
  float* out = part + (size_t)t.split * K * Ncol;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = t.k0 + L.wm * 32 + 16 * i + L.c16;
    float* row = out + (size_t)m * Ncol + t.c0;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int n = L.wn * 144 + 16 * j + 4 * L.h4;
      wg_st4(row + (n >> 6) * C + (n & 63), acc[i][j]);
    }
  }
}

// ---- register rings: every value is a named register selected at compile time (an array
// indexed inside the loader lambdas goes to scratch) ----
template <int I>
using WgI = std::integral_constant<int, I>;

// slot S of the named slots s0, s1, ...
template <int S, class T, class... Rest>
__device__ __forceinline__ T& wg_slot(T& s0, Rest&... rest) {
  if constexpr (S == 0) return s0;
  else return wg_slot<S - 1>(rest...);
}

}  // namespace
