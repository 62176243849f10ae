// Device code of the two-view pretraining losses on the staging of bf16x3_stage.h: the double-buffered
// chunk loop of a TM x 128 output tile (vicreg.hip; barlow.hip keeps its one-buffer loop, see
// profiles/loss_gemm_share.txt) and the row-group sum of both units' column statistics. The maps from a
// logical tile number to a tile (grouped_walk, tri_fold) are host code too and live in loss_gemm_plan.h.
#pragma once
#include "bf16x3_stage.h"
#include "loss_gemm_plan.h"

namespace sdx_stage {

constexpr int kTileN = sdx_lossgemm::kTile;
static_assert(kStageChunk == sdx_lossgemm::kChunk, "the staging header's chunk is the plan's");

// A workgroup is 4 waves, 2 x 2 over the tile: wave (wm, wn) owns (TM/2) x 64 of it. In a wave, h is the
// 16-lane group (reduction sub-block of the fragments, row group of the accumulator) and c the
// fragment row / accumulator column. The loop and the epilogues each spell these four out: routed
// through one function (by value, by reference, typed as either call site), the compiler scheduled
// the staging of vic_cov and vic_bwd differently and both measured up to 2 % slower
// (profiles/loss_gemm_share.txt).
//
// TM x 128 tile at (m0, n0): acc[t][u][r] = Σ_k a[m0 + wm·TM/2 + 16t + 4h + r][k]·b[n0 + 64·wn + 16u + c][k],
// the reduction in 32-wide chunks, ascending. `stage` holds two buffers of (A hi, A lo, B hi, B lo):
// chunk k + 1 is loaded before the MFMAs of chunk k, stays raw in registers under them and is committed
// after them to the other buffer, so there is ONE barrier per chunk.
// DIAG: b is a, staged once. skip: this wave stages and synchronises but issues no MFMAs.
template <int TM, int MA, int SA, int MB, int SB, bool DIAG>
__device__ __forceinline__ void mma_tile(const Operand& a, const Operand& b, int m0, int n0, int chunks, bool skip,
                                         unsigned char* stage, f32x4 (&acc)[TM / 32][4]) {
  static_assert(!DIAG || TM == kTileN, "a diagonal tile is square");
  constexpr int TN = kTileN;
  constexpr int ROW_B = kStageRowB;
  constexpr int MT = TM / 32;
  constexpr int A_B = 2 * TM * ROW_B;                       // bytes of A's two images
  constexpr int BUF = A_B + (DIAG ? 0 : 2 * TN * ROW_B);    // one buffer
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int wm = wv >> 1, wn = wv & 1;
  const int h = lane >> 4;
  const int c = lane & 15;

  Stager<MA, SA, TM> sa;
  Stager<MB, SB, TN> sb;
  sa.init(a, m0, tid);
  sa.load(a, 0);
  if constexpr (!DIAG) {
    sb.init(b, n0, tid);
    sb.load(b, 0);
  }
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};

  sa.commit(a, 0, stage, stage + TM * ROW_B);
  if constexpr (!DIAG) sb.commit(b, 0, stage + A_B, stage + A_B + TN * ROW_B);

  for (int kc = 0; kc < chunks; ++kc) {
    unsigned char* cur = stage + (kc & 1) * BUF;
    unsigned char* nxt = stage + ((kc + 1) & 1) * BUF;
    // chunk kc is visible, and every wave is done reading the buffer that chunk kc + 1 goes to
    __syncthreads();
    const bool more = kc + 1 < chunks;
    if (more) {   // the next chunk's loads fly under this chunk's MFMAs
      sa.load(a, (kc + 1) * kStageChunk);
      if constexpr (!DIAG) sb.load(b, (kc + 1) * kStageChunk);
    }
    if (!skip) {
      const unsigned char* a_hi = cur;
      const unsigned char* a_lo = cur + TM * ROW_B;
      const unsigned char* b_hi = DIAG ? a_hi : cur + A_B;
      const unsigned char* b_lo = DIAG ? a_lo : cur + A_B + TN * ROW_B;
      bf16x8 o_hi[4], o_lo[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int boff = sw_off(wn * 64 + 16 * u + c, h);
        o_hi[u] = *reinterpret_cast<const bf16x8*>(b_hi + boff);
        o_lo[u] = *reinterpret_cast<const bf16x8*>(b_lo + boff);
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const int aoff = sw_off(wm * (TM / 2) + 16 * t + c, h);
        const bf16x8 f_hi = *reinterpret_cast<const bf16x8*>(a_hi + aoff);
        const bf16x8 f_lo = *reinterpret_cast<const bf16x8*>(a_lo + aoff);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f_hi, o_hi[u], acc[t][u], 0, 0, 0);
          acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f_hi, o_lo[u], acc[t][u], 0, 0, 0);
          acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f_lo, o_hi[u], acc[t][u], 0, 0, 0);
        }
      }
    }
    if (more) {
      sa.commit(a, (kc + 1) * kStageChunk, nxt, nxt + TM * ROW_B);
      if constexpr (!DIAG) sb.commit(b, (kc + 1) * kStageChunk, nxt + A_B, nxt + A_B + TN * ROW_B);
    }
  }
}

// Column statistics: a block owns 64 columns, its 4 row groups (waves) rows n ≡ rg (mod 4). K fp64
// partials per thread -> row group 0 holds the sums, the 4 groups added in wave order; returns
// whether this thread is of row group 0.
template <int K>
__device__ __forceinline__ bool add_row_groups(double (&v)[K]) {
  __shared__ double part[K][4][sdx_lossgemm::kStatCols];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) part[k][rg][cl] = v[k];
  __syncthreads();
  if (rg == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((part[k][0][cl] + part[k][1][cl]) + part[k][2][cl]) + part[k][3][cl];
  }
  return rg == 0;
}

}  // namespace sdx_stage
