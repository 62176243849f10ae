// Host-side planning arithmetic of the Barlow Twins loss kernels (barlow.hip): the supported
// range, tile and grid counts and workspace sizes. Plain C++ (no HIP, no torch) so the launchers
// and the binding layer share one copy.
//
//   xcorr  C[D][D]    = ẑ1ᵀ·ẑ2 / N      M = D, N = D, reduction over the batch (transposed staging)
//   bwd    dz_v[N][D] = ẑ_o·G^(ᵀ) / N   M = batch, N = D, reduction D, two views in one launch
//
// Both walk their reduction in 32-wide chunks, ascending and never split, so every sum depends
// on (N, D) alone.
#pragma once
#include "loss_gemm_plan.h"

namespace sdx_barlow {

using namespace sdx_lossgemm;   // kChunk, kTile, kTileMB, kGroup, kMinD, kMaxD, kStatCols, kLossRows, supported

constexpr int kTileMX = kTile;   // xcorr output tile rows (2 waves x 64)

struct Plan : BasePlan {
  int x_tiles_m, x_tiles_n, x_tiles, x_chunks;   // xcorr
  int loss_blocks;                               // loss_grad grid = rows of r2 / loss partials (r1 complete per block)
  int finish_blocks;                             // r2 column blocks + 1 loss block
  int64_t r2_partial_elems;                      // loss_blocks · D
};

inline bool make_plan(int64_t n, int64_t d, Plan* out) {
  Plan p{};
  if (!make_base(n, d, &p)) return false;
  p.x_tiles_m = (int)ceil_div(d, kTileMX);
  p.x_tiles_n = (int)ceil_div(d, kTile);
  p.x_tiles = p.x_tiles_m * p.x_tiles_n;
  p.x_chunks = (int)ceil_div(n, kChunk);
  p.loss_blocks = (int)(d / kLossRows);
  p.finish_blocks = (int)ceil_div(d, 256) + 1;
  p.r2_partial_elems = (int64_t)p.loss_blocks * d;
  *out = p;
  return true;
}

}  // namespace sdx_barlow
