// Host-side planning arithmetic of the VICReg loss kernels (vicreg.hip): the supported range, tile
// and grid counts and workspace sizes. Plain C++ (no HIP, no torch) so the launchers and the binding
// layer share one copy.
//
//   cov   C_v[D][D]   = x̄_vᵀ·x̄_v / (N − 1)   symmetric: only the tiles (ti, tj) with ti <= tj are
//                                             computed, T(T + 1)/2 per view, reduction over the batch
//   bwd   dz_v[N][D]  = x̄_v·G_v + …           M = batch, N = D, reduction D, two views in one launch
//
// Both walk their reduction in 32-wide chunks, ascending and never split, so every sum depends
// on (N, D) alone.
//
// The triangle is folded into a rectangle of fold_h x fold_w logical tiles (tri_fold in
// loss_gemm_plan.h), which is walked like any tile grid (grouped_walk): a workgroup finds its tile with
// two divisions, no search.
#pragma once
#include "loss_gemm_plan.h"

namespace sdx_vicreg {

using namespace sdx_lossgemm;   // kChunk, kTile, kTileMB, kGroup, kMinD, kMaxD, kStatCols, kLossRows, supported

struct Plan : BasePlan {
  int c_t, c_fold_w, c_fold_h, c_tiles, c_chunks;   // cov: T, the folded rectangle, tiles per view
  int loss_blocks;                                  // loss_grad grid = slots of the loss partials (both views)
};

inline bool make_plan(int64_t n, int64_t d, Plan* out) {
  Plan p{};
  if (!make_base(n, d, &p)) return false;
  p.c_t = (int)ceil_div(d, kTile);
  p.c_tiles = p.c_t * (p.c_t + 1) / 2;
  p.c_fold_w = p.c_t | 1;
  p.c_fold_h = p.c_tiles / p.c_fold_w;
  p.c_chunks = (int)ceil_div(n, kChunk);
  p.loss_blocks = (int)(2 * d / kLossRows);
  *out = p;
  return true;
}

}  // namespace sdx_vicreg
