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
#include <stdint.h>

namespace sdx_barlow {

constexpr int kChunk = 32;       // reduction elements staged per step (one MFMA k-block)
constexpr int kTileN = 128;      // output tile columns (2 waves x 64)
constexpr int kTileMX = 128;     // xcorr output tile rows (2 waves x 64)
constexpr int kTileMB = 64;      // bwd output tile rows (2 waves x 32): N = 256 still fills the chip
constexpr int kGroupM = 4;       // tile rows walked together: co-resident tiles share operand strips in L2
constexpr int kMinD = 64;
constexpr int kMaxD = 8192;
constexpr int kStatCols = 64;    // colstats: columns per block (4 row groups of 64 lanes)
constexpr int kLossRows = 8;     // loss_grad: rows of C per block (r1 complete per block)

struct Plan {
  int n, d;
  int x_tiles_m, x_tiles_n, x_tiles, x_chunks;   // xcorr
  int b_tiles_m, b_tiles_n, b_tiles, b_chunks;   // bwd, per view
  int stat_blocks;                               // colstats grid.x (grid.y = 2 views)
  int loss_blocks;                               // loss_grad grid = rows of r2 / loss partials
  int finish_blocks;                             // r2 column blocks + 1 loss block
  int64_t r2_partial_elems;                      // loss_blocks · D
};

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// n: rows on this rank (the kernels' loop bound); the batch size N of the formulas may be larger
inline bool supported(int64_t n, int64_t d) {
  if (n < 1 || d < kMinD || d > kMaxD || d % 64 != 0) return false;
  return n * d < (1LL << 31) && n + kChunk < (1LL << 31);
}

inline bool make_plan(int64_t n, int64_t d, Plan* out) {
  if (!supported(n, d)) return false;
  Plan p{};
  p.n = (int)n;
  p.d = (int)d;
  p.x_tiles_m = (int)ceil_div(d, kTileMX);
  p.x_tiles_n = (int)ceil_div(d, kTileN);
  p.x_tiles = p.x_tiles_m * p.x_tiles_n;
  p.x_chunks = (int)ceil_div(n, kChunk);
  p.b_tiles_m = (int)ceil_div(n, kTileMB);
  p.b_tiles_n = (int)ceil_div(d, kTileN);
  p.b_tiles = p.b_tiles_m * p.b_tiles_n;
  p.b_chunks = (int)(d / kChunk);
  p.stat_blocks = (int)(d / kStatCols);
  p.loss_blocks = (int)(d / kLossRows);
  p.finish_blocks = (int)ceil_div(d, 256) + 1;
  p.r2_partial_elems = (int64_t)p.loss_blocks * d;
  *out = p;
  return true;
}

}  // namespace sdx_barlow
