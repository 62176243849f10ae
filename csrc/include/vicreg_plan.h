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
// The triangle is folded into a rectangle of fold_h x fold_w logical tiles: rectangle row r holds
// tile row r (T − r tiles) followed by tile row T − r (T odd) resp. T − 1 − r (T even), which has
// the missing r resp. r + 1 tiles. A workgroup finds its tile with two divisions, no search.
#pragma once
#include <stdint.h>

namespace sdx_vicreg {

constexpr int kChunk = 32;       // reduction elements staged per step (one MFMA k-block)
constexpr int kTile = 128;       // cov output tile, rows and columns (2 x 2 waves of 64 x 64)
constexpr int kTileMB = 64;      // bwd output tile rows (2 waves x 32); its columns are kTile
constexpr int kGroup = 4;        // logical tile rows walked together: co-resident tiles share strips in L2
constexpr int kMinD = 64;
constexpr int kMaxD = 8192;
constexpr int kStatCols = 64;    // colstats: columns per block (4 row groups of 64 lanes)
constexpr int kLossRows = 8;     // loss_grad: rows of C_v per block

struct Plan {
  int n, d;
  int c_t, c_fold_w, c_fold_h, c_tiles, c_chunks;   // cov: T, the folded rectangle, tiles per view
  int b_tiles_m, b_tiles_n, b_tiles, b_chunks;      // bwd, per view
  int stat_blocks;                                  // colstats grid
  int loss_blocks;                                  // loss_grad grid = slots of the loss partials (both views)
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
  p.c_t = (int)ceil_div(d, kTile);
  p.c_tiles = p.c_t * (p.c_t + 1) / 2;
  p.c_fold_w = p.c_t | 1;
  p.c_fold_h = p.c_tiles / p.c_fold_w;
  p.c_chunks = (int)ceil_div(n, kChunk);
  p.b_tiles_m = (int)ceil_div(n, kTileMB);
  p.b_tiles_n = (int)ceil_div(d, kTile);
  p.b_tiles = p.b_tiles_m * p.b_tiles_n;
  p.b_chunks = (int)(d / kChunk);
  p.stat_blocks = (int)(d / kStatCols);
  p.loss_blocks = (int)(2 * d / kLossRows);
  *out = p;
  return true;
}

}  // namespace sdx_vicreg
