// Host-side planning arithmetic that the two-view pretraining losses share (barlow_plan.h,
// vicreg_plan.h): the tile constants, the supported range, the backward plan, and the two maps from
// a logical tile number to a tile, which the kernels call too. Plain C++ (no HIP, no torch) so the
// launchers, the binding layer and the stand-alone check (csrc/tools/loss_gemm_plan_check.cpp) share
// one copy.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SDX_HOST_DEVICE __host__ __device__
#else
#define SDX_HOST_DEVICE
#endif

namespace sdx_lossgemm {

constexpr int kChunk = 32;       // reduction elements staged per step (one MFMA k-block)
constexpr int kTile = 128;       // output tile columns (2 waves x 64); rows too where the tile is square
constexpr int kTileMB = 64;      // bwd output tile rows (2 waves x 32): N = 256 still fills the chip
constexpr int kGroup = 4;        // logical tile rows walked together: co-resident tiles share operand strips in L2
constexpr int kMinD = 64;
constexpr int kMaxD = 8192;
constexpr int kStatCols = 64;    // colstats: columns per block (4 row groups of 64 lanes)
constexpr int kLossRows = 8;     // loss_grad: rows of C per block

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }   // float4 access: checked by the launchers

// n: rows on this rank (the kernels' loop bound); the batch size N of the formulas may be larger
inline bool supported(int64_t n, int64_t d) {
  if (n < 1 || d < kMinD || d > kMaxD || d % 64 != 0) return false;
  return n * d < (1LL << 31) && n + kChunk < (1LL << 31);
}

// What both losses plan alike. bwd: dz_v[N][D], M = batch, N = D, reduction D, two views in one launch.
struct BasePlan {
  int n, d;
  int b_tiles_m, b_tiles_n, b_tiles, b_chunks;   // bwd, per view
  int stat_blocks;                               // colstats grid.x
};

inline bool make_base(int64_t n, int64_t d, BasePlan* p) {
  if (!supported(n, d)) return false;
  p->n = (int)n;
  p->d = (int)d;
  p->b_tiles_m = (int)ceil_div(n, kTileMB);
  p->b_tiles_n = (int)ceil_div(d, kTile);
  p->b_tiles = p->b_tiles_m * p->b_tiles_n;
  p->b_chunks = (int)(d / kChunk);
  p->stat_blocks = (int)(d / kStatCols);
  return true;
}

struct TilePos {
  int row, col;
};

// Logical tile lt of a rows x cols grid: `group` tile rows down, then the next tile column, then the
// next group of rows. Consecutive logical tiles of a group share the tile column, and a group's
// tiles share `group` row strips.
SDX_HOST_DEVICE inline TilePos grouped_walk(int lt, int rows, int cols, int group) {
  const int per = group * cols;
  const int grp = lt / per, in = lt - grp * per;
  const int first = grp * group;
  const int left = rows - first;
  const int h = left < group ? left : group;   // rows of this (the last: maybe short) group
  const int col = in / h;
  return {first + (in - col * h), col};
}

// The triangle ti <= tj < T of a symmetric T x T tile grid, folded into a rectangle of T(T + 1)/2
// tiles, (T | 1) wide: rectangle row r holds tile row r (its T − r tiles from the diagonal on)
// followed by tile row T − r (T odd) resp. T − 1 − r (T even), which has the missing r resp. r + 1
// tiles. (r, col) of the rectangle -> (ti, tj) as (row, col).
SDX_HOST_DEVICE inline TilePos tri_fold(int r, int col, int T) {
  const int cut = T - r;   // tiles of tile row r
  if (col < cut) return {r, r + col};
  const int ti = cut - 1 + (T & 1);
  return {ti, ti + (col - cut)};
}

}  // namespace sdx_lossgemm
