// Host-side planning arithmetic of the NNCLR kernels (nnclr.hip): the supported range, the row block,
// the streamed tile, the three cuts of a streamed axis and the workspace sizes. Plain C++ (no HIP, no
// torch) so the launchers and the binding layer share one copy.
//
//   search  2n query rows (both views of this rank) against the K queue rows: ceil(2n / 64) row blocks
//           x k_splits spans of the queue axis, one (value, index) pair per (split, row).
//   fwd     per view, ceil(n / 64) blocks of held neighbour rows x f_splits spans of the N streamed p̂
//           rows of the other view, one (max, sumexp) pair per (split, row).
//   bwd     per view, ceil(N / 64) blocks of held p̂ rows x b_splits spans of the n streamed neighbour
//           rows, one dp̂ slab [2N][D] per split.
//   cut     an axis of `tiles` 32-row tiles is cut so that blocks x splits fills the chip (kTargetGrid
//           workgroups) while a span keeps at least kMinSpanTiles tiles. Every count depends on the sizes
//           alone, and the partials are combined in split order: runs are bit-identical.
#pragma once
#include <stdint.h>

namespace sdx_nnclr {

constexpr int kRowBlock = 64;        // held rows per workgroup: 4 waves x 16
constexpr int kTileRows = 32;        // streamed rows per LDS tile: one MFMA k-block of the backward product
constexpr int kMinD = 64;
constexpr int kMaxD = 256;
constexpr int kMinK = 64;
constexpr int kMaxK = 1 << 20;
constexpr int kTargetGrid = 512;     // two workgroups per CU
constexpr int kMinSpanTiles = 3;

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct Cut {
  int blocks, tiles, span_tiles, splits;
};

// blocks: all the workgroups of one split (both views where the grid has them)
inline Cut cut(int64_t blocks, int64_t rows_per_grid_z, int64_t tiles) {
  Cut c{};
  c.blocks = (int)blocks;
  c.tiles = (int)tiles;
  int64_t s = ceil_div(kTargetGrid, blocks * rows_per_grid_z);
  const int64_t max_s = tiles / kMinSpanTiles;
  if (s > max_s) s = max_s;
  if (s < 1) s = 1;
  c.span_tiles = (int)ceil_div(tiles, s);
  c.splits = (int)ceil_div(tiles, c.span_tiles);   // no empty span
  return c;
}

struct Plan {
  int n, N, d, k;
  Cut search, fwd, bwd;
  int64_t pair_elems;   // floats: search.splits·2n·2
  int64_t part_elems;   // floats: fwd.splits·2n·2
  int64_t slab_elems;   // floats: bwd.splits·2N·d
};

// n: rows of this rank per view, N: rows of the global batch per view
inline bool make_plan(int64_t n, int64_t N, int64_t d, int64_t k, Plan* out) {
  if (n < 1 || N < n || d < kMinD || d > kMaxD || d % 64 != 0 || k < kMinK || k > kMaxK || k % 64 != 0) return false;
  if (2 * N * d >= (1LL << 31) || k * d >= (1LL << 31)) return false;
  Plan p{};
  p.n = (int)n; p.N = (int)N; p.d = (int)d; p.k = (int)k;
  p.search = cut(ceil_div(2 * n, kRowBlock), 1, k / kTileRows);
  p.fwd = cut(ceil_div(n, kRowBlock), 2, ceil_div(N, kTileRows));
  p.bwd = cut(ceil_div(N, kRowBlock), 2, ceil_div(n, kTileRows));
  p.pair_elems = (int64_t)p.search.splits * 2 * n * 2;
  p.part_elems = (int64_t)p.fwd.splits * 2 * n * 2;
  p.slab_elems = (int64_t)p.bwd.splits * 2 * N * d;
  if (p.pair_elems >= (1LL << 31) || p.part_elems >= (1LL << 31) || p.slab_elems >= (1LL << 31)) return false;
  *out = p;
  return true;
}

inline bool supported(int64_t n, int64_t N, int64_t d, int64_t k) {
  Plan p;
  return make_plan(n, N, d, k, &p);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace sdx_nnclr
