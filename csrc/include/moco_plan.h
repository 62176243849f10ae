// Host-side planning arithmetic of the MoCo loss kernels (moco.hip): the supported range, the row
// block, the queue tile, the split of the queue axis and the workspace sizes. Plain C++ (no HIP, no
// torch) so the launchers and the binding layer share one copy.
//
//   sweep   a workgroup owns kRowBlock q rows (a wave 16 of them, their hi/lo fragments in registers)
//           and ONE contiguous span of the queue, span_tiles tiles of kTileRows rows. Two LDS buffers
//           of both bf16 planes of a tile are 2·2·kTileRows·2·D bytes: 64 KiB at the largest D.
//   splits  the queue axis is cut so that row_blocks x splits fills the chip (kTargetGrid workgroups)
//           while a span keeps at least kMinSpanTiles tiles. The count depends on (N, K) alone, and the
//           partials are combined in split order: runs are bit-identical.
//   part    [splits][N] (max, sumexp) pairs of the forward; slab [splits][N][D], the dq̂ partials.
#pragma once
#include <stdint.h>

namespace sdx_moco {

constexpr int kRowBlock = 64;        // q rows per workgroup: 4 waves x 16
constexpr int kTileRows = 32;        // queue rows per LDS tile: one MFMA k-block of the backward product
constexpr int kMinD = 64;
constexpr int kMaxD = 256;
constexpr int kMinK = 64;
constexpr int kMaxK = 1 << 20;
constexpr int kTargetGrid = 512;     // two workgroups per CU
constexpr int kMinSpanTiles = 3;

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct Plan {
  int n, d, k;
  int row_blocks, tiles, span_tiles, splits;
  int64_t part_elems;   // floats: splits·n·2
  int64_t slab_elems;   // floats: splits·n·d
};

// n: q rows on this rank
inline bool make_plan(int64_t n, int64_t d, int64_t k, Plan* out) {
  if (n < 1 || d < kMinD || d > kMaxD || d % 64 != 0 || k < kMinK || k > kMaxK || k % 64 != 0) return false;
  if (n * d >= (1LL << 31) || k * d >= (1LL << 31)) return false;
  Plan p{};
  p.n = (int)n; p.d = (int)d; p.k = (int)k;
  p.row_blocks = (int)ceil_div(n, kRowBlock);
  p.tiles = (int)(k / kTileRows);
  int64_t s = ceil_div(kTargetGrid, p.row_blocks);
  const int64_t max_s = p.tiles / kMinSpanTiles;
  if (s > max_s) s = max_s;
  if (s < 1) s = 1;
  p.span_tiles = (int)ceil_div(p.tiles, s);
  p.splits = (int)ceil_div(p.tiles, p.span_tiles);   // no empty span
  p.part_elems = (int64_t)p.splits * n * 2;
  p.slab_elems = (int64_t)p.splits * n * d;
  if (p.slab_elems >= (1LL << 31)) return false;
  *out = p;
  return true;
}

inline bool supported(int64_t n, int64_t d, int64_t k) {
  Plan p;
  return make_plan(n, d, k, &p);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace sdx_moco
