// Host-side planning arithmetic of the DINO loss kernels (dino.hip): the supported range, the row
// block, the tile rows, the split rules of both sweeps and the workspace sizes. Plain C++ (no HIP, no
// torch) so the launchers and the binding layer share one copy; ops/dino.py mirrors it.
//
//   rows    the 2n sample rows of a rank are the two views stacked. Inside the kernels each view is
//           padded to np = 64·ceil(n / 64) rows (rp = 2·np), so a row block or a tile never straddles
//           a view, and student row r goes with teacher row (r + np) mod rp: sample i of teacher view v
//           with sample i of student view 1 − v. Pad rows are zero planes whose saved lse is +inf.
//   tiles   32 streamed rows at D <= 128 and 16 above. A staged tile holds BOTH networks and both bf16
//           planes, so two buffers of 32-row tiles at D = 256 would be 128 KiB; with 16 rows they are
//           64 KiB, which a workgroup names statically. The kernels take 16-row tiles there and do
//           not opt into dynamic LDS; the backward product of a 16-row tile is one
//           v_mfma_f32_16x16x16_bf16 per output tile and plane pair instead of a 16x16x32.
//   k sweep (rows held) the prototype axis is cut as moco_plan.h cuts the queue: row_blocks x k_splits
//           fills kTargetGrid while a span keeps kMinSpanTiles tiles.
//   r sweep (prototypes held) k / 64 workgroups. From kEpilogueBlocks of them on the sample axis is
//           not cut and dV leaves the sweep's epilogue; below, it is cut into spans of at least
//           kMinRowSpanTiles tiles and the slabs go through dino_norm_bwd.
//   Both counts depend on the shape alone and every partial is combined in split order.
//   part    [5][k_splits][rp]: (max_s, sum_s, max_t, sum_t, a). zslab [k_splits][rp][D]. vslab
//           [r_splits][K][D] (r_splits > 1 only).
#pragma once
#include <stdint.h>

namespace sdx_dino {

constexpr int kRowBlock = 64;        // held rows per workgroup: 4 waves x 16
constexpr int kMinD = 64;
constexpr int kMaxD = 256;
constexpr int kMinK = 64;
constexpr int kMaxK = 131072;
constexpr int kTargetGrid = 512;     // two workgroups per CU
constexpr int kMinSpanTiles = 3;
constexpr int kMinRowSpanTiles = 2;
constexpr int kEpilogueBlocks = 64;

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
constexpr int tile_rows(int d) { return d <= 128 ? 32 : 16; }

// tiles -> (span, splits) with no empty span
inline void cut(int64_t tiles, int64_t blocks, int64_t min_span, int* span, int* splits) {
  int64_t s = ceil_div(kTargetGrid, blocks);
  const int64_t max_s = tiles / min_span;
  if (s > max_s) s = max_s;
  if (s < 1) s = 1;
  *span = (int)ceil_div(tiles, s);
  *splits = (int)ceil_div(tiles, *span);
}

struct Plan {
  int n, d, k;          // n: rows per view on this rank
  int np, rp, tk;
  int row_blocks, k_tiles, k_span, k_splits;
  int proto_blocks, r_tiles, r_span, r_splits;
  int64_t part_elems;    // floats: 5·k_splits·rp
  int64_t zslab_elems;   // floats: k_splits·rp·d
  int64_t vslab_elems;   // floats: r_splits·k·d, 0 when the epilogue writes dV
};

inline bool make_plan(int64_t n, int64_t d, int64_t k, Plan* out) {
  if (n < 1 || d < kMinD || d > kMaxD || d % 64 != 0 || k < kMinK || k > kMaxK || k % 64 != 0) return false;
  Plan p{};
  const int64_t np = ceil_div(n, kRowBlock) * kRowBlock;
  if (2 * np * d >= (1LL << 31) || k * d >= (1LL << 31)) return false;
  p.n = (int)n; p.d = (int)d; p.k = (int)k;
  p.np = (int)np; p.rp = (int)(2 * np); p.tk = tile_rows((int)d);
  p.row_blocks = p.rp / kRowBlock;
  p.k_tiles = p.k / p.tk;
  cut(p.k_tiles, p.row_blocks, kMinSpanTiles, &p.k_span, &p.k_splits);
  p.proto_blocks = p.k / kRowBlock;
  p.r_tiles = p.rp / p.tk;
  if (p.proto_blocks >= kEpilogueBlocks) {
    p.r_span = p.r_tiles;
    p.r_splits = 1;
  } else {
    cut(p.r_tiles, p.proto_blocks, kMinRowSpanTiles, &p.r_span, &p.r_splits);
  }
  p.part_elems = 5LL * p.k_splits * p.rp;
  p.zslab_elems = (int64_t)p.k_splits * p.rp * d;
  p.vslab_elems = p.r_splits > 1 ? (int64_t)p.r_splits * k * d : 0;
  if (p.zslab_elems >= (1LL << 31) || p.vslab_elems >= (1LL << 31)) return false;
  *out = p;
  return true;
}

inline bool supported(int64_t n, int64_t d, int64_t k) {
  Plan p;
  return make_plan(n, d, k, &p);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace sdx_dino
