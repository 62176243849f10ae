// Host-side planning arithmetic of the MFMA classifier head (head_gemm.hip): the supported
// range, the padded extents, tile and grid counts of the three GEMM forms and the workspace
// sizes. Plain C++ (no HIP, no torch) so the launchers, the binding layer and the stand-alone
// sanitizer check (csrc/tools/head_gemm_plan_check.cpp) share one copy.
//
//   NT  logits[G][B][C] : M = B,    N = G·C, reduction K
//   NN  dX[B][K]        : M = B,    N = K,   reduction C   (single head only)
//   TN  Gw[G·C][K]      : M = G·C,  N = K,   reduction B
//
// Every form uses the same 64 x 64 output tile and walks its reduction in 64-wide chunks in
// ascending order, with no split: tile shape and summation order depend on (B, K, C) alone,
// G only stretches the G·C extent. One output element is accumulated in the same order
// wherever it sits in its tile, so head g of a sweep is bit-identical to that head alone.
#pragma once
#include <stdint.h>

namespace sdx_headgemm {

constexpr int kTile = 64;        // output tile edge (4 waves x 16 columns, 4 x 16 rows each)
constexpr int kChunk = 64;       // reduction elements staged per step
constexpr int kMinK = 64;
constexpr int kMaxK = 4096;
constexpr int kMaxC = 32768;
constexpr int kMaxHeads = 16;
constexpr int kRowsPerBlock = 4; // ce_rows: one wave per logits row
constexpr int kBiasPerBlock = 256;

struct Form {
  int m, n, red;        // output rows, output columns, reduction length
  int tiles_m, tiles_n; // ceil(m / kTile), ceil(n / kTile)
  int red_pad;          // reduction length padded with zeros to a multiple of kChunk
  int chunks;           // red_pad / kChunk
  int tiles;            // tiles_m * tiles_n = GEMM blocks of the launch
};

struct Plan {
  Form nt, nn, tn;
  int rows;             // G·B logits rows
  int row_blocks;       // ce_rows grid
  int bias_blocks;      // role blocks after the TN tiles: bias columns, the last one also the statistics
  int64_t logits_elems; // G·B·C (logits, dz)
  int64_t rowstat_elems;// G·B·3
};

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline bool supported(int64_t G, int64_t B, int64_t K, int64_t C) {
  if (G < 1 || G > kMaxHeads || B < 1 || C < 1 || C > kMaxC) return false;
  if (K < kMinK || K > kMaxK || K % kChunk != 0) return false;
  const int64_t lim = 1LL << 31;
  if (B >= lim) return false;
  // element counts, the padded reduction over B included (index arithmetic stays in int)
  return G * B * C < lim && B * K < lim && G * C * K < lim && G * B * 3 < lim && B + kChunk < lim;
}

inline Form make_form(int64_t m, int64_t n, int64_t red) {
  Form f{};
  f.m = (int)m;
  f.n = (int)n;
  f.red = (int)red;
  f.tiles_m = (int)ceil_div(m, kTile);
  f.tiles_n = (int)ceil_div(n, kTile);
  f.chunks = (int)ceil_div(red, kChunk);
  f.red_pad = f.chunks * kChunk;
  f.tiles = f.tiles_m * f.tiles_n;
  return f;
}

// Returns false (and leaves *out alone) outside the supported range.
inline bool make_plan(int64_t G, int64_t B, int64_t K, int64_t C, Plan* out) {
  if (!supported(G, B, K, C)) return false;
  Plan p{};
  p.nt = make_form(B, G * C, K);
  p.nn = make_form(B, K, C);
  p.tn = make_form(G * C, K, B);
  p.rows = (int)(G * B);
  p.row_blocks = (int)ceil_div(G * B, kRowsPerBlock);
  p.bias_blocks = (int)ceil_div(G * C, kBiasPerBlock);
  p.logits_elems = G * B * C;
  p.rowstat_elems = G * B * 3;
  *out = p;
  return true;
}

}  // namespace sdx_headgemm
