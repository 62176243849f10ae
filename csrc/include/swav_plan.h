// Host-side planning arithmetic of the SwAV loss kernels (swav.hip): the supported range, the
// padded leading dimension of the score matrix, tile and grid counts and workspace sizes. Plain C++
// (no HIP, no torch) so the launchers and the binding layer share one copy.
//
//   scores  S_v[N][Kp]  = ẑ_v·Cᵀ        M = N per view, N = K, reduction D, two views in one launch
//   dzhat   dẑ[2N][D]   = dS·C          M = 2N, N = D, reduction Kp (the padding of dS is zero)
//   dproto  dC[K][D]    = dSᵀ·ẑ         M = K, N = D, reduction 2N: both views at once
//
// All three walk their reduction in 32-wide chunks, ascending and never split. The Sinkhorn kernel
// owns kStrip sample rows of one view per workgroup (a wave kStrip / 4 of them) and writes one row of
// the next prototype sum's partials per strip; the score kernel writes one per 64-row tile.
#pragma once
#include "loss_gemm_plan.h"

namespace sdx_swav {

using sdx_lossgemm::aligned16;
using sdx_lossgemm::ceil_div;
using sdx_lossgemm::grouped_walk;
using sdx_lossgemm::kChunk;
using sdx_lossgemm::kGroup;
using sdx_lossgemm::kTile;
using sdx_lossgemm::TilePos;

constexpr int kTileM = 64;       // output tile rows of every GEMM here (2 waves x 32)
constexpr int kPad = 64;         // leading dimension of S and dS: K rounded up to this, the padding zero
constexpr int kStrip = 16;       // Sinkhorn: sample rows per workgroup
constexpr int kWaveRows = 4;     // rows a wave carries together: one u_k serves all of them
constexpr int kMinD = 64;
constexpr int kMaxD = 2048;
constexpr int kMinK = 2;
constexpr int kMaxK = 16384;
static_assert(kStrip == 4 * kWaveRows, "a workgroup is 4 waves");

inline int64_t padded(int64_t k) { return ceil_div(k, kPad) * kPad; }

// n: sample rows per view on this rank
inline bool supported(int64_t n, int64_t d, int64_t k, int64_t iters = 1) {
  if (n < 2 || d < kMinD || d > kMaxD || d % 64 != 0 || k < kMinK || k > kMaxK || iters < 1) return false;
  return 2 * n * padded(k) < (1LL << 31) && 2 * n * d < (1LL << 31);
}

struct Plan {
  int n, d, k, kp;
  int s_tiles_m, s_tiles_n, s_tiles, s_chunks;   // scores, per view; s_tiles_m rows of first-r partials
  int strips;                                    // Sinkhorn workgroups per view = rows of its partials
  int z_tiles_m, z_tiles_n, z_chunks;            // dzhat
  int c_tiles_m, c_tiles_n, c_chunks;            // dproto
};

inline bool make_plan(int64_t n, int64_t d, int64_t k, Plan* out) {
  if (!supported(n, d, k)) return false;
  Plan p{};
  p.n = (int)n; p.d = (int)d; p.k = (int)k; p.kp = (int)padded(k);
  p.s_tiles_m = (int)ceil_div(n, kTileM);
  p.s_tiles_n = (int)ceil_div(p.kp, kTile);
  p.s_tiles = p.s_tiles_m * p.s_tiles_n;
  p.s_chunks = (int)(d / kChunk);
  p.strips = (int)ceil_div(n, kStrip);
  p.z_tiles_m = (int)ceil_div(2 * n, kTileM);
  p.z_tiles_n = (int)ceil_div(d, kTile);
  p.z_chunks = p.kp / kChunk;
  p.c_tiles_m = (int)ceil_div(k, kTileM);
  p.c_tiles_n = (int)ceil_div(d, kTile);
  p.c_chunks = (int)ceil_div(2 * n, kChunk);
  *out = p;
  return true;
}

}  // namespace sdx_swav
