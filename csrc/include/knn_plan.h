// Host-side planning arithmetic of the k-NN top-k kernels (knn.hip): split counts, rows per
// split and workspace sizes. Plain C++ (no HIP, no torch) so the binding layer, the launcher
// and the stand-alone sanitizer check (csrc/tools/knn_plan_check.cpp) share one copy.
#pragma once
#include <stdint.h>

namespace sdx_knn {

constexpr int kQueryTile = 64;    // queries per workgroup (4 waves x 16)
constexpr int kBankTile = 64;     // bank rows per LDS tile
constexpr int kMaxK = 256;        // list capacity per query
constexpr int kMaxSplits = 64;
constexpr int kMaxClasses = 1024;
constexpr int kNumCu = 256;       // MI355X

struct Plan {
  int n_split;          // bank splits actually launched (every one non-empty)
  int rows_per_split;   // multiple of kBankTile
  int64_t slab_elems;   // per-split list slab elements: n_split * nq * k (0 when n_split == 1)
};

inline bool dim_supported(int64_t D) {
  return D >= 64 && D <= 2048 && D % 64 == 0 && (((D / 64) & (D / 64 - 1)) == 0);
}

inline bool supported(int64_t D, int64_t n_cls, int64_t k) {
  return dim_supported(D) && n_cls >= 1 && n_cls <= kMaxClasses && k >= 1 && k <= kMaxK;
}

// Split count that fills the chip: the fewest splits whose workgroups cover >= 90 % of the
// CU slots of their last round (one workgroup per CU at the largest list), each split
// keeping at least 4 bank tiles.
inline int auto_splits(int64_t nq, int64_t nb) {
  const int64_t qt = (nq + kQueryTile - 1) / kQueryTile;
  int64_t cap = nb / (4 * kBankTile);
  if (cap > kMaxSplits) cap = kMaxSplits;
  if (cap < 1) cap = 1;
  int best = 1;
  double best_eff = 0.0;
  for (int64_t s = 1; s <= cap; ++s) {
    const int64_t wgs = qt * s;
    const int64_t rounds = (wgs + kNumCu - 1) / kNumCu;
    const double eff = (double)wgs / (double)(rounds * kNumCu);
    if (eff >= 0.9) return (int)s;
    if (eff > best_eff) { best_eff = eff; best = (int)s; }
  }
  return best;
}

// n_split_req: 0 = automatic. Returns false when an argument is out of range.
inline bool make_plan(int64_t nq, int64_t nb, int64_t k, int64_t n_split_req, Plan* out) {
  if (nq < 1 || nb < 1 || k < 1 || k > kMaxK || k > nb || n_split_req < 0 || n_split_req > kMaxSplits) return false;
  if (nq > (1LL << 30) || nb > (1LL << 30)) return false;
  int64_t s = n_split_req > 0 ? n_split_req : auto_splits(nq, nb);
  int64_t per = (nb + s - 1) / s;
  per = ((per + kBankTile - 1) / kBankTile) * kBankTile;
  s = (nb + per - 1) / per;
  out->n_split = (int)s;
  out->rows_per_split = (int)per;
  out->slab_elems = s > 1 ? s * nq * k : 0;
  return true;
}

}  // namespace sdx_knn
