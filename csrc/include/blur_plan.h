// Host-side size arithmetic of the Gaussian-blur augmentation kernel (aug.hip
// aug_blur_kernel): the automatic kernel size, the validity rule and the LDS bytes of the
// streamed separable blur. Plain C++ (no HIP, no torch) so the binding layer, the launcher
// and the stand-alone sanitizer check (csrc/tools/blur_plan_check.cpp) share one copy;
// data/augment.py blur_plan() mirrors it for AugConfig's ValueError.
//
// The kernel streams a view through LDS top to bottom, `rows` rows per barrier round, in
// column strips of `strip` output columns (one strip = the whole width whenever that fits):
//   stage  rows x 3 planes x stage_w   pre-blur rows of the strip plus its horizontal halo
//   ring   (k + rows - 1) x 3 planes x strip   horizontally blurred rows: the k rows under the
//          oldest output row of a round up to the newest row just produced
#pragma once
#include <stdint.h>

namespace sdx_blur {

constexpr int64_t kLdsPerCu = 160 * 1024;   // MI355X LDS per CU = the most one workgroup may hold
constexpr int64_t kLdsDefault = 64 * 1024;  // dynamic LDS a kernel may ask for without raising its limit
constexpr int64_t kStaticLds = 256;         // reserve for the kernel's static __shared__ (view params, reduction)
constexpr int kMaxRows = 16;                // rows per barrier round
constexpr int kMinStrip = 64;               // narrowest strip of a view wider than this

struct Plan {
  int k, r;             // taps, radius
  int rows;             // pre-blur rows produced per barrier round
  int ring_rows;        // k + rows - 1
  int strip;            // output columns per strip (<= S)
  int n_strips;
  int stage_w;          // floats per staging plane: min(S, strip + 2r)
  int w_floats;         // weight table w[0..r], padded to 16 B
  int64_t lds_bytes;    // dynamic LDS: weights + stage + ring
};

// SimCLR recipe: 10 % of the image side, made odd, at least 3
inline int auto_kernel(int64_t S) {
  const int64_t k = (S / 10) | 1;
  return (int)(k < 3 ? 3 : k);
}

inline int64_t stage_width(int64_t S, int64_t k, int64_t strip) {
  const int64_t w = strip + (k - 1);
  return w < S ? w : S;
}

inline int64_t weight_floats(int64_t k) { return (((k - 1) / 2 + 1) + 3) / 4 * 4; }

inline int64_t lds_bytes(int64_t S, int64_t k, int64_t rows, int64_t strip) {
  return 4 * (weight_floats(k) + 3 * (rows * stage_width(S, k, strip) + (k + rows - 1) * strip));
}

// k_req: 0 = automatic. rows_req: 0 = automatic: whole-width strips with the most rows of
// 4, 2, 1 that still lets two workgroups share a CU, else the most that fits one; when not
// even one row fits, one row per round over the fewest equal strips that fit.
// Returns false when the request cannot be served: k even or < 3, radius beyond S - 1
// (reflection undefined), or no strip of at least min(S, kMinStrip) columns fits the LDS.
inline bool make_plan(int64_t S, int64_t k_req, int64_t rows_req, Plan* out) {
  if (S < 1 || S > (1 << 15) || k_req < 0 || k_req > (1 << 15) || rows_req < 0 || rows_req > kMaxRows) return false;
  const int64_t k = k_req > 0 ? k_req : auto_kernel(S);
  if (k < 3 || (k & 1) == 0) return false;
  const int64_t r = (k - 1) / 2;
  if (r > S - 1) return false;
  const int64_t budget = kLdsPerCu - kStaticLds;
  int64_t rows = rows_req;
  if (rows == 0) {
    for (int64_t c : {4, 2, 1})
      if (rows == 0 && lds_bytes(S, k, c, S) <= kLdsPerCu / 2 - kStaticLds) rows = c;
    for (int64_t c : {4, 2, 1})
      if (rows == 0 && lds_bytes(S, k, c, S) <= budget) rows = c;
    if (rows == 0) rows = 1;
  }
  int64_t n_strips = 1, strip = S;
  while (lds_bytes(S, k, rows, strip) > budget) {
    ++n_strips;
    strip = (S + n_strips - 1) / n_strips;
    if (strip < (S < kMinStrip ? S : kMinStrip)) return false;
  }
  n_strips = (S + strip - 1) / strip;
  out->k = (int)k;
  out->r = (int)r;
  out->rows = (int)rows;
  out->ring_rows = (int)(k + rows - 1);
  out->strip = (int)strip;
  out->n_strips = (int)n_strips;
  out->stage_w = (int)stage_width(S, k, strip);
  out->w_floats = (int)weight_floats(k);
  out->lds_bytes = lds_bytes(S, k, rows, strip);
  return true;
}

// reflect padding without repeating the edge: -j -> j, n-1+j -> n-1-j (|overshoot| <= n-1)
inline int64_t reflect(int64_t i, int64_t n) {
  if (i < 0) i = -i;
  if (i > n - 1) i = 2 * (n - 1) - i;
  return i;
}

}  // namespace sdx_blur
