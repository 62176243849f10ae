// Planning arithmetic of the BatchNorm projector head kernels (csrc/kernels/head_bn.hip): the
// supported range, the forward kernel's strip width and row fragments per wave, the backward
// kernel's rows per thread. Plain C++ (no HIP, no torch), shared by the launchers, the binding
// layer and the kernels' template dispatch.
//
// Forward (hbn_fwd): one workgroup of kWaves waves owns ALL rows of a strip of 16 or 32 output
// columns. Row fragment f (16 rows) belongs to wave f % kWaves, so a wave holds `frags` fragments
// = frags x (strip / 16) x 4 fp32 accumulators per lane, next to two k-steps of its rows' x
// operands (2 x frags x 4 registers). The widest plan, N = 2048, is frags = 16 on 16-wide strips:
// 64 accumulators + 128 operand registers, inside the 256 registers a lane has at 2 waves per
// SIMD. A 32-wide strip is taken only where it still gives every CU a strip (H / 32 >= kCUs) and
// frags <= 8.
#pragma once
#include <stdint.h>

namespace sdx_hbn {

constexpr int kWaves = 8;            // waves per workgroup, both kernels
constexpr int kThreads = kWaves * 64;
constexpr int kChunk = 64;           // reduction elements of W staged per barrier (two MFMA k-steps)
constexpr int kMinRows = 2;          // the unbiased running variance divides by N - 1
constexpr int kMaxRows = 2048;
constexpr int kMaxK = 8192;
constexpr int kMaxH = 8192;
constexpr int kCUs = 256;            // MI355X
constexpr int kBwdStrip = 16;        // hbn_bwd: columns per workgroup (two 16-byte lanes per row)
constexpr int kBwdRowsPass = kThreads / 2;   // rows one pass of the backward workgroup covers

inline bool supported(int64_t n, int64_t k, int64_t h) {
  return n >= kMinRows && n <= kMaxRows && k >= kChunk && k <= kMaxK && k % kChunk == 0 && h >= 32 && h <= kMaxH &&
         h % 32 == 0;
}

struct FwdPlan {
  int strip;    // 16 | 32 output columns per workgroup
  int frags;    // 16-row fragments per wave: 1, 2, 4, 8 or 16
  int strips;   // grid size
  int acc_regs, x_regs;   // per lane: fp32 accumulators, prefetched x operand registers
  int lds_bytes;
};

// strip: 0 = the plan's choice; 16 or 32 forces a width (refused where it cannot run)
inline bool make_fwd(int64_t n, int64_t k, int64_t h, int strip, FwdPlan* p) {
  if (!supported(n, k, h)) return false;
  const int need = (int)((n + 16 * kWaves - 1) / (16 * kWaves));   // fragments of the busiest wave
  int frags = 1;
  while (frags < need) frags *= 2;
  if (strip == 0) strip = (frags <= 8 && h / 32 >= kCUs) ? 32 : 16;
  if ((strip != 16 && strip != 32) || (strip == 32 && frags > 8)) return false;
  p->strip = strip;
  p->frags = frags;
  p->strips = (int)(h / strip);
  p->acc_regs = frags * (strip / 16) * 4;
  p->x_regs = 2 * frags * 4;
  p->lds_bytes = 2 * strip * kChunk * 2 + kWaves * strip * 4 + 2 * strip * 4;
  return true;
}

struct BwdPlan {
  int rows_per_thread;   // 1, 2, 4 or 8: 16 packed registers each (da and yb)
  int strips;
};

inline bool make_bwd(int64_t n, int64_t h, BwdPlan* p) {
  if (n < kMinRows || n > kMaxRows || h < 32 || h > kMaxH || h % 32 != 0) return false;
  const int need = (int)((n + kBwdRowsPass - 1) / kBwdRowsPass);
  int r = 1;
  while (r < need) r *= 2;
  p->rows_per_thread = r;
  p->strips = (int)(h / kBwdStrip);
  return true;
}

}  // namespace sdx_hbn
