// Soft-target cross-entropy of one logits row (Mixup / CutMix / label smoothing), shared by the
// SOFT forms of linear_ce_fwd (linear_ce.hip, logits in LDS) and ce_rows (head_gemm.hip, logits
// in global memory). One wave per row.
//
// The target of a row with labels a and b is t_c = wa·[c = a] + wb·[c = b] + u with
//   wa = (1 − ε)·λ,  wb = (1 − ε)·(1 − λ),  u = ε / C      (SoftTarget, made once on the host side
//                                                           of the launch, in fp32)
//   loss = lse − ((wa·z_a + wb·z_b) + u·Σ_c z_c),  dz = (softmax − t)·gscale,
// top-1 / top-5 hits against label a with the plain kernels' rank rule #{z_c > z_a} < k. A row with
// either label outside [0, C): loss NaN, no hit, dz = softmax·gscale (the plain convention).
//
// The max, the exponent sum, lse and the softmax are the plain kernels' expressions in the plain
// kernels' order, so b = a, λ = 1, ε = 0 reproduces them bit for bit: wa = 1, wb = 0, u = 0, hence
// t is exactly the one-hot vector, wa·z_a + wb·z_b = z_a + 0 = z_a, and Σ_c z_c is not even formed
// (u = 0), so no overflow of that sum can reach the loss.
#pragma once
#include "common.h"

namespace sdx {

struct SoftTarget {
  float wa, wb, u;
};

inline SoftTarget make_soft_target(float lam, float eps, int C) {
  const float keep = 1.f - eps;
  return SoftTarget{keep * lam, keep * (1.f - lam), eps / (float)C};
}

// z: the row's C logits; a, b: its labels, valid (both in [0, C)) when ok; dz / logits_out: the
// row's destinations, either may be nullptr; rowstat: the row's 3 values
__device__ __forceinline__ void soft_ce_row(const float* z, int C, int a, int b, bool ok, const SoftTarget t,
                                            float gscale, float* __restrict__ logits_out, float* __restrict__ dz,
                                            float* __restrict__ rowstat, int lane) {
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, z[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += __expf(z[c] - m);
  s = wave_sum(s);
  const float lse = m + __logf(s);
  const float za = ok ? z[a] : 0.f;
  const float zb = ok ? z[b] : 0.f;
  const float wa = ok ? t.wa : 0.f, wb = ok ? t.wb : 0.f, u = ok ? t.u : 0.f;
  float above = 0.f, sz = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = z[c];
    if (logits_out != nullptr) logits_out[c] = v;
    above += v > za ? 1.f : 0.f;
    sz += v;
    const float tc = ((c == a ? wa : 0.f) + (c == b ? wb : 0.f)) + u;
    if (dz != nullptr) dz[c] = (__expf(v - lse) - tc) * gscale;
  }
  above = wave_sum(above);
  float tgt = wa * za + wb * zb;
  if (u != 0.f) tgt += u * wave_sum(sz);   // (wave-uniform)
  if (lane == 0) {
    rowstat[0] = ok ? lse - tgt : NAN;
    rowstat[1] = (ok && above < 1.f) ? 1.f : 0.f;
    rowstat[2] = (ok && above < 5.f) ? 1.f : 0.f;
  }
}

}  // namespace sdx
