// Knowledge-distillation loss of one logits row (supervised trainer: --distill_ckpt), shared by the
// DISTILL forms of linear_ce_fwd (linear_ce.hip, logits in LDS) and ce_rows (head_gemm.hip, logits
// in global memory). One wave per row. The teacher's logits row v is read from global memory in
// both (three passes over a row that sits in L2): no LDS beyond what the soft forms use.
//
// With p = softmax(z), q_s = softmax(z·it), q_t = softmax(v·it), it = fp32(1/τ) and the soft target
// t of soft_ce.h (labels a, b; wa, wb, u):
//   ce   = lse(z) − ((wa·z_a + wb·z_b) + u·Σ_c z_c)                    (soft_ce_row's expression and order)
//   kd   = τ²·KL(q_t ‖ q_s) = τ²·((Σ_c q_t,c·((v_c − z_c)·it) − lse(v·it)) + lse(z·it))
//   loss = (1 − α)·ce + α·kd
//   dz_c = ((1 − α)·(p_c − t_c) + (α·τ)·(q_s,c − q_t,c))·gscale
// top-1 / top-5 hits of z against label a by the plain kernels' rank rule #{z_c > z_a} < k.
//
// Conventions:
//   α = 0   reproduces soft_ce_row bit for bit for finite v: the ce part is that routine's
//           expressions in its order and enters as 1·x + 0·y (fused or not, that is x).
//   α = 1   forms no ce term at all — neither lse(z), p nor the target — the way u = 0 skips Σz in
//           soft_ce_row. A row whose label lies outside [0, C) is then valid: its loss is kd and it
//           scores no hit (an unlabelled image).
//   α < 1   keeps the plain rule for such a row: loss NaN, no hit, dz without the target term.
//   τ = 1   takes no shortcut: z·1 = z exactly, so q_s comes out bit-equal to p by the same operations.
// The scaled logits are rounded products (__fmul_rn: never fused into the subtraction that
// follows), so max_c fl(z_c·it) = fl(max_c z_c·it) — rounding is monotone and it > 0 — and the two
// scaled maxima cost no reduction of their own. A teacher row equal to the student row gives
// kd = 0 exactly: every term v_c − z_c is 0 and the two scaled lse are the same operations.
#pragma once
#include "common.h"
#include "soft_ce.h"

namespace sdx {

struct DistillArgs {
  float it, tau, alpha;   // it = 1.f / tau, made on the host side of the launch
};

// τ and 1/τ finite and > 0, 0 <= α <= 1 (a NaN fails every comparison)
inline bool distill_args_ok(float tau, float alpha) {
  const float fmax = 3.402823466e38f;
  return tau > 0.f && tau <= fmax && 1.f / tau <= fmax && alpha >= 0.f && alpha <= 1.f;
}

inline DistillArgs make_distill_args(float tau, float alpha) { return DistillArgs{1.f / tau, tau, alpha}; }

// z: the student's C logits; v: the teacher's (global memory); a, b: the labels, valid (both in
// [0, C)) when ok; dz / logits_out: the row's destinations, either may be nullptr; rowstat: the
// row's 3 values
__device__ __forceinline__ void distill_ce_row(const float* z, const float* __restrict__ v, int C, int a, int b,
                                               bool ok, const SoftTarget t, const DistillArgs d, float gscale,
                                               float* __restrict__ logits_out, float* __restrict__ dz,
                                               float* __restrict__ rowstat, int lane) {
  SDX_DCHECK(!ok || (a >= 0 && a < C && b >= 0 && b < C));
  const bool hard = d.alpha != 1.f;   // (wave-uniform) α = 1: no ce term
  const float it = d.it;
  float m = -INFINITY, mv = -INFINITY;
  for (int c = lane; c < C; c += 64) {
    m = fmaxf(m, z[c]);
    mv = fmaxf(mv, v[c]);
  }
  m = wave_max(m);
  mv = wave_max(mv);
  const float ms = __fmul_rn(m, it), mt = __fmul_rn(mv, it);
  float s = 0.f, ss = 0.f, st = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float zc = z[c];
    if (hard) s += __expf(zc - m);
    ss += __expf(__fmul_rn(zc, it) - ms);
    st += __expf(__fmul_rn(v[c], it) - mt);
  }
  const float lses = ms + __logf(wave_sum(ss));
  const float lset = mt + __logf(wave_sum(st));
  float lse = 0.f;
  if (hard) {
    s = wave_sum(s);
    lse = m + __logf(s);
  }
  const float za = ok ? z[a] : 0.f;
  const float zb = ok ? z[b] : 0.f;
  const float wa = ok ? t.wa : 0.f, wb = ok ? t.wb : 0.f, u = ok ? t.u : 0.f;
  const float ca = 1.f - d.alpha, ck = d.alpha * d.tau;
  float above = 0.f, sz = 0.f, kl = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float zc = z[c], vc = v[c];
    if (logits_out != nullptr) logits_out[c] = zc;
    above += zc > za ? 1.f : 0.f;
    sz += zc;
    const float qs = __expf(__fmul_rn(zc, it) - lses);
    const float qt = __expf(__fmul_rn(vc, it) - lset);
    kl += qt * ((vc - zc) * it);
    float g = ck * (qs - qt);
    if (hard) {
      const float tc = ((c == a ? wa : 0.f) + (c == b ? wb : 0.f)) + u;
      g = ca * (__expf(zc - lse) - tc) + g;
    }
    if (dz != nullptr) dz[c] = g * gscale;
  }
  above = wave_sum(above);
  kl = wave_sum(kl);
  const float kd = (d.tau * d.tau) * ((kl - lset) + lses);
  float loss = d.alpha * kd;
  if (hard) {
    float tgt = wa * za + wb * zb;
    if (u != 0.f) tgt += u * wave_sum(sz);   // (wave-uniform)
    loss = ca * (lse - tgt) + loss;
  }
  if (lane == 0) {
    rowstat[0] = (ok || !hard) ? loss : NAN;
    rowstat[1] = (ok && above < 1.f) ? 1.f : 0.f;
    rowstat[2] = (ok && above < 5.f) ? 1.f : 0.f;
  }
}

}  // namespace sdx
