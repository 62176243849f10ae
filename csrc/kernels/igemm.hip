// Implicit-GEMM convolution on gfx950 MFMA (bf16 in, fp32 accumulate), NHWC.
//
// One kernel template implements the three convolution GEMMs of training
// (reference model: networks/resnet_big.py:38-118, every nn.Conv2d of the encoder):
//
//   FWD   y[m=(n,p,q)][co]    = Σ_{k=(r,s,ci)} x[n][p·st−pad+r][q·st−pad+s][ci] · W[co][r][s][ci]
//   DGRAD dx[m=(n,h,w)][ci]   = Σ_{k=(r,s,co)} dy[n][(h+pad−r)/st][(w+pad−s)/st][co] · Wt[ci][r][s][co]
//   WGRAD dW[co][j=(r,s,ci)]  = Σ_{kk=(n,p,q)} dy[kk][co] · x[n][p·st−pad+r][q·st−pad+s][ci]   (split-K)
//
// Strided DGRAD is decomposed into st² sub-pixel classes (h ≡ ph, w ≡ pw mod st): within
// a class only the taps r ≡ ph+pad (mod st) contribute and (h+pad−r)/st is exact, so every
// MFMA does useful work (a plain masked gather wastes 3/4 of it at stride 2).
//
// Tiles: BM x BN output per 256-thread workgroup (4 waves, each a 64x64 sub-tile of 4x4
// v_mfma_f32_16x16x32_bf16 accumulators), BK = 64. Operands are register-staged (16-byte
// global loads, im2col gather + zero padding in 32-bit address math, k decoded
// incrementally) into a double-buffered LDS image: the next K-tile's loads are issued
// before the current tile's MFMAs and written to the other buffer after them (one barrier
// per K-tile). "K-inner" images ([rows][64] bf16, XOR-swizzled 128-B rows) are read with
// ds_read_b128; "K-outer" images ([64][cols], WGRAD, both operands strided along K) with
// ds_read_b64_tr_b16 transposed reads.
//
// The MFMA is issued as D = Bᵀ·Aᵀ, so each lane's accumulator holds FOUR CONSECUTIVE OUTPUT
// COLUMNS of one output row: the epilogues write 8-byte (bf16) / 16-byte (fp32) pieces.
// FWD/DGRAD store bf16 through an LDS-staged tile as whole 16-B row chunks (optionally to
// remapped rows: DGRAD sub-pixel classes); FWD also emits per-channel BatchNorm statistics
// (per-M-tile Σy, Σy² of the stored values → one slab row, reduced in fp64 by
// bn_stats_reduce). WGRAD writes an fp32 partial slab per K-split (deterministic; reduced
// by splitk.hip), never atomics. Block→tile order is XCD-aware.
//
// This unit holds the four public launchers and instantiates no kernel: the kernel template
// and its dispatch are igemm_kernel.h, compiled by igemm_fwd.hip, igemm_dgrad.hip and
// igemm_wgrad.hip (one per GEMM family) and igemm_tap.hip (the tap-reuse configs of FWD and
// DGRAD); the split-K reduction is splitk.hip.
#include "igemm_kernel.h"

namespace {
// the unit of the last launch with SDX_IGEMM_TRACE on: its g_igemm_trace holds the timeline
enum { UNIT_NONE = -1, UNIT_FWD = MODE_FWD, UNIT_DGRAD = MODE_DGRAD, UNIT_WGRAD = MODE_WGRAD, UNIT_TAP };
int g_trace_unit = UNIT_NONE;

hipError_t launch_unit(int mode, const IgemmParams& p, int cfg, hipStream_t s) {
  const int unit = sdx_plan::is_tap_cfg(cfg) ? UNIT_TAP : mode;
  if (igemm_trace_on()) g_trace_unit = unit;
  switch (unit) {
    case UNIT_FWD: return igemm_launch_fwd(&p, cfg, s);
    case UNIT_DGRAD: return igemm_launch_dgrad(&p, cfg, s);
    case UNIT_WGRAD: return igemm_launch_wgrad(&p, cfg, s);
    default: return igemm_launch_tap(mode, &p, cfg, s);
  }
}

void set_epi(IgemmParams& p, const GemmEpi* epi) {
  if (epi == nullptr) return;
  p.bias = epi->bias;
  p.relu = epi->relu;
  p.out_f32 = epi->out_f32;
  p.add_pre = epi->add_pre;
  p.bn_sc = epi->bn_scale;
  p.bn_sh = epi->bn_shift;
  p.bn_rsc = epi->resid_scale;
  p.a2 = reinterpret_cast<const uint16_t*>(epi->cat_a);
  p.a2_ch = epi->cat_ch;
  p.bias_pre = epi->bias_pre;
  p.bn_rsh = epi->resid_shift;
  p.mask_out = epi->mask_out;
  if (epi->resid != nullptr) p.addend = reinterpret_cast<const uint16_t*>(epi->resid);
}
}  // namespace

hipError_t launch_conv_fwd(const ConvGeom& g, const void* x, const void* w, void* y, float* stats, int cfg,
                           hipStream_t s, const float* in_scale, const float* in_shift, const GemmEpi* epi) {
  IgemmParams p{};
  set_epi(p, epi);
  if (p.out_f32 && stats != nullptr) return hipErrorInvalidValue;
  // BN-apply epilogue: stride-1 1x1 geometry (the residual shares the output rows), no
  // statistics / fp32 output / bias; statistics-only pass: y == nullptr needs stats
  if (p.bn_sc != nullptr &&
      (p.bn_sh == nullptr || p.addend == nullptr || (p.bn_rsc == nullptr) != (p.bn_rsh == nullptr) ||
       stats != nullptr || p.out_f32 || p.bias != nullptr || p.relu || in_scale != nullptr || y == nullptr || g.R != 1 || g.S != 1 || g.stride != 1 || g.pad != 0))
    return hipErrorInvalidValue;
  if (y == nullptr && (stats == nullptr || p.bn_sc != nullptr)) return hipErrorInvalidValue;
  p.in_scale = in_scale;
  p.in_shift = in_shift;
  p.g = g;
  p.a = (const uint16_t*)x;
  p.b = (const uint16_t*)w;
  p.out = y;
  p.stats = stats;
  p.M = g.N * g.P * g.Q;
  p.Ncol = g.K;
  p.Kdim = g.R * g.S * g.C;
  p.b_row = p.Kdim;
  p.b_t0 = 0;
  p.b_tr = g.S * g.C;
  p.b_ts = g.C;
  p.a_elems = (long)g.N * g.H * g.W * g.C;
  p.b_elems = (long)p.Ncol * p.Kdim;
  return launch_unit(MODE_FWD, p, cfg, s);
}

hipError_t launch_conv_dgrad_class(const ConvGeom& g, int ph, int pw, const void* dy, const void* wt, void* dx,
                                   const void* addend, int cfg, hipStream_t s, const void* addend_mask,
                                   const BnBwdStat* bstat, int addend_sub, const GemmEpi* epi) {
  IgemmParams p{};
  set_epi(p, epi);
  if (p.out_f32 && (g.stride != 1 || addend != nullptr || (bstat != nullptr && bstat->slab != nullptr)))
    return hipErrorInvalidValue;
  p.addend_sub = addend_sub;
  if (bstat != nullptr) p.bs = *bstat;
  p.addend_mask = (const uint8_t*)addend_mask;
  p.g = g;
  p.a = (const uint16_t*)dy;
  p.b = (const uint16_t*)wt;   // the full Wt [C][R][S][K]; the class's taps are strided into it
  p.out = dx;
  p.addend = (const uint16_t*)addend;
  p.ph = ph;
  p.pw = pw;
  const sdx_plan::DgradClass c = sdx_plan::dgrad_class(g, ph, pw);
  p.r0 = c.r0; p.nr = c.nr; p.s0 = c.s0; p.ns = c.ns; p.Hc = c.Hc; p.Wc = c.Wc;
  p.M = c.M;
  if (p.M == 0) return hipSuccess;
  p.Ncol = g.C;
  p.Kdim = p.nr * p.ns * g.K;
  p.b_row = g.R * g.S * g.K;
  if (p.a2 != nullptr || p.a2_ch != 0) {
    if (p.a2 == nullptr || !sdx_plan::dgrad_cat_supported(g, p.a2_ch, sdx_plan::knobs())) return hipErrorInvalidValue;
    p.a2_sh = __builtin_ctz((unsigned)(g.K / p.a2_ch));
    p.a2_elems = (long)g.N * g.P * g.Q * p.a2_ch;
    p.Kdim += p.a2_ch;
    p.b_row += p.a2_ch;
  }
  if (p.bias_pre != nullptr && (g.stride != 1 || (reinterpret_cast<uintptr_t>(p.bias_pre) & 15) != 0))
    return hipErrorInvalidValue;
  p.b_t0 = (p.r0 * g.S + p.s0) * g.K;
  p.b_tr = g.stride * g.S * g.K;
  p.b_ts = g.stride * g.K;
  p.a_elems = (long)g.N * g.P * g.Q * g.K;
  p.b_elems = (long)p.Ncol * p.b_row;
  return launch_unit(MODE_DGRAD, p, cfg, s);
}

hipError_t launch_conv_dgrad_merged(const ConvGeom& g, const sdx_plan::DgradPlan& plan, const void* dy, const void* wt,
                                    void* dx, const void* addend, hipStream_t s, const void* addend_mask,
                                    const BnBwdStat* bstat, int addend_sub) {
  const int st = g.stride;
  if (!plan.merged || !plan.ok || st != 2) return hipErrorInvalidValue;
  if (plan.ncls == 0) return hipSuccess;
  IgemmParams p{};
  p.addend_sub = addend_sub;
  if (bstat != nullptr) p.bs = *bstat;
  p.addend_mask = (const uint8_t*)addend_mask;
  p.g = g;
  p.a = (const uint16_t*)dy;
  p.b = (const uint16_t*)wt;
  p.out = dx;
  p.addend = (const uint16_t*)addend;
  p.Ncol = g.C;
  p.b_row = g.R * g.S * g.K;
  p.b_tr = st * g.S * g.K;
  p.b_ts = st * g.K;
  p.a_elems = (long)g.N * g.P * g.Q * g.K;
  p.b_elems = (long)p.Ncol * p.b_row;
  // the plan's classes: those with more taps first (longest blocks dispatched first)
  for (int i = 0; i < plan.ncls; ++i) {
    const sdx_plan::DgradClass& c = plan.cls[i];
    IgemmParams::Cls& cd = p.cls[i];
    cd.ph = c.ph; cd.pw = c.pw; cd.Hc = c.Hc; cd.Wc = c.Wc;
    cd.r0 = c.r0; cd.nr = c.nr; cd.s0 = c.s0; cd.ns = c.ns;
    cd.M = c.M;
    cd.Kdim = c.nr * c.ns * g.K;
    cd.b_t0 = (c.r0 * g.S + c.s0) * g.K;
  }
  p.ncls = plan.ncls;
  // launch-level choices (main loop, single-stage form) see the largest class; the per-class
  // fields below are the first class's (every block overwrites them with its own)
  const IgemmParams::Cls& c0 = p.cls[0];
  p.ph = c0.ph; p.pw = c0.pw; p.Hc = c0.Hc; p.Wc = c0.Wc; p.r0 = c0.r0; p.s0 = c0.s0;
  p.nr = c0.nr; p.ns = c0.ns; p.b_t0 = c0.b_t0;
  p.M = plan.max_M;
  p.Kdim = plan.max_Kdim;
  return launch_unit(MODE_DGRAD, p, plan.cfg, s);
}

hipError_t launch_conv_wgrad(const ConvGeom& g, const sdx_plan::WgradPlan& plan, const void* dy, const void* x,
                             float* partial, float* dw, int accumulate, hipStream_t s, const float* in_scale,
                             const float* in_shift) {
  if (!plan.ok || plan.family != sdx_plan::WGRAD_GENERIC) return hipErrorInvalidValue;
  IgemmParams p{};
  p.in_scale = in_scale;
  p.in_shift = in_shift;
  p.g = g;
  p.a = (const uint16_t*)dy;
  p.b = (const uint16_t*)x;
  p.M = g.K;
  p.Ncol = g.R * g.S * g.C;
  p.Kdim = g.N * g.P * g.Q;
  p.a_elems = (long)g.N * g.P * g.Q * g.K;
  p.b_elems = (long)g.N * g.H * g.W * g.C;
  p.k_per_split = plan.per;
  p.splits = plan.splits;
  p.div_pq = make_fastdiv((unsigned)(g.P * g.Q));
  p.div_q = make_fastdiv((unsigned)g.Q);
  auto log2_exact = [](int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return (1 << l) == v ? l : -1;
  };
  // WGRAD block order: 1 split-major (default), 0 tile-major
  static const int worder = (int)sdx_plan::env_int("SDX_WGRAD_ORDER", 1);
  p.worder = worder;
  p.lq = log2_exact(g.Q);
  p.lpq = log2_exact(g.P * g.Q);
  if (p.lq < 0 || p.lpq < 0) p.lq = p.lpq = -1;
  // a single split writes straight into dW (unless accumulating)
  const bool direct = plan.direct && !accumulate;
  if (!direct && partial == nullptr) return hipErrorInvalidValue;
  p.out = direct ? (void*)dw : (void*)partial;
  hipError_t e = launch_unit(MODE_WGRAD, p, plan.cfg, s);
  if (e != hipSuccess || direct) return e;
  return launch_splitk_reduce(partial, p.splits, (long)p.M * p.Ncol / 4, dw, accumulate, s);
}

// the diagnostic timeline of the last traced launch (SDX_IGEMM_TRACE=1): 2 x kTraceSlots u64
int igemm_trace_slots() { return kTraceSlots; }
hipError_t igemm_trace_copy(unsigned long long* host, hipStream_t s) {
  hipError_t e = hipStreamSynchronize(s);
  if (e != hipSuccess) return e;
  switch (g_trace_unit) {
    case UNIT_FWD: return igemm_trace_copy_fwd(host);
    case UNIT_DGRAD: return igemm_trace_copy_dgrad(host);
    case UNIT_WGRAD: return igemm_trace_copy_wgrad(host);
    case UNIT_TAP: return igemm_trace_copy_tap(host);
    default:   // nothing traced yet: the buffers are still zero
      memset(host, 0, sizeof(unsigned long long) * 2 * kTraceSlots);
      return hipSuccess;
  }
}
