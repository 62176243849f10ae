// Host-side dispatch planning of the convolution kernels (igemm.hip / igemm_kernel.h, wgrad1x1.hip,
// wgrad3x3.hip): which tile config, main loop and kernel variant a conv pass runs, its split
// counts, statistics-slab rows and workspace sizes, and every run-time switch that moves
// them. Plain C++ (no HIP, no torch), header-only like knn_plan.h: the kernel translation
// units, the binding layer and the stand-alone sanitizer check
// (csrc/tools/conv_plan_check.cpp) share this one copy, and a plan is a pure function of
// (geometry, request, Knobs). tests/golden/conv_plan.json pins it per shape and knob setting.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

struct ConvGeom {
  int N, H, W, C;   // input NHWC
  int K;            // output channels
  int R, S;         // filter
  int P, Q;         // output spatial
  int stride, pad;
};

namespace sdx_plan {

// ---- environment ------------------------------------------------------------------------
// the one place the extension reads its environment
inline const char* env_str(const char* name) { return getenv(name); }
inline long long env_int(const char* name, long long dflt) {
  const char* e = env_str(name);
  return e ? atoll(e) : dflt;
}
inline bool env_flag(const char* name, bool dflt) {   // unset: dflt; else "non-zero"
  const char* e = env_str(name);
  return e ? atoi(e) != 0 : dflt;
}

// Every run-time switch of the conv dispatch, read once from the environment (docs/KNOBS.md).
// The run-time setters (tap3_set, wgrad_block_target_set, wgrad1x1_pairs_set,
// wgrad1x1_big_set, igemm_one_k_set) write the process's copy between steps.
struct Knobs {
  int conv_cfg = -1;          // SDX_CONV_CFG 0..8: pinned fwd/dgrad tile config (-1: auto)
  int tap3 = 1;               // SDX_TAP3: tap-reuse 3x3 loop in auto dispatch
  int cfg_rules = 4;          // SDX_CFG_RULES: bit mask of the conv_cfg corrections
  bool conv_d6 = true;        // SDX_CONV_D6: cfg 6 for long-K, 256-multiple outputs
  int dgrad_merge = 2;        // SDX_DGRAD_MERGE: 0 per class, 1 merged, 2 merged for 3x3 only
  long long w3_blocks = 128;  // SDX_W3_BLOCKS: block target of the dedicated wgrad kernels
  bool wgrad3 = true;         // SDX_WGRAD3: tap-reuse 3x3 wgrad kernel in auto dispatch
  bool wgrad1 = true;         // SDX_WGRAD1: 1x1 wgrad kernel in auto dispatch
  bool wgrad_wide64 = true;   // SDX_WGRAD_WIDE64: 64x256 tile for 64-row generic wgrads
  long long w3_tail_pix = 0;        // SDX_W3_TAIL_PIX (0: off)
  long long w3_tail_blocks = 256;   // SDX_W3_TAIL_BLOCKS
  long long w1_pair_blocks = 256;   // SDX_W1_PAIR_BLOCKS
  long long wgrad_target = 512;     // SDX_WGRAD_TARGET: block target of the generic wgrad
  bool tap_pad = true;        // SDX_TAP_PAD: padded-row tap tiles
  int igemm_glds = 1;         // SDX_IGEMM_GLDS: LDS-DMA staging 0 off, 1 FWD/DGRAD, 2 + WGRAD
  int igemm_depth = 2;        // SDX_IGEMM_DEPTH=1|2: register-prefetch depth of the K loop
  int igemm_one = 1;          // SDX_IGEMM_ONE: single-stage form of the DEPTH 3 loop
  int one_k[2] = {256, 64};   // SDX_IGEMM_ONE_K / _DGRAD: longest reduction on that form
  int w1_pairs = 0;           // SDX_W1_PAIRS: pixel-pair view of 64-channel 1x1 wgrads
  int w1_big = 1;             // SDX_W1_BIG: 256-row 1x1 wgrad 0 off, 1 by the rule, 2 always
  long w1_big_min = 8192;     // SDX_W1_BIG_MIN
  int w1_bn = 0;              // SDX_W1_BN=128: force the 128-column 1x1 wgrad tile
  bool w1_pipe = true;        // SDX_W1_PIPE
  bool w1_strided = true;     // SDX_W1_STRIDED
  bool w3_pad = true;         // SDX_W3_PAD
  bool w3_s2 = true;          // SDX_W3_S2

  static Knobs from_env() {
    Knobs k;
    const int pin = (int)env_int("SDX_CONV_CFG", -1);
    k.conv_cfg = pin >= 0 && pin <= 8 ? pin : -1;
    k.tap3 = (int)env_int("SDX_TAP3", 1);
    k.cfg_rules = (int)env_int("SDX_CFG_RULES", 4);
    k.conv_d6 = env_flag("SDX_CONV_D6", true);
    k.dgrad_merge = (int)env_int("SDX_DGRAD_MERGE", 2);
    k.w3_blocks = env_int("SDX_W3_BLOCKS", 128);
    k.wgrad3 = env_flag("SDX_WGRAD3", true);
    k.wgrad1 = env_flag("SDX_WGRAD1", true);
    k.wgrad_wide64 = env_flag("SDX_WGRAD_WIDE64", true);
    k.w3_tail_pix = env_int("SDX_W3_TAIL_PIX", 0);
    k.w3_tail_blocks = env_int("SDX_W3_TAIL_BLOCKS", 256);
    k.w1_pair_blocks = env_int("SDX_W1_PAIR_BLOCKS", 256);
    k.wgrad_target = env_int("SDX_WGRAD_TARGET", 512);
    k.tap_pad = env_flag("SDX_TAP_PAD", true);
    k.igemm_glds = (int)env_int("SDX_IGEMM_GLDS", 1);
    const char* d = env_str("SDX_IGEMM_DEPTH");
    k.igemm_depth = (d && d[0] == '1') ? 1 : 2;
    k.igemm_one = (int)env_int("SDX_IGEMM_ONE", 1);
    k.one_k[0] = (int)env_int("SDX_IGEMM_ONE_K", 256);
    k.one_k[1] = (int)env_int("SDX_IGEMM_ONE_K_DGRAD", 64);
    k.w1_pairs = env_flag("SDX_W1_PAIRS", false) ? 1 : 0;
    const int big = (int)env_int("SDX_W1_BIG", 1);
    k.w1_big = big < 0 ? 0 : big > 2 ? 2 : big;
    k.w1_big_min = (long)env_int("SDX_W1_BIG_MIN", 8192);
    k.w1_bn = (int)env_int("SDX_W1_BN", 0);
    k.w1_pipe = env_flag("SDX_W1_PIPE", true);
    k.w1_strided = env_flag("SDX_W1_STRIDED", true);
    k.w3_pad = env_flag("SDX_W3_PAD", true);
    k.w3_s2 = env_flag("SDX_W3_S2", true);
    return k;
  }
};

// the process's knobs (setters write through knobs_mut())
inline Knobs& knobs_mut() {
  static Knobs k = Knobs::from_env();
  return k;
}
inline const Knobs& knobs() { return knobs_mut(); }

// ---- tiles ------------------------------------------------------------------------------
constexpr int kBK = 64;   // K-tile of the implicit GEMM
enum { MODE_FWD = 0, MODE_DGRAD = 1, MODE_WGRAD = 2 };

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// tile configs: 0 128x128 (2x2 waves of 64x64), 1 256x64 (4x1), 2 64x256 (1x4), 3 64x64 (2x2 waves of 32x32),
// 4 128x128 with 8 waves (2x4 of 64x32: twice the waves per SIMD for latency hiding),
// 5 256x128 with 8 waves (4x2 of 64x64, one block per CU), 6 128x256 with 8 waves (2x4 of
// 64x64); both run the in-wave pipelined loop (DEPTH 6, 144 KiB LDS ring) at K > 128.
// (7 / 8, 4-wave 64x128 wave tiles, measured slower than 5 / 6 in round 4 and removed.)
// tap-reuse 3x3 (FWD / stride-1 DGRAD only): 11 256x64 with 4 waves of 64x64 and one halo
// buffer (C = 64: two blocks per CU), 12 256x128 with 8 waves (4x2 of 64x64), 13 128x128
// with 8 waves (2x4 of 64x32)
inline int tile_m(int64_t cfg) {
  static const int m[14] = {128, 256, 64, 64, 128, 256, 128, 0, 0, 0, 0, 256, 256, 128};
  return (cfg >= 0 && cfg < 14) ? m[cfg] : 0;
}
inline int tile_n(int64_t cfg) {
  static const int n[14] = {128, 64, 256, 64, 128, 128, 256, 0, 0, 0, 0, 64, 128, 128};
  return (cfg >= 0 && cfg < 14) ? n[cfg] : 0;
}
inline int tile_waves(int64_t cfg) {
  static const int w[14] = {4, 4, 4, 4, 8, 8, 8, 0, 0, 0, 0, 4, 8, 8};
  return (cfg >= 0 && cfg < 14) ? w[cfg] : 0;
}
inline bool is_tap_cfg(int64_t cfg) { return cfg >= 11 && cfg <= 13; }
inline int tap_depth(int64_t cfg) { return cfg == 11 ? 8 : 7; }

// ---- tap-reuse 3x3 loop (DEPTH 7 / 8) ------------------------------------------------------
// DEPTH 7 / 8 halo buffer size in KiB: the largest window a BM-row tile needs over the
// supported image widths (BM = 256: 4 images of 8x8 = 4·10·10 pixels = 50 KiB at 64
// channels; BM = 128: 8 images of 4x4 = 8·6·6 pixels = 36 KiB)
constexpr int tap_halo_kb(int bm) { return bm == 256 ? 50 : 36; }

// what launch_tap copies into the kernel parameters (IgemmParams t_*, igemm_kernel.h)
struct TapGeom {
  int t_rw, t_rs, t_imgs, t_is, t_hp, t_nhp, t_ky, t_nch;
};

// Geometry of the tap-reuse loop (DEPTH 7 / 8) for a BM-row tile; false = not supported:
// a pad-1 3x3 stride-1 conv (DGRAD: the stride-1 class) whose tile rows are whole image
// rows of whole images or of one image band, a channel dim (cdim: FWD C, DGRAD K) of
// 64-channel chunks and a window that fits the halo buffer. Swizzle phase t_ky: fragments of
// 16 output pixels span 1 row (W >= 16), 2 rows (W = 8: ky = 0) or 4 rows (W = 4: ky = 4) —
// conflict-free ds_read_b128 lane groups for every tap (checked by brute force over the lane
// groups of the LDS table in MI355X_MICROARCH.md); other widths are correct, not conflict-free.
// SDX_TAP_PAD=0: no padded-row tiles (widths that do not divide BM stay on the implicit GEMM)
inline bool tap_geom(const ConvGeom& g, int cdim, int bm, int depth, const Knobs& k, TapGeom* t) {
  if (g.R != 3 || g.S != 3 || g.stride != 1 || g.pad != 1 || g.P != g.H || g.Q != g.W) return false;
  const int HW = g.H * g.W;
  if (cdim % 64 != 0) return false;
  t->t_rw = 0;
  int rw = g.W;
  if (bm % g.W != 0 || !(HW % bm == 0 || bm % HW == 0)) {
    // padded rows: a band of bm / rw whole image rows of rw = pow2 >= W virtual pixels each
    // (fragments of 16 virtual pixels stay inside one row: rw >= 16). Single-chunk DEPTH-8
    // tiles only: 56x56x64 fwd / dgrad 376 / 378 us vs 389 / 427 on the best implicit-GEMM
    // tile, but the 128-row DEPTH-7 tile at 28x28x128 runs 446 / 419 vs 258 / 266
    // (profiles/tap_pad_r6.txt, 1024 views)
    rw = 16;
    while (rw < g.W) rw <<= 1;
    if (!k.tap_pad || depth != 8 || bm % rw != 0 || g.H % (bm / rw) != 0) return false;
    t->t_rw = rw;
  }
  t->t_rs = g.W + 2;
  t->t_imgs = (t->t_rw == 0 && bm >= HW) ? bm / HW : 0;
  const int rows = t->t_imgs > 0 ? g.H : bm / rw;
  t->t_is = (rows + 2) * t->t_rs;
  t->t_hp = (t->t_imgs > 0 ? t->t_imgs : 1) * t->t_is;
  t->t_nhp = (t->t_hp + 7) / 8;
  t->t_ky = g.W == 4 ? 4 : 0;
  t->t_nch = cdim / 64;
  if (t->t_nhp > tap_halo_kb(bm)) return false;
  // padded rows: the last row's padded fragments read up to pixel (rows + 1)·t_rs + rw + 1,
  // still inside the halo buffer
  if (t->t_rw > 0 && (rows + 1) * t->t_rs + rw + 2 > tap_halo_kb(bm) * 8) return false;
  if (bm == 256 && t->t_ky != 0) return false;   // the BM = 256 loop keeps 3 address variants
  if (depth == 8 && t->t_nch != 1) return false;
  return true;
}

// tap-reuse tile config (11-13) for a pad-1 stride-1 3x3 conv whose reduction runs over cdim
// channels and whose output has ncol channels (DGRAD: cdim = K, ncol = C), or -1
inline int tap_cfg(const ConvGeom& g, int cdim, int ncol, const Knobs& k) {
  if (g.R != 3 || g.S != 3 || g.stride != 1 || g.pad != 1 || cdim % 64 != 0) return -1;
  const int cands[3] = {cdim == 64 && ncol <= 64 ? 11 : -1, g.W >= 8 ? 12 : -1, 13};
  for (int cfg : cands) {
    TapGeom t;
    if (cfg >= 0 && tap_geom(g, cdim, tile_m(cfg), tap_depth(cfg), k, &t)) return cfg;
  }
  return -1;
}

// M-tiles (statistics-slab rows) of a fwd / dgrad-class launch of M output rows under cfg: a
// padded-row tap tile counts its virtual rows (they tile exactly — H is a multiple of the
// band height)
inline int64_t conv_mtiles(const ConvGeom& g, int cdim, int64_t cfg, int64_t M, const Knobs& k) {
  const int bm = tile_m(cfg);
  if (bm <= 0) return 0;
  TapGeom t;
  if (is_tap_cfg(cfg) && tap_geom(g, cdim, bm, tap_depth(cfg), k, &t) && t.t_rw > 0)
    return (int64_t)g.N * g.H * t.t_rw / bm;
  return cdiv(M, bm);
}

// ---- fwd / dgrad tile config --------------------------------------------------------------
// Pick the tile config (0 128x128, 1 256x64, 2 64x256, 3 64x64) minimising
//   padded work x per-config efficiency penalty x grid fill,
// where fill = (launch rounds x resident slots) / tiles charges a grid that leaves CUs idle
// in its last round (e.g. M=8192 x N=512: 256 tiles of 128x128 fill only half of the 512
// two-per-CU slots). The small 64x64 tile is only penalised when the GEMM is
// compute-bound (long K); short-K (memory-bound) GEMMs favour its higher occupancy.
// Calibrated with tools/conv_bench.py --cfg 0..3 on the ResNet-50 shapes.
// SDX_CONV_CFG=c pins the fwd/dgrad tile config (tests): the BN-statistics epilogue's per-tile
// fp32 partial sums then cover the same rows whatever the per-rank batch, so a W-rank step
// reproduces the single-rank statistics bit for bit (tests/test_gpu_dist.py)
inline int auto_cfg(int64_t M, int64_t Ncol, int64_t Kdim, bool fill, const Knobs& k) {
  if (fill && k.conv_cfg >= 0) return k.conv_cfg;
  const int64_t bm[4] = {128, 256, 64, 64}, bn[4] = {128, 64, 256, 64};
  const bool long_k = Kdim == 0 || Kdim > 256;
  const double pen_long[4] = {1.0, 1.04, 1.04, 1.35}, pen_short[4] = {1.0, 1.0, 1.0, 1.05};
  const double slots[4] = {512, 512, 512, 1280};   // resident blocks chip-wide (LDS/VGPR-limited)
  int best = 0;
  double best_s = 1e300;
  for (int c = 0; c < 4; ++c) {
    const int64_t mt = (M + bm[c] - 1) / bm[c], nt = (Ncol + bn[c] - 1) / bn[c];
    const double padded = (double)(mt * bm[c]) * (double)(nt * bn[c]);
    double f = 1.0;
    if (fill) {
      const double tiles = (double)(mt * nt);
      f = ceil(tiles / slots[c]) * slots[c] / tiles;
    }
    const double sc = padded * (long_k ? pen_long[c] : pen_short[c]) * f;
    if (sc < best_s) { best_s = sc; best = c; }
  }
  // fwd/dgrad: the 8-wave 128x128 tile (cfg 4, 2x4 waves of 64x32) beats the 4-wave one by
  // 3-12% on every ResNet-50 shape with a reduction of >= 128 (more waves hide the LDS-DMA
  // and epilogue latency); on the K=64 layer-1 GEMMs its longer prologue costs more than it
  // hides. wgrad keeps the 4-wave tiles (its split-K slabs are short). profiles/conv_cfg4_r1.txt
  if (fill && best == 0 && Kdim >= 128) best = 4;
  // long-K GEMMs whose output width is a multiple of 256 (layers 3-4): the 8-wave 128x256 tile
  // on the in-wave pipelined LDS-DMA ring (cfg 6, DEPTH 6) — l3 3x3 fwd/dgrad 41.3 -> 38.1 us,
  // l4.0.sc dgrad 67.5 -> 64.8 us; it loses on narrower or short-K GEMMs, where one tile per CU
  // leaves its prologue/epilogue exposed (profiles/conv_core_r4.txt)
  if (fill && k.conv_d6 && Ncol % 256 == 0 && Kdim >= 1024) best = 6;
  return best;
}

// fwd / dgrad tile config of a conv: the tap-reuse 3x3 loop where it applies (pad-1 stride-1
// 3x3; not with a pinned config, the in-kernel statistics reduction or the BN+ReLU operand
// prologue: plain = false), else auto_cfg. SDX_TAP3=0 disables it. Per shape
// (tools/tap3_sweep.py, profiles/tap3_r5.txt) it beats the best implicit-GEMM tile at every
// CIFAR ResNet-50 3x3: fwd / dgrad l1 52 / 51 vs 67 / 68 us, l2 45 / 42 vs 47 / 45,
// l3 34 / 34 vs 38 / 37, l4 38 / 38 vs 58 / 56
//
// Then per-pass corrections to auto_cfg from the round-5 re-calibration (every fwd / dgrad
// of the CIFAR ResNet-50 at 512 views under every tile config, the dgrads with their
// BN-statistics epilogue: tools/cfg_sweep.py, profiles/cfg_sweep_r5.txt; 5.32 -> 5.24 ms
// summed stand-alone). Three corrections won stand-alone; in the step (bench A/B, same box,
// SDX_CFG_RULES bit mask) only bit 4 does, so it alone is on by default:
//  1 the 128x256 DEPTH-6 tile only when it fills the chip (>= 256 tiles): l4 1x1 / strided
//    3x3 fwd at M = 8192 on the 8-wave 128x128 (52.8 vs 58.1 us) — neutral in the step;
//  2 expanding stride-1 dgrads (dx has >= 256 and >= twice the reduction's channels) on the
//    64x256 tile (l1 137.8 vs 146.3 us) — +0.05 ms in the step (12.21 vs 12.155 ms): more
//    blocks per CU under the heavy epilogue is exactly what the side-stream wgrads lose;
//  4 strided dgrads with 256-multiple outputs on DEPTH 6 (l3.0 3x3 84.4 vs 90.4 us, l3.0
//    shortcut 127.3 vs 135.9) — -0.03 ms in the step (12.12 vs 12.155)
inline int conv_cfg(const ConvGeom& g, int cdim, int ncol, int64_t M, int64_t Kdim, bool plain, bool dgrad,
                    const Knobs& k) {
  if (k.tap3 > 0 && plain && k.conv_cfg < 0) {
    const int t = tap_cfg(g, cdim, ncol, k);
    if (t >= 0) return t;
  }
  int cfg = auto_cfg(M, ncol, Kdim, true, k);
  if (k.conv_cfg >= 0) return cfg;
  const int rules = k.cfg_rules;
  if ((rules & 1) && cfg == 6 && cdiv(M, tile_m(6)) * cdiv(ncol, tile_n(6)) < 256) cfg = 4;
  if ((rules & 2) && dgrad && g.stride == 1 && ncol >= 256 && 2 * Kdim <= ncol) cfg = 2;
  if ((rules & 4) && dgrad && g.stride > 1 && ncol % 256 == 0 && Kdim * g.stride * g.stride >= 1024) cfg = 6;
  return cfg;
}

// ---- main loop of a fwd / dgrad launch (the template dispatch stays in igemm_kernel.h) ----------
// K-concatenated dgrad [dy | a2]·[Wd ; Mx] (BN3 fold): a stride-1 unpadded 1x1 whose dy
// width is a power-of-two multiple of a2's (both multiples of BK), on the LDS-DMA loops
inline bool dgrad_cat_supported(const ConvGeom& g, int cat_ch, const Knobs& k) {
  if (cat_ch <= 0 || g.R != 1 || g.S != 1 || g.stride != 1 || g.pad != 0 || g.P != g.H || g.Q != g.W) return false;
  if (g.K % kBK != 0 || cat_ch % kBK != 0 || g.K % cat_ch != 0) return false;
  const unsigned r = (unsigned)(g.K / cat_ch);
  return (r & (r - 1)) == 0 && k.igemm_glds != 0;
}

// Main loop of a tile config 0-6 launch: 3 = LDS-DMA double buffer, 6 = in-wave pipelined
// LDS-DMA ring, 2 / 1 = register-staged with / without a second prefetch stage.
// cdim: reduction channels per tap (FWD C, DGRAD K + concatenated channels); taps: R·S (a
// dgrad class: its nr·ns); prologue: the BN+ReLU operand prologue; bstat: the BN-statistics
// epilogue of a dgrad.
// DEPTH 6: 8-wave 256x128 / 128x256 tiles at more than two K-tiles whose channel dim is a
// multiple of BK (branch-free K decode). Depth 2 only where the second register stage fits
// without spilling (checked with -Rpass-analysis=kernel-resource-usage).
inline int igemm_loop(int mode, int bm, int bn, int waves, int Kdim, int cdim, int taps, bool prologue, bool bstat,
                      const Knobs& k) {
  if (mode == MODE_WGRAD) {   // LDS-DMA (SDX_IGEMM_GLDS=2) not with the prologue
    if (!prologue && k.igemm_glds == 2) return 3;
    return (bm == 64 && bn == 64 && k.igemm_depth == 2) ? 2 : 1;
  }
  if (!prologue && k.igemm_glds != 0) {
    const bool w1 = waves == 8 && bm * bn == 256 * 128 && Kdim > 2 * kBK && cdim % kBK == 0 && taps <= 32;
    return w1 ? 6 : 3;
  }
  const bool depth2 = (bm == 64 && bn == 64) || (mode == MODE_FWD && bm != 256);
  return (depth2 && k.igemm_depth == 2 && !bstat) ? 2 : 1;
}

// The single-stage (ONE) form is DEPTH 3 with a reduction of at most SDX_IGEMM_ONE_K (forward,
// default 256) / SDX_IGEMM_ONE_K_DGRAD (data gradient, default BK = one K-tile, the only case
// before round 6). Up to 256 the forward 1x1 GEMMs gain 5-12 % (3 blocks per CU instead of 2:
// l3.x.c3 32.1 -> 29.6 us, l2.x.c3 47.2 -> 42.3, stem 34.2 -> 28.7); the dgrads are mixed
// (l1.0.c3 61.9 -> 56.4, l3.0.c1 65.0 -> 71.3), and K = 512 loses on both
// (profiles/one_stage_r6.txt)
inline bool igemm_one_stage(int mode, int depth, int Kdim, const Knobs& k) {
  return depth == 3 && mode != MODE_WGRAD && Kdim <= k.one_k[mode == MODE_FWD ? 0 : 1] && k.igemm_one;
}

// the BN-apply epilogue (forward-folded BN3) runs on the LDS-DMA tiles, not the register-staged ones
inline bool fwd_bnapply_supported(const Knobs& k) { return k.igemm_glds != 0; }

// ---- forward ------------------------------------------------------------------------------
struct FwdPlan {
  int cfg;
  int64_t m_tiles;   // = statistics-slab rows
  int64_t n_tiles;
  bool tap;          // tap-reuse tile (tg valid)
  TapGeom tg;
  int depth;         // main loop (igemm_loop; 7 / 8 tap reuse)
  bool one;          // single-stage form
  bool ok;           // the launcher takes it (else hipErrorInvalidValue)
};

// cfg_req < 0: auto. prologue: BN+ReLU operand prologue (not built into the tap loops).
inline FwdPlan plan_fwd(const ConvGeom& g, int64_t cfg_req, bool prologue, const Knobs& k) {
  FwdPlan p{};
  const int64_t M = (int64_t)g.N * g.P * g.Q;
  const int Kdim = g.R * g.S * g.C;
  p.cfg = cfg_req >= 0 ? (int)cfg_req : conv_cfg(g, g.C, g.K, M, Kdim, !prologue, false, k);
  const int bm = tile_m(p.cfg), bn = tile_n(p.cfg);
  if (bm == 0) return p;
  p.tap = is_tap_cfg(p.cfg);
  p.ok = !p.tap || (tap_geom(g, g.C, bm, tap_depth(p.cfg), k, &p.tg) && !prologue);
  p.m_tiles = conv_mtiles(g, g.C, p.cfg, M, k);
  p.n_tiles = cdiv(g.K, bn);
  p.depth = p.tap ? tap_depth(p.cfg) : igemm_loop(MODE_FWD, bm, bn, tile_waves(p.cfg), Kdim, g.C, g.R * g.S, prologue, false, k);
  p.one = igemm_one_stage(MODE_FWD, p.depth, Kdim, k);
  return p;
}

// ---- data gradient --------------------------------------------------------------------------
// strided dgrad = stride² sub-pixel classes (h ≡ ph, w ≡ pw mod stride): class (ph, pw) gets
// the taps r = r0 + st·i (i < nr), s = s0 + st·j (j < ns) and Hc x Wc output pixels per image
struct DgradClass {
  int ph, pw, r0, nr, s0, ns, Hc, Wc;
  int M;         // output rows N·Hc·Wc
  int m_tiles;   // M-tiles = its slab rows with a BnBwdStat
};
inline DgradClass dgrad_class(const ConvGeom& g, int ph, int pw) {
  DgradClass c{};
  const int st = g.stride;
  c.ph = ph;
  c.pw = pw;
  c.r0 = (ph + g.pad) % st;
  c.s0 = (pw + g.pad) % st;
  c.nr = c.r0 < g.R ? (g.R - c.r0 + st - 1) / st : 0;
  c.ns = c.s0 < g.S ? (g.S - c.s0 + st - 1) / st : 0;
  c.Hc = ph < g.H ? (g.H - ph + st - 1) / st : 0;
  c.Wc = pw < g.W ? (g.W - pw + st - 1) / st : 0;
  c.M = g.N * c.Hc * c.Wc;
  return c;
}

struct DgradPlan {
  int cfg;
  bool merged;       // every sub-pixel class in ONE launch (stride 2)
  int ncls;          // the non-empty (M > 0) classes: (ph, pw) order, or the merged kernel's
  DgradClass cls[16];   // (classes with more taps first: longest blocks dispatched first)
  int rows;          // statistics-slab rows = Σ m_tiles over every class, in cls order
  int64_t n_tiles;
  int64_t grid;      // merged: blocks of the one launch
  int max_M, max_Kdim;   // merged: launch-level choices (main loop, single-stage form) see the largest class
  bool tap;          // stride 1 on a tap-reuse tile
  TapGeom tg;
  int depth[16];     // per launch (merged: one)
  bool one[16];
  bool ok;
};

// cfg_req < 0: auto. cat_ch: channels of the K-concatenated second operand (BN3 fold), else 0.
// bstat: with the BN-statistics epilogue.
// SDX_DGRAD_MERGE: 0 one launch per class, 1 merged for every strided dgrad, 2 merged for
// strided 3x3 only (default: a strided 1x1 has one non-empty class, whose launch is faster
// on its own — profiles/dgrad_merge_r4.txt)
inline DgradPlan plan_dgrad(const ConvGeom& g, int64_t cfg_req, int cat_ch, bool bstat, const Knobs& k) {
  DgradPlan p{};
  const int st = g.stride;
  const int64_t M = (int64_t)g.N * g.H * g.W / (st * st);
  p.cfg = cfg_req >= 0 ? (int)cfg_req
                       : conv_cfg(g, g.K, g.C, M, (int64_t)g.R * g.S * (g.K + cat_ch) / (st * st), true, true, k);
  const int bm = tile_m(p.cfg), bn = tile_n(p.cfg);
  if (bm == 0 || st < 1 || st > 4) return p;
  p.n_tiles = cdiv(g.C, bn);
  p.merged = st == 2 && (k.dgrad_merge == 1 || (k.dgrad_merge == 2 && g.R > 1));
  for (int ph = 0; ph < st; ++ph)
    for (int pw = 0; pw < st; ++pw) {
      DgradClass c = dgrad_class(g, ph, pw);
      if (c.M == 0) continue;
      c.m_tiles = (int)(st == 1 ? conv_mtiles(g, g.K, p.cfg, c.M, k) : cdiv(c.M, bm));   // (a tap tile may pad rows)
      p.cls[p.ncls++] = c;
    }
  if (p.merged)   // stable insertion sort by taps, most first
    for (int i = 1; i < p.ncls; ++i)
      for (int j = i; j > 0 && p.cls[j].nr * p.cls[j].ns > p.cls[j - 1].nr * p.cls[j - 1].ns; --j) {
        const DgradClass t = p.cls[j];
        p.cls[j] = p.cls[j - 1];
        p.cls[j - 1] = t;
      }
  p.tap = is_tap_cfg(p.cfg);
  p.ok = st == 1 ? (!p.tap || tap_geom(g, g.K, bm, tap_depth(p.cfg), k, &p.tg)) : !p.tap;
  if (cat_ch > 0) p.ok = p.ok && !p.tap && dgrad_cat_supported(g, cat_ch, k);
  int64_t most = 0;
  for (int i = 0; i < p.ncls; ++i) {
    const DgradClass& c = p.cls[i];
    p.rows += c.m_tiles;
    most = c.m_tiles * p.n_tiles > most ? c.m_tiles * p.n_tiles : most;
    p.max_M = c.M > p.max_M ? c.M : p.max_M;
    p.max_Kdim = c.nr * c.ns * g.K > p.max_Kdim ? c.nr * c.ns * g.K : p.max_Kdim;
  }
  p.grid = most * p.ncls;
  const int launches = p.merged ? (p.ncls > 0 ? 1 : 0) : p.ncls;
  for (int i = 0; i < launches; ++i) {
    const DgradClass& c = p.cls[i];
    const int Kdim = (p.merged ? p.max_Kdim : c.nr * c.ns * g.K) + cat_ch;
    p.depth[i] = p.tap ? tap_depth(p.cfg)
                       : igemm_loop(MODE_DGRAD, bm, bn, tile_waves(p.cfg), Kdim, g.K + cat_ch, c.nr * c.ns, false, bstat, k);
    p.one[i] = igemm_one_stage(MODE_DGRAD, p.depth[i], Kdim, k);
    // K-concatenation: LDS-DMA loops only
    if (cat_ch > 0 && p.depth[i] != 3 && p.depth[i] != 6) p.ok = false;
  }
  return p;
}

// ---- weight gradient --------------------------------------------------------------------------
// Split normalisation, the one copy: `steps` reduction steps over at most `req` splits of
// `per` steps each (per a multiple of `unit`), every split non-empty. The binding sizes the
// partial slab by the result and the launcher addresses it by the same numbers.
struct Splits {
  int per, n;
};
inline Splits norm_splits(int64_t steps, int64_t req, int unit) {
  if (req < 1) req = 1;
  int64_t per = cdiv(steps, req);
  per = cdiv(per, unit) * unit;
  return {(int)per, (int)cdiv(steps, per)};
}

// -- 1x1 kernels (wgrad1x1.hip)
constexpr int kW1Bm = 128;    // output channels (dW rows) per block
constexpr int kW1BigBm = 256;

enum W1Kind { W1_PLAIN = 0, W1_PIPE, W1_PIPE_GEN, W1_BIG };

// pixel-pair view (stride 1, a 64-channel side: the layer-1 bottleneck 1x1 convs, reference
// networks/resnet_big.py:44,48 at planes = 64): two consecutive pixels' 64 channels form one
// 128-wide row, so the kernel's 128-row / 128-column tiles stay whole. The GEMM over the
// pair view also forms the even x odd cross blocks (MFMA work thrown away: these GEMMs are
// HBM-bound), while dy and x are read at full 16-B chunks in one pass
//
// Opt-in (SDX_W1_PAIRS=1, or wgrad1x1_pairs_set): measured no faster than the generic
// kernel at CIFAR (65-68 vs 70 us stand-alone at 256 blocks, in-step within noise) and slower
// at config 5 (71.3 vs 70.5 ms/step): the 32-pixel-pair step loop is latency-bound once its
// MFMA work doubles (profiles/wgrad1x1_pairs_r5.txt)
inline bool w1_pairs(const ConvGeom& g, const Knobs& k) {
  return k.w1_pairs != 0 && g.stride == 1 && g.R == 1 && g.S == 1 && g.pad == 0 && (g.K == 64 || g.C == 64) &&
         g.K % 64 == 0 && g.C % 64 == 0 && ((long)g.N * g.P * g.Q) % 64 == 0;
}

inline bool w1_pipe_enabled(const ConvGeom& g, const Knobs& k) {
  // 32-bit element offsets: dy (output pixels) and x (input pixels)
  return k.w1_pipe && (long)g.N * g.P * g.Q * g.K < (1L << 31) && (long)g.N * g.H * g.W * g.C < (1L << 31);
}

// the 256-row LDS-DMA kernel: dy channels % 256, the non-GEN x addressing (stride 1, or a
// strided shortcut whose 32-pixel step is whole output rows), not the pixel-pair view.
// SDX_W1_BIG / wgrad1x1_big_set: 0 off (the 128-row kernels for every shape), 1 (default) by
// the rule below, 2 every eligible shape.
// Only for GEMMs with steps_total x tiles >= SDX_W1_BIG_MIN (default 8192: >= 64 steps per
// split at the 128-block in-step target). Stand-alone the kernel is 2-12 % faster on every
// layer 2-4 shape; in the step, on every shape, it made the step 0.04 ms SLOWER (11.786 vs
// 11.749 ms, 3 interleaved rounds, profiles/w1_big_ab_r6.txt): its 128 KiB of LDS per block
// leaves no room for a main-stream block on its CU, and at 32 steps per split its fp32 slab
// round trip (twice the old kernel's at the same block count) eats the gain. The long-split
// shapes (projection blocks, l2 expand convs) keep 9-12 %.
inline bool w1_big(const ConvGeom& g, const Knobs& k) {
  if (!(k.w1_big != 0 && !w1_pairs(g, k) && g.K % kW1BigBm == 0 && g.C % 128 == 0 && w1_pipe_enabled(g, k) &&
        (g.stride == 1 || 32 % g.Q == 0)))
    return false;
  const long steps = (long)g.N * g.P * g.Q / 32;
  const long tiles = (long)(g.K / kW1BigBm) * (g.C / (g.C % 256 == 0 ? 256 : 128));
  return k.w1_big == 2 || steps * tiles >= k.w1_big_min;
}

// 1x1 wgrad kernels: K % 128 == 0, C % 128 == 0, N*H*W % 32 == 0 — stride 1 (any image
// size), or a strided 1x1 (projection shortcut, reference networks/resnet_big.py:50-55) on the
// pipelined kernel when the input is exactly st x the output (Q | 32: the x source of a step
// pixel is base + step·const; otherwise the GEN instantiation divides the step pixel index by
// Q; SDX_W1_STRIDED=0: strided shortcuts on the generic kernel) — or stride 1 with a
// 64-channel side (pixel pairs, N*H*W % 64)
inline bool w1_supported(const ConvGeom& g, const Knobs& k) {
  const bool strided_ok = k.w1_strided && g.stride > 1 && g.H == g.stride * g.P && g.W == g.stride * g.Q &&
                          (long)g.N * g.P * g.Q * g.Q < (1L << 32) && w1_pipe_enabled(g, k);
  if (g.R == 1 && g.S == 1 && g.pad == 0 && g.stride == 1 && g.P == g.H && g.Q == g.W && w1_pairs(g, k))
    return w1_pipe_enabled(g, k);
  return g.R == 1 && g.S == 1 && g.pad == 0 && (g.stride == 1 ? (g.P == g.H && g.Q == g.W) : strided_ok) &&
         g.K % kW1Bm == 0 && g.C % 128 == 0 && ((long)g.N * g.P * g.Q) % 32 == 0;
}

struct W1Geom {
  bool pairs;
  W1Kind kind;
  int Kv, Cv;   // the GEMM's rows / columns (pair view: twice the channels)
  int bn;       // column tile 128 | 256
  int k_tiles, c_tiles, steps;
};
// SDX_W1_BN=128 forces the 128-column tile on every shape (co-residency experiments: the
// non-pipelined 128x128 kernel holds 112 VGPRs, so an 8-wave main-stream block fits beside it)
inline W1Geom w1_geom(const ConvGeom& g, const Knobs& k) {
  W1Geom w{};
  w.pairs = w1_pairs(g, k);
  w.Kv = w.pairs ? 2 * g.K : g.K;
  w.Cv = w.pairs ? 2 * g.C : g.C;
  w.bn = k.w1_bn == 128 ? 128 : (w.Cv % 256 == 0 ? 256 : 128);
  const bool big = w1_big(g, k);
  // (a strided shape is supported only when the pipelined kernel is enabled)
  w.kind = big ? W1_BIG
               : w1_pipe_enabled(g, k) ? ((g.stride > 1 && 32 % g.Q != 0) ? W1_PIPE_GEN : W1_PIPE) : W1_PLAIN;
  w.k_tiles = w.Kv / (big ? kW1BigBm : kW1Bm);
  w.c_tiles = w.Cv / w.bn;
  w.steps = (int)((long)g.N * g.P * g.Q / (w.pairs ? 64 : 32));
  return w;
}

// -- tap-reuse 3x3 kernels (wgrad3x3.hip): stride 1 or 2, pad 1, C,K % 64 == 0
enum W3Kind { W3_PLAIN = 0, W3_PAD, W3_S2, W3_S2_PAD };

// padded-slot kernel: slot width WS (next power of two >= W) for stride-1 widths that are not
// one of {4, 8, 16, 32} (SDX_W3_PAD=0: those widths on the generic kernel)
inline int w3_pad_ws(const ConvGeom& g, const Knobs& k) {
  if (!k.w3_pad || g.stride != 1 || g.W == 4 || g.W == 8 || g.W == 16 || g.W == 32 || g.W < 5 || g.W > 64) return 0;
  const int ws = g.W <= 8 ? 8 : g.W <= 16 ? 16 : g.W <= 32 ? 32 : 64;
  const int sw = ws < 32 ? ws : 32, spr = ws / sw, rps = 32 / sw;
  return ((long)g.N * g.H * spr) % rps == 0 ? ws : 0;
}

// stride-2 slots per output row: Q itself (4/8/16/32), else the next of 8/16/32 above it
// (0: unsupported); a step is 32/slots whole output rows
inline int w3_s2_slots(const ConvGeom& g, const Knobs& k) {
  if (g.Q == 4 || g.Q == 8 || g.Q == 16 || g.Q == 32) return g.Q;
  // (w3_pad_ws of the output-sized stride-1 geometry: honours SDX_W3_PAD)
  if (g.Q < 5 || g.Q > 32 || !w3_pad_ws(ConvGeom{g.N, g.P, g.Q, g.C, g.K, 3, 3, g.P, g.Q, 1, 1}, k)) return 0;
  const int sq = g.Q <= 8 ? 8 : g.Q <= 16 ? 16 : 32;
  return ((long)g.N * g.P) % (32 / sq) == 0 ? sq : 0;
}

// SDX_W3_S2=0: stride-2 3x3 wgrads on the generic kernel
inline bool w3_supported(const ConvGeom& g, const Knobs& k) {
  const bool q_ok = g.Q == 4 || g.Q == 8 || g.Q == 16 || g.Q == 32;
  if (g.stride == 2 && k.w3_s2 && g.R == 3 && g.S == 3 && g.pad == 1 && g.P == g.Q && g.H == 2 * g.P &&
      g.W == 2 * g.Q && g.C % 64 == 0 && g.K % 64 == 0 && !q_ok && w3_s2_slots(g, k) > 0)
    return true;   // padded output rows
  const bool geo = g.stride == 1 ? (g.P == g.H && g.Q == g.W)
                                 : (k.w3_s2 && g.stride == 2 && g.H == 2 * g.P && g.W == 2 * g.Q);
  const bool base = g.R == 3 && g.S == 3 && g.pad == 1 && g.P == g.Q && geo && g.C % 64 == 0 && g.K % 64 == 0;
  if (base && g.stride == 1 && g.H == g.W && w3_pad_ws(g, k) > 0) return true;   // padded slots
  return base && q_ok && ((long)g.N * g.P * g.Q) % 32 == 0;
}

struct W3Geom {
  W3Kind kind;
  int slot;    // slot width: W (plain), WS (padded slots), Q or its padded width (stride 2)
  int steps;
};
inline W3Geom w3_geom(const ConvGeom& g, const Knobs& k) {
  W3Geom w{};
  const int ws = (g.stride == 1 && g.H == g.W) ? w3_pad_ws(g, k) : 0;
  if (ws > 0) {   // segments of the padded-slot kernel / segments per step
    const int sw = ws < 32 ? ws : 32;
    w = {W3_PAD, ws, (int)((long)g.N * g.H * (ws / sw) / (32 / sw))};
  } else if (g.stride == 2 && !(g.Q == 4 || g.Q == 8 || g.Q == 16 || g.Q == 32)) {   // padded rows
    const int sq = w3_s2_slots(g, k);
    w = {W3_S2_PAD, sq, sq > 0 ? (int)((long)g.N * g.P / (32 / sq)) : 0};
  } else {
    w = {g.stride == 2 ? W3_S2 : W3_PLAIN, g.stride == 2 ? g.Q : g.W, (int)((long)g.N * g.P * g.Q / 32)};
  }
  return w;
}

enum WgradFamily { WGRAD_GENERIC = 0, WGRAD_3X3, WGRAD_1X1 };

struct WgradPlan {
  bool ok;          // false: the request names a dedicated kernel (cfg 9 / 10) the shape does not fit
  WgradFamily family;
  int cfg;          // generic: its tile config; 9 / 10 for the 3x3 / 1x1 kernels
  W1Geom w1;        // family 1x1
  W3Geom w3;        // family 3x3
  int depth;        // generic: main loop
  int64_t steps;    // reduction steps (generic: the N·P·Q pixels, split in BK multiples)
  int64_t tiles;    // output tiles
  int per, splits;  // steps per split, normalised split count
  int64_t slices;   // partial-slab slices (pixel pairs: two per split)
  int64_t slab_elems;   // fp32 elements of the partial slab (0: none needed)
  bool direct;      // one split stored straight into dW
  int64_t grid;
};

// Split count of a dedicated (1x1 / 3x3) kernel: `target` 8-wave blocks, >= 8 steps per split
inline int64_t dedicated_splits(int64_t target, int64_t tiles, int64_t steps) {
  int64_t splits = target / tiles > 1 ? target / tiles : 1;
  const int64_t cap = steps / 8 > 1 ? steps / 8 : 1;
  return splits < cap ? splits : cap;
}

// splits_req <= 0: by the heuristics below. cfg_req: -1 auto (the dedicated kernels for every
// shape they support, else generic), -2 generic auto, 0-6 generic tile config, 9 the tap-reuse
// 3x3 kernel (wgrad3x3.hip), 10 the 1x1 kernel (wgrad1x1.hip); SDX_WGRAD3=0 / SDX_WGRAD1=0:
// generic only in auto dispatch. prologue: BN+ReLU operand prologue (generic kernel only).
inline WgradPlan plan_wgrad(const ConvGeom& g, int64_t splits_req, int64_t cfg_req, bool accumulate, bool prologue,
                            const Knobs& k) {
  WgradPlan p{};
  const int64_t M = g.K, Ncol = (int64_t)g.R * g.S * g.C, Kd = (int64_t)g.N * g.P * g.Q;
  int64_t splits = splits_req, cfg = cfg_req;
  const bool w3 = (cfg == 9 || (cfg == -1 && k.wgrad3 && splits <= 0)) && !prologue && w3_supported(g, k);
  const bool w1 = (cfg == 10 || (cfg == -1 && k.wgrad1 && splits <= 0)) && !prologue && w1_supported(g, k);
  if ((cfg == 9 && !w3) || (cfg == 10 && !w1)) return p;
  // The stage-1 weight gradients (the most pixels) are the last work of the backward: when
  // they run, the main stream has (almost) nothing left, so the half-chip block target that
  // keeps the side stream off the critical-path kernels only leaves CUs idle in the step's
  // tail (profiles: a 390 us gap before the SGD at 256 images/GPU). GEMMs with at least
  // SDX_W3_TAIL_PIX pixels (2^18 = stage 1 at 128 and 256 images/GPU) get
  // SDX_W3_TAIL_BLOCKS (default 256) blocks. Default 0 (off): the gap shrinks to 180 us but
  // the wider stage-1 wgrads slow the concurrent stage-1 dgrads more, 12.43 vs 12.37 ms
  // (512 blocks: 12.52; same-box A/B, profiles/tail_ab_r4.txt)
  const bool tail = k.w3_tail_pix > 0 && Kd >= k.w3_tail_pix;
  int unit = 1;
  if (w1) {
    p.family = WGRAD_1X1;
    p.cfg = 10;
    p.w1 = w1_geom(g, k);
    p.steps = p.w1.steps;
    p.tiles = (int64_t)p.w1.k_tiles * p.w1.c_tiles;
    // as for the 3x3 kernel: SDX_W3_BLOCKS (128) 8-wave blocks, >= 8 steps each;
    // pixel-pair shapes (HBM-bound, twice the MFMA work per byte): SDX_W1_PAIR_BLOCKS
    if (splits <= 0)
      splits = dedicated_splits(tail ? k.w3_tail_blocks : (p.w1.pairs ? k.w1_pair_blocks : k.w3_blocks), p.tiles, p.steps);
  } else if (w3) {
    p.family = WGRAD_3X3;
    p.cfg = 9;
    p.w3 = w3_geom(g, k);
    p.steps = p.w3.steps;
    p.tiles = (int64_t)(g.K / 64) * (g.C / 64);
    // SDX_W3_BLOCKS (default 128) 8-wave blocks, >= 8 steps per split. Standalone, 256
    // blocks (one per CU) is fastest (tools/w3_sweep.py), but in the training step these
    // kernels run on the wgrad side stream: a block holds ~416 of a SIMD lane's 512 VGPRs,
    // so the critical-path kernels (128-VGPR dgrads, the BN reductions) cannot co-reside on
    // its CU. 128 blocks leave half the CUs to the main stream: step 13.71 -> 13.34 ms at
    // 256 images/GPU, 8.48 -> 8.20 ms at 128 (profiles/wgrad3x3_r2.txt)
    if (splits <= 0) splits = dedicated_splits(tail ? k.w3_tail_blocks : k.w3_blocks, p.tiles, p.steps);
  } else {
    p.family = WGRAD_GENERIC;
    // 64-output-channel GEMMs with a wide reduction side (layer-1 3x3: 64 x 576): the 64x256
    // tile (four 64x64 wave tiles) beats the exact-fit 64x64 one despite its padding, at
    // ~512 blocks (tools/wgrad_split_probe.py: 145 -> 124 us)
    if (k.wgrad_wide64 && cfg < 0 && splits <= 0 && M <= 64 && Ncol >= 512) cfg = 2;
    if (cfg < 0) cfg = auto_cfg(M, Ncol, 0, false, k);
    if (tile_m(cfg) == 0 || is_tap_cfg(cfg)) return p;
    p.cfg = (int)cfg;
    p.steps = Kd;
    unit = kBK;
    p.tiles = cdiv(M, tile_m(cfg)) * cdiv(Ncol, tile_n(cfg));
    p.depth = igemm_loop(MODE_WGRAD, tile_m(cfg), tile_n(cfg), tile_waves(cfg), (int)Kd, 0, 0, prologue, false, k);
    if (splits <= 0) {
      // SDX_WGRAD_TARGET: block target of the generic wgrad split heuristic (default 512)
      splits = k.wgrad_target / p.tiles > 1 ? k.wgrad_target / p.tiles : 1;
      const int64_t max_splits = Kd / 512 > 1 ? Kd / 512 : 1;   // >= 8 K-tiles per split
      splits = splits < max_splits ? splits : max_splits;
      // bound the fp32 partial slab to ~64 MiB, and to ~16 MiB / 256 splits for 1x1 GEMMs with
      // a small output (M*Ncol <= 64K: the layer-1/2 pointwise convs), where the slab round
      // trip outweighs the extra splits' parallelism (profiles/wgrad_sweep_r1.txt: 83 -> 67 us
      // on the 256x64 layer-1 GEMMs; the 3x3 and larger GEMMs keep more splits)
      const bool small_1x1 = g.R == 1 && g.S == 1 && M * Ncol <= 65536;
      const int64_t bound = (small_1x1 ? (4LL << 20) : (16LL << 20)) / (M * Ncol);
      splits = splits < (bound > 1 ? bound : 1) ? splits : (bound > 1 ? bound : 1);
      if (small_1x1 && splits > 256) splits = 256;
    }
  }
  const Splits s = norm_splits(p.steps, splits, unit);
  p.per = s.per;
  p.splits = s.n;
  p.slices = (w1 && p.w1.pairs) ? 2 * (int64_t)s.n : s.n;
  p.slab_elems = (p.slices > 1 || accumulate) ? p.slices * M * Ncol : 0;
  // a single split writes straight into dW (unless accumulating; the pair view always reduces)
  p.direct = s.n == 1 && !accumulate && !(w1 && p.w1.pairs);
  p.grid = p.tiles * s.n;
  p.ok = true;
  return p;
}

}  // namespace sdx_plan
