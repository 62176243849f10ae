// Stand-alone check of the conv dispatch plan (csrc/include/conv_plan.h): geometries swept
// over the edges of every support rule, under the default knobs and the switches that move a
// rule. Build with -fsanitize=address,undefined (tests/test_conv_plan.py does): every partial
// slab the plan sizes is allocated and the last element each split addresses is touched, so an
// undersized workspace or an overflowing product fails under the sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "conv_plan.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK failed: %s  [%s%s]\n", __FILE__, __LINE__, #c, g_case, g_sub); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

using namespace sdx_plan;

static char g_case[128], g_sub[128];
static const int64_t kInt31 = 1LL << 31;

static ConvGeom geom(int N, int H, int C, int K, int R, int st, int pad) {
  ConvGeom g{};
  g.N = N; g.H = g.W = H; g.C = C; g.K = K; g.R = g.S = R; g.stride = st; g.pad = pad;
  g.P = g.Q = (H + 2 * pad - R) / st + 1;
  return g;
}

// a padded-row tap tile's last fragment read stays inside the halo buffer, the halo fits its
// LDS pieces, and the virtual rows tile exactly
static void check_tap(const ConvGeom& g, int cdim, int cfg, const TapGeom& t, int64_t m_tiles) {
  const int bm = tile_m(cfg);
  CHECK(t.t_nhp <= tap_halo_kb(bm) && t.t_hp <= t.t_nhp * 8 && t.t_nch == cdim / 64 && t.t_rs == g.W + 2);
  if (t.t_rw > 0) {
    const int rows = bm / t.t_rw;
    CHECK(t.t_rw >= 16 && t.t_rw >= g.W && (t.t_rw & (t.t_rw - 1)) == 0 && g.H % rows == 0);
    CHECK((rows + 1) * t.t_rs + t.t_rw + 1 < tap_halo_kb(bm) * 8);   // last padded fragment's last pixel
    CHECK(m_tiles * bm == (int64_t)g.N * g.H * t.t_rw);
  } else {
    CHECK(m_tiles == cdiv((int64_t)g.N * g.H * g.W, bm));
    CHECK(t.t_imgs > 0 ? t.t_imgs * g.H * g.W == bm : (g.H * g.W) % bm == 0);
  }
}

static int check_fwd_dgrad(const ConvGeom& g, const Knobs& k) {
  int n = 0;
  const int64_t x_elems = (int64_t)g.N * g.H * g.W * g.C, y_elems = (int64_t)g.N * g.P * g.Q * g.K;
  for (int prologue = 0; prologue < 2; ++prologue) {
    const FwdPlan f = plan_fwd(g, -1, prologue != 0, k);
    CHECK(f.ok && tile_m(f.cfg) > 0 && (!f.tap || !prologue));
    CHECK(f.m_tiles * tile_m(f.cfg) >= (int64_t)g.N * g.P * g.Q && f.n_tiles * tile_n(f.cfg) >= g.K);
    CHECK(f.m_tiles * f.n_tiles < kInt31 && x_elems < kInt31 && y_elems < kInt31);   // 32-bit grid / GEMM indexing
    CHECK(f.depth == 1 || f.depth == 2 || f.depth == 3 || f.depth == 6 || f.depth == 7 || f.depth == 8);
    CHECK(!f.one || f.depth == 3);
    if (f.tap) check_tap(g, g.C, f.cfg, f.tg, f.m_tiles);
    ++n;
  }
  for (int bstat = 0; bstat < 2; ++bstat) {
    const DgradPlan d = plan_dgrad(g, -1, 0, bstat != 0, k);
    CHECK(d.ok && d.ncls >= 1 && d.ncls <= g.stride * g.stride && (!d.merged || g.stride == 2));
    // slab rows = the sum of the per-class M-tiles, and the classes cover dx exactly once
    int rows = 0;
    int64_t pix = 0, most = 0;
    for (int i = 0; i < d.ncls; ++i) {
      const DgradClass& c = d.cls[i];
      CHECK(c.M > 0 && c.m_tiles * (int64_t)tile_m(d.cfg) >= c.M);
      if (i > 0 && d.merged) CHECK(c.nr * c.ns <= d.cls[i - 1].nr * d.cls[i - 1].ns);   // most taps first
      rows += c.m_tiles;
      pix += c.M;
      most = c.m_tiles * d.n_tiles > most ? c.m_tiles * d.n_tiles : most;
    }
    CHECK(rows == d.rows && pix == (int64_t)g.N * g.H * g.W);
    CHECK(!d.merged || d.grid == most * d.ncls);
    CHECK(d.grid < kInt31);
    if (d.tap) check_tap(g, g.K, d.cfg, d.tg, d.rows);
    ++n;
  }
  return n;
}

// touch: allocate the partial slabs (the default knobs and the big shapes; an allocation per
// plan would dominate the sweep)
static int check_wgrad(const ConvGeom& g, const Knobs& k, bool touch) {
  int n = 0;
  const int64_t M = g.K, Ncol = (int64_t)g.R * g.S * g.C;
  const int64_t cfgs[] = {-1, -2, 3, 9, 10};
  const int64_t reqs[] = {0, 1, 7, 1000};
  for (int64_t cfg : cfgs)
    for (int64_t req : reqs)
      for (int acc = 0; acc < 2; ++acc)
        for (int prologue = 0; prologue < 2; ++prologue) {
          snprintf(g_sub, sizeof(g_sub), " wgrad cfg %ld req %ld acc %d bn %d", (long)cfg, (long)req, acc, prologue);
          const WgradPlan p = plan_wgrad(g, req, cfg, acc != 0, prologue != 0, k);
          if (!p.ok) {   // only a dedicated kernel asked for a shape it does not run
            CHECK(cfg == 9 || cfg == 10);
            CHECK(prologue || (cfg == 9 ? !w3_supported(g, k) : !w1_supported(g, k)));
            continue;
          }
          CHECK(cfg != 9 || p.family == WGRAD_3X3);
          CHECK(cfg != 10 || p.family == WGRAD_1X1);
          CHECK(!prologue || p.family == WGRAD_GENERIC);
          // the splits tile [0, steps) and none is empty
          CHECK(p.splits >= 1 && p.per >= 1 && p.steps >= 1);
          CHECK((int64_t)p.splits * p.per >= p.steps && (int64_t)(p.splits - 1) * p.per < p.steps);
          if (req > 0) CHECK(p.splits <= req);
          if (p.family == WGRAD_GENERIC) CHECK(p.per % kBK == 0 && tile_m(p.cfg) > 0 && !is_tap_cfg(p.cfg));
          // 32-bit sizes: grid, operand elements, the pixels a split starts at
          CHECK(p.grid == p.tiles * p.splits && p.grid < kInt31);
          CHECK((int64_t)g.N * g.P * g.Q * g.K < kInt31 && (int64_t)g.N * g.H * g.W * g.C < kInt31);
          if (p.family == WGRAD_1X1) {
            const W1Geom& w = p.w1;
            CHECK(w.k_tiles >= 1 && w.c_tiles >= 1 && w.k_tiles * (w.kind == W1_BIG ? kW1BigBm : kW1Bm) == w.Kv &&
                  w.c_tiles * w.bn == w.Cv);
            CHECK((int64_t)w.steps * (w.pairs ? 64 : 32) == (int64_t)g.N * g.P * g.Q);
            CHECK(w.kind != W1_PIPE_GEN || g.stride > 1);
            CHECK(p.slices == (w.pairs ? 2 : 1) * p.splits && (!w.pairs || !p.direct));
          } else {
            CHECK(p.slices == p.splits);
          }
          if (p.family == WGRAD_3X3) {
            CHECK(g.K % 64 == 0 && g.C % 64 == 0 && p.w3.slot >= 4 && p.w3.slot <= 64 && p.w3.steps == p.steps);
            const int out_w = g.stride == 2 ? g.Q : g.W;
            CHECK(p.w3.slot >= out_w && (p.w3.slot & (p.w3.slot - 1)) == 0);
          }
          // the partial slab: >= slices·M·Ncol when one is needed; allocate it and touch the last
          // element each split addresses
          CHECK(p.direct == (p.slices == 1 && !acc));
          CHECK(p.direct ? p.slab_elems == 0 : p.slab_elems >= p.slices * M * Ncol);
          if (touch && p.slab_elems > 0 && p.slab_elems <= (1 << 20)) {
            std::vector<float> slab((size_t)p.slab_elems);
            for (int64_t s = 0; s < p.slices; ++s) slab[(size_t)((s + 1) * M * Ncol - 1)] = (float)s;
            CHECK(slab[(size_t)p.slab_elems - 1] == (float)(p.slices - 1));
          }
          ++n;
        }
  g_sub[0] = 0;
  return n;
}

int main() {
  // knob settings: the defaults and each switch that moves a support rule or a split target
  std::vector<Knobs> ks(1);
  auto add = [&](void (*f)(Knobs&)) { ks.emplace_back(); f(ks.back()); };
  add([](Knobs& k) { k.tap3 = 0; });
  add([](Knobs& k) { k.tap_pad = false; });
  add([](Knobs& k) { k.conv_cfg = 4; });
  add([](Knobs& k) { k.cfg_rules = 7; });
  add([](Knobs& k) { k.dgrad_merge = 0; });
  add([](Knobs& k) { k.dgrad_merge = 1; });
  add([](Knobs& k) { k.igemm_glds = 0; k.igemm_depth = 1; });
  add([](Knobs& k) { k.igemm_glds = 2; });
  add([](Knobs& k) { k.wgrad3 = false; k.wgrad1 = false; });
  add([](Knobs& k) { k.w3_blocks = 256; k.w3_tail_pix = 1 << 12; k.w3_tail_blocks = 512; });
  add([](Knobs& k) { k.w1_pairs = 1; });
  add([](Knobs& k) { k.w1_big = 0; });
  add([](Knobs& k) { k.w1_big = 2; k.w1_bn = 128; });
  add([](Knobs& k) { k.w1_pipe = false; });
  add([](Knobs& k) { k.w1_strided = false; k.w3_pad = false; k.w3_s2 = false; });
  add([](Knobs& k) { k.wgrad_target = 4096; k.wgrad_wide64 = false; });

  const int sizes[] = {1, 4, 5, 7, 8, 14, 16, 28, 32, 33, 56, 64, 65};
  const int chans[] = {8, 64, 128, 256};
  const int batches[] = {1, 3, 32};
  struct Filt { int R, st, pad; };
  const Filt filts[] = {{1, 1, 0}, {1, 2, 0}, {3, 1, 1}, {3, 2, 1}, {7, 2, 3}, {3, 1, 0}};
  int n = 0;
  for (const Knobs& k : ks)
    for (const Filt& f : filts)
      for (int H : sizes)
        for (int N : batches)
          for (int C : chans)
            for (int K : chans) {
              if (H + 2 * f.pad < f.R) continue;
              if ((int64_t)N * H * H * (C > K ? C : K) > (1 << 22)) continue;   // keeps the sweep in seconds
              const ConvGeom g = geom(N, H, C, K, f.R, f.st, f.pad);
              snprintf(g_case, sizeof(g_case), "N %d H %d C %d K %d R %d st %d pad %d", N, H, C, K, f.R, f.st, f.pad);
              n += check_fwd_dgrad(g, k);
              n += check_wgrad(g, k, &k == &ks[0] && N == 3 && C == K);
            }

  // the K-concatenated dgrad: dy width a power-of-two multiple of a2's, both multiples of BK
  const Knobs k0;
  snprintf(g_case, sizeof(g_case), "cat");
  CHECK(dgrad_cat_supported(geom(8, 8, 64, 256, 1, 1, 0), 64, k0) && dgrad_cat_supported(geom(8, 8, 64, 256, 1, 1, 0), 256, k0));
  CHECK(!dgrad_cat_supported(geom(8, 8, 64, 192, 1, 1, 0), 64, k0) && !dgrad_cat_supported(geom(8, 8, 64, 256, 1, 1, 0), 96, k0));
  CHECK(!dgrad_cat_supported(geom(8, 8, 64, 256, 3, 1, 1), 64, k0) && !dgrad_cat_supported(geom(8, 8, 64, 256, 1, 2, 0), 64, k0));
  const DgradPlan cat = plan_dgrad(geom(512, 8, 256, 1024, 1, 1, 0), -1, 256, true, k0);
  CHECK(cat.ok && (cat.depth[0] == 3 || cat.depth[0] == 6) && cat.rows == cdiv(512 * 64, tile_m(cat.cfg)));
  Knobs kg;
  kg.igemm_glds = 0;
  CHECK(!plan_dgrad(geom(512, 8, 256, 1024, 1, 1, 0), -1, 256, true, kg).ok);
  // split normalisation at its edges
  for (int64_t steps : {1, 2, 63, 64, 65, 1000, 65536})
    for (int64_t req : {-3, 0, 1, 2, 7, 64, 100000})
      for (int unit : {1, 64}) {
        const Splits s = norm_splits(steps, req, unit);
        CHECK(s.n >= 1 && s.per % unit == 0 && (int64_t)s.n * s.per >= steps && (int64_t)(s.n - 1) * s.per < steps);
        const Splits again = norm_splits(steps, s.n, unit);   // binding and launcher agree
        CHECK(again.n == s.n && again.per == s.per);
      }
  // the largest supported operands keep every product inside int64 and the plan inside int32
  const ConvGeom big = geom(1024, 56, 256, 64, 1, 1, 0);
  snprintf(g_case, sizeof(g_case), "big");
  n += check_wgrad(big, k0, true);
  printf("CONV-PLAN-OK %d cases\n", n);
  return 0;
}
