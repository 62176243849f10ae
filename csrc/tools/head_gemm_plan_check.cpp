// Stand-alone check of the MFMA classifier head's host arithmetic (csrc/include/head_gemm_plan.h).
// Build with -fsanitize=address,undefined (tests/test_headgemm_oracle.py does). It sweeps the
// supported range and the values just outside it and asserts that
//   - the tiles of every form cover every output element exactly once (every element is
//     marked through the kernels' own tile -> element addressing, in a buffer of the exact
//     output size, so a tile that reaches past the output fails under the sanitizers),
//   - no count overflows int (each is recomputed in 64 bits and compared),
//   - the plan does not depend on G beyond the G·C extent.
// --dump prints the plans of a fixed case list, one line each, for the Python mirror of the plan.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "head_gemm_plan.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

using namespace sdx_headgemm;

static const int64_t kIntMax = 2147483647LL;

static void check_form(const Form& f, int64_t m, int64_t n, int64_t red, bool cover) {
  CHECK(f.m == m && f.n == n && f.red == red);
  const int64_t tm = (m + kTile - 1) / kTile, tn = (n + kTile - 1) / kTile, ch = (red + kChunk - 1) / kChunk;
  CHECK(tm * tn <= kIntMax && ch * kChunk <= kIntMax);
  CHECK(f.tiles_m == tm && f.tiles_n == tn && f.chunks == ch && f.red_pad == ch * kChunk && f.tiles == tm * tn);
  CHECK(f.red_pad >= red && f.red_pad - red < kChunk && f.chunks >= 1);
  if (!cover || m * n > (1 << 20)) return;
  std::vector<unsigned char> seen((size_t)(m * n), 0);
  for (int bid = 0; bid < f.tiles; ++bid) {
    const int t_m = bid / f.tiles_n, t_n = bid - t_m * f.tiles_n;   // the kernel's block -> tile map
    for (int i = 0; i < kTile; ++i)
      for (int j = 0; j < kTile; ++j) {
        const int64_t r = (int64_t)t_m * kTile + i, c = (int64_t)t_n * kTile + j;
        if (r < m && c < n) ++seen[(size_t)(r * n + c)];
      }
  }
  for (size_t e = 0; e < seen.size(); ++e) CHECK(seen[e] == 1);
}

static void check_case(int64_t G, int64_t B, int64_t K, int64_t C, bool cover) {
  Plan p{};
  CHECK(make_plan(G, B, K, C, &p));
  check_form(p.nt, B, G * C, K, cover);
  check_form(p.nn, B, K, C, cover);
  check_form(p.tn, G * C, K, B, cover);
  CHECK(p.rows == G * B && (int64_t)p.row_blocks * kRowsPerBlock >= G * B &&
        (int64_t)(p.row_blocks - 1) * kRowsPerBlock < G * B);
  CHECK((int64_t)p.bias_blocks * kBiasPerBlock >= G * C && (int64_t)(p.bias_blocks - 1) * kBiasPerBlock < G * C);
  CHECK((int64_t)p.tn.tiles + p.bias_blocks <= kIntMax);
  CHECK(p.logits_elems == G * B * C && p.logits_elems <= kIntMax && p.rowstat_elems == G * B * 3 &&
        p.rowstat_elems <= kIntMax);
  // G only stretches the G·C extent: the plan of G heads of C classes is the plan of one head
  // of G·C classes wherever that one is in range, and the per-head quantities are those of G = 1
  Plan one{};
  CHECK(make_plan(1, B, K, C, &one));
  CHECK(one.nn.tiles == p.nn.tiles && one.nn.chunks == p.nn.chunks && one.nn.tiles_m == p.nn.tiles_m);
  CHECK(one.nt.chunks == p.nt.chunks && one.nt.tiles_m == p.nt.tiles_m && one.tn.chunks == p.tn.chunks &&
        one.tn.tiles_n == p.tn.tiles_n);
  Plan wide{};
  if (G * C <= kMaxC && make_plan(1, B, K, G * C, &wide)) {
    CHECK(memcmp(&wide.nt, &p.nt, sizeof(Form)) == 0 && memcmp(&wide.tn, &p.tn, sizeof(Form)) == 0);
    CHECK(wide.bias_blocks == p.bias_blocks);
  }
}

static void dump_case(int64_t G, int64_t B, int64_t K, int64_t C) {
  Plan p{};
  const bool ok = make_plan(G, B, K, C, &p);
  printf("%lld %lld %lld %lld %d", (long long)G, (long long)B, (long long)K, (long long)C, ok ? 1 : 0);
  if (ok) {
    const Form* fs[3] = {&p.nt, &p.nn, &p.tn};
    for (const Form* f : fs)
      printf(" %d %d %d %d %d %d %d %d", f->m, f->n, f->red, f->tiles_m, f->tiles_n, f->red_pad, f->chunks, f->tiles);
    printf(" %d %d %d %lld %lld", p.rows, p.row_blocks, p.bias_blocks, (long long)p.logits_elems,
           (long long)p.rowstat_elems);
  }
  printf("\n");
}

int main(int argc, char** argv) {
  const int64_t Gs[] = {1, 2, 3, 16};
  const int64_t Bs[] = {1, 5, 31, 33, 63, 64, 65, 256, 1000};
  const int64_t Ks[] = {64, 128, 192, 2048, 4032, 4096};
  const int64_t Cs[] = {1, 3, 17, 63, 64, 65, 1000, 1030, 32768};
  if (argc > 1 && strcmp(argv[1], "--dump") == 0) {
    for (int64_t G : Gs)
      for (int64_t B : Bs)
        for (int64_t K : Ks)
          for (int64_t C : Cs) dump_case(G, B, K, C);
    dump_case(1, 8, 96, 10);
    dump_case(1, 8, 64, 40000);
    dump_case(17, 8, 64, 10);
    dump_case(16, 1 << 20, 64, 1000);
    return 0;
  }
  int n = 0;
  for (int64_t G : Gs)
    for (int64_t B : Bs)
      for (int64_t K : Ks)
        for (int64_t C : Cs) {
          const bool fits = G * B * C < (1LL << 31) && G * C * K < (1LL << 31);   // B·K is small here
          CHECK(supported(G, B, K, C) == fits);
          if (!fits) {
            Plan q{};
            CHECK(!make_plan(G, B, K, C, &q));
            continue;
          }
          check_case(G, B, K, C, /*cover=*/K <= 192 || (B <= 65 && C <= 65 && G <= 3));
          ++n;
        }
  // just outside the range: refused, and the plan is left alone
  Plan p{};
  p.rows = -7;
  const int64_t bad[][4] = {{0, 8, 64, 10},  {17, 8, 64, 10},    {1, 0, 64, 10},    {1, 8, 0, 10},     {1, 8, 32, 10},
                            {1, 8, 96, 10},  {1, 8, 4160, 10},   {1, 8, 8192, 10},  {1, 8, 64, 0},     {1, 8, 64, 32769},
                            {1, 8, 64, 40000}, {-1, 8, 64, 10},  {1, -8, 64, 10},   {1, 8, -64, 10},   {1, 8, 64, -1}};
  for (const auto& b : bad) {
    CHECK(!supported(b[0], b[1], b[2], b[3]) && !make_plan(b[0], b[1], b[2], b[3], &p));
    CHECK(p.rows == -7);
  }
  // element counts at 2^31: B·K, G·B·C, G·C·K
  CHECK(supported(1, (1LL << 25) - 1, 64, 1) && !supported(1, 1LL << 25, 64, 1));
  CHECK(supported(1, 65535, 64, 32768) && !supported(1, 65536, 64, 32768));
  CHECK(supported(16, 1, 4096, 32767) && !supported(16, 1, 4096, 32768));
  CHECK(!supported(1, 1LL << 31, 64, 1) && !supported(1, 1LL << 40, 64, 1));
  // the largest accepted extents keep every count inside int
  check_case(1, (1LL << 25) - 1, 64, 1, false);
  check_case(1, 65535, 64, 32768, false);
  check_case(16, 1, 4096, 32767, false);
  check_case(16, 4095, 64, 32768, false);
  printf("HEAD-GEMM-PLAN-OK %d cases\n", n + 4);
  return 0;
}
