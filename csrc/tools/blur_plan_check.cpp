// Stand-alone check of the blur kernel's host arithmetic (csrc/include/blur_plan.h): the
// automatic kernel size, the validity rule and the LDS plan, swept over S in 1..512 and k in
// 1..63 (and the automatic k and explicit rows-per-round requests).
// Build with -fsanitize=address,undefined (tests/test_blur_oracle.py does): for the smaller
// plans the LDS image is allocated at the plan's size and every stage / ring element the
// kernel addresses (aug.hip aug_blur_kernel: phases A, B, C of every round of every strip) is
// touched, and every row phase C reads must be the row phase B last wrote to that slot, so an
// undersized buffer or a ring that recycles a slot too early fails.
// `blur_plan_check --table` instead prints the plan of every (S, k, rows) of the sweep, one
// "S k rows -> ..." line each, which tests/test_blur_oracle.py compares with the Python mirror
// of make_plan (data/augment.py blur_plan).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "blur_plan.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

using namespace sdx_blur;

// the kernel's addressing, with row numbers in place of pixel values
static void simulate(int S, const Plan& p) {
  std::vector<float> lds((size_t)p.lds_bytes / 4);
  float* stage = lds.data() + p.w_floats;
  float* ring = stage + (size_t)p.rows * 3 * p.stage_w;
  CHECK(ring + (size_t)p.ring_rows * 3 * p.strip == lds.data() + lds.size());
  const int R = p.r, n_rounds = (S + p.rows - 1) / p.rows;
  std::vector<int> stored((size_t)S * S, 0);
  for (int x0 = 0; x0 < S; x0 += p.strip) {
    const int tw = std::min(p.strip, S - x0);
    const int xa = std::max(0, x0 - R), xb = std::min(S, x0 + tw + R), pw = xb - xa;
    CHECK(pw <= p.stage_w && tw <= p.strip);
    int o_next = 0;
    for (int n = 0; n <= n_rounds; ++n) {
      if (n < n_rounds) {   // A
        const int y0 = n * p.rows, nr = std::min(p.rows, S - y0);
        for (int rr = 0; rr < nr; ++rr)
          for (int t = 0; t < pw; ++t)
            for (int c = 0; c < 3; ++c) stage[((size_t)rr * 3 + c) * p.stage_w + t] = (float)(xa + t);
      }
      if (n > 0) {   // C
        const int y1 = std::min(n * p.rows, S) - 1;
        const int o_end = y1 == S - 1 ? S : y1 - R + 1;
        const int cnt = std::max(0, o_end - o_next);
        for (int o = o_next; o < o_next + cnt; ++o)
          for (int j = -R; j <= R; ++j) {
            const int yy = (int)reflect(o + j, S);
            CHECK(yy >= 0 && yy < S && yy <= y1 && yy > y1 - p.ring_rows);
            for (int t : {0, tw / 2, tw - 1})
              for (int c = 0; c < 3; ++c)
                CHECK(ring[((size_t)(yy % p.ring_rows) * 3 + c) * p.strip + t] == (float)yy);
          }
        for (int o = o_next; o < o_next + cnt; ++o)
          for (int t = 0; t < tw; ++t) ++stored[(size_t)o * S + x0 + t];
        o_next += cnt;
      }
      if (n == n_rounds) break;
      const int y0 = n * p.rows, nr = std::min(p.rows, S - y0);   // B
      for (int rr = 0; rr < nr; ++rr)
        for (int t = 0; t < tw; ++t) {
          for (int j = -R; j <= R; ++j) {
            const int xx = (int)reflect(x0 + t + j, S);
            CHECK(xx >= xa && xx < xb);
            CHECK(stage[((size_t)rr * 3 + 2) * p.stage_w + (xx - xa)] == (float)xx);
          }
          for (int c = 0; c < 3; ++c) ring[((size_t)((y0 + rr) % p.ring_rows) * 3 + c) * p.strip + t] = (float)(y0 + rr);
        }
    }
    CHECK(o_next == S);
  }
  for (int v : stored) CHECK(v == 1);   // every output pixel stored exactly once
}

static void check_plan(int S, int k_req, int rows_req, const Plan& p) {
  CHECK(p.k >= 3 && (p.k & 1) == 1 && p.r == (p.k - 1) / 2 && p.r <= S - 1);
  if (k_req > 0) CHECK(p.k == k_req);
  if (rows_req > 0) CHECK(p.rows == rows_req);
  CHECK(p.rows >= 1 && p.rows <= kMaxRows && p.ring_rows == p.k + p.rows - 1);
  CHECK(p.strip >= 1 && p.strip <= S && p.strip >= std::min(S, kMinStrip));
  CHECK(p.n_strips == (S + p.strip - 1) / p.strip);
  CHECK(p.stage_w == std::min(S, p.strip + 2 * p.r) && p.w_floats >= p.r + 1 && p.w_floats % 4 == 0);
  CHECK(p.lds_bytes == 4 * ((int64_t)p.w_floats + 3 * ((int64_t)p.rows * p.stage_w + (int64_t)p.ring_rows * p.strip)));
  CHECK(p.lds_bytes + kStaticLds <= kLdsPerCu && kLdsPerCu == 160 * 1024);
}

// k 0 = automatic, rows 0 = automatic: the requests AugConfig and the binding can make
static void print_table() {
  for (int S = 1; S <= 512; ++S)
    for (int k = 0; k <= 63; ++k)
      for (int rows : {0, 1, 3, 16}) {
        Plan p{};
        if (make_plan(S, k, rows, &p))
          printf("%d %d %d -> %d %d %d %d %lld\n", S, k, rows, p.k, p.rows, p.strip, p.n_strips, (long long)p.lds_bytes);
        else
          printf("%d %d %d -> none\n", S, k, rows);
      }
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "--table") == 0) {
    print_table();
    return 0;
  }
  int n_ok = 0, n_sim = 0;
  for (int S = 1; S <= 512; ++S) {
    for (int k = 1; k <= 63; ++k) {
      Plan p{};
      const bool ok = make_plan(S, k, 0, &p);
      const bool valid = k >= 3 && (k & 1) && (k - 1) / 2 <= S - 1;
      if (!valid) CHECK(!ok);
      if (!ok) continue;
      check_plan(S, k, 0, p);
      ++n_ok;
      // k <= 63 always finds a strip: 64 columns x (63 + 1) rows x 12 B < 160 KiB
      if ((S <= 40 || S % 37 == 0 || S == 224 || S == 512) && (k <= 9 || k % 10 == 3 || k == 63)) {
        simulate(S, p);
        ++n_sim;
      }
    }
    for (int k = 3; k <= 63; k += 2)
      if ((k - 1) / 2 <= S - 1) {
        Plan p{};
        CHECK(make_plan(S, k, 0, &p));
      }
    // the automatic size: odd, >= 3, accepted for every S >= 2
    const int ka = auto_kernel(S);
    CHECK(ka >= 3 && (ka & 1) == 1 && (S < 30 ? ka == 3 : ka == ((S / 10) | 1)));
    Plan p{};
    if (S >= 2) {
      CHECK(make_plan(S, 0, 0, &p) && p.k == ka);
      check_plan(S, 0, 0, p);
      if (S % 16 == 0 || S < 40) simulate(S, p);
    } else {
      CHECK(!make_plan(S, 0, 0, &p));
    }
    // explicit rows per round
    for (int rows : {1, 2, 3, 4, 8, 16}) {
      Plan q{};
      if (S >= 2 && make_plan(S, 0, rows, &q)) {
        check_plan(S, 0, rows, q);
        if (S % 56 == 0 || S < 12) simulate(S, q);
      }
    }
  }
  Plan p{};
  CHECK(auto_kernel(32) == 3 && auto_kernel(224) == 23);
  // the flagship shape: one strip, above the 64 KiB default, two workgroups per CU
  CHECK(make_plan(224, 0, 0, &p) && p.k == 23 && p.n_strips == 1 && p.lds_bytes > kLdsDefault &&
        2 * (p.lds_bytes + kStaticLds) <= kLdsPerCu);
  // refused, not wrapped: out-of-range requests, and a ring no 64-column strip can hold
  CHECK(!make_plan(0, 3, 0, &p) && !make_plan(-5, 3, 0, &p) && !make_plan(32, -3, 0, &p) && !make_plan(32, 4, 0, &p));
  CHECK(!make_plan(32, 1, 0, &p) && !make_plan(5, 11, 0, &p) && make_plan(5, 9, 0, &p));
  CHECK(!make_plan(32, 3, -1, &p) && !make_plan(32, 3, kMaxRows + 1, &p));
  CHECK(!make_plan(256, 255, 0, &p) && !make_plan(1 << 16, 3, 0, &p) && !make_plan(1 << 15, (1 << 15) - 1, 0, &p));
  CHECK(reflect(-3, 5) == 3 && reflect(7, 5) == 1 && reflect(4, 5) == 4 && reflect(0, 5) == 0);
  printf("BLUR-PLAN-OK %d plans, %d simulated\n", n_ok, n_sim);
  return 0;
}
