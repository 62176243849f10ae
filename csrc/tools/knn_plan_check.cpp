// Stand-alone check of the k-NN binding layer's host arithmetic (csrc/include/knn_plan.h):
// shape rules, split plans and workspace sizes over the edge cases of the supported range.
// Build with -fsanitize=address,undefined (tests/test_knn.py does): every slab the plan
// sizes is allocated and every (split, query, slot) element the kernels address is touched,
// so an undersized workspace or an overflowing product fails under the sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "knn_plan.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

using namespace sdx_knn;

static void check_case(int64_t nq, int64_t nb, int64_t k, int64_t req) {
  Plan p{};
  CHECK(make_plan(nq, nb, k, req, &p));
  CHECK(p.n_split >= 1 && p.n_split <= kMaxSplits);
  if (req > 0) CHECK(p.n_split <= req);
  CHECK(p.rows_per_split % kBankTile == 0 && p.rows_per_split >= kBankTile);
  // the splits tile [0, nb) and none is empty
  CHECK((int64_t)p.n_split * p.rows_per_split >= nb);
  CHECK((int64_t)(p.n_split - 1) * p.rows_per_split < nb);
  CHECK(p.slab_elems == (p.n_split > 1 ? (int64_t)p.n_split * nq * k : 0));
  if (p.slab_elems > 0 && p.slab_elems <= (1 << 22)) {
    std::vector<float> slab_s((size_t)p.slab_elems);
    std::vector<int> slab_i((size_t)p.slab_elems);
    for (int s = 0; s < p.n_split; ++s)
      for (int64_t q = 0; q < nq; ++q) {
        const size_t base = ((size_t)s * nq + q) * k;   // the kernels' slab addressing
        for (int64_t j = 0; j < k; ++j) {
          slab_s[base + j] = (float)j;
          slab_i[base + j] = (int)j;
        }
      }
    CHECK(slab_i[(size_t)p.slab_elems - 1] == (int)(k - 1));
  }
}

int main() {
  for (int64_t D : {64, 128, 256, 512, 1024, 2048}) CHECK(dim_supported(D));
  for (int64_t D : {0, 32, 96, 192, 2047, 4096, -64}) CHECK(!dim_supported(D));
  CHECK(supported(2048, 1024, 256) && !supported(2048, 1025, 200) && !supported(512, 10, 257) &&
        !supported(512, 10, 0) && !supported(100, 10, 20));

  const int64_t nqs[] = {1, 5, 63, 64, 65, 70, 130, 10000};
  const int64_t nbs[] = {1, 63, 64, 65, 96, 257, 300, 1037, 2085, 50000};
  const int64_t ks[] = {1, 20, 96, 200, 256};
  const int64_t reqs[] = {0, 1, 3, 7, 64};
  int n = 0;
  for (int64_t nq : nqs)
    for (int64_t nb : nbs)
      for (int64_t k : ks)
        for (int64_t r : reqs) {
          if (k > nb) {
            Plan p{};
            CHECK(!make_plan(nq, nb, k, r, &p));
            continue;
          }
          check_case(nq, nb, k, r);
          ++n;
        }
  // out-of-range requests are refused, not wrapped
  Plan p{};
  CHECK(!make_plan(0, 10, 1, 0, &p) && !make_plan(10, 0, 1, 0, &p) && !make_plan(10, 10, 0, 0, &p));
  CHECK(!make_plan(10, 1000, 257, 0, &p) && !make_plan(10, 1000, 10, -1, &p) && !make_plan(10, 1000, 10, 65, &p));
  CHECK(!make_plan((1LL << 30) + 1, 1000, 10, 0, &p) && !make_plan(10, (1LL << 31), 10, 0, &p));
  // the largest accepted sizes keep the slab count inside int64
  CHECK(make_plan(1LL << 30, 1LL << 30, 256, 64, &p) && p.slab_elems == 64LL * (1LL << 30) * 256);
  // the CIFAR-sized case fills the chip with few splits
  CHECK(make_plan(10000, 50000, 200, 0, &p) && p.n_split >= 2 && p.n_split <= 8);
  CHECK(auto_splits(64, 100) == 1);
  printf("KNN-PLAN-OK %d cases\n", n);
  return 0;
}
