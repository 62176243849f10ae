// Stand-alone check of the tile maps and plans of the two-view loss GEMMs
// (csrc/include/loss_gemm_plan.h, barlow_plan.h, vicreg_plan.h): the grouped walk is a bijection onto
// its grid and keeps a group's consecutive tiles in one tile column; the triangle fold visits every
// tile (ti, tj), ti <= tj, exactly once. Build with -fsanitize=address,undefined
// (tests/test_loss_gemm_plan.py does): every visit is counted in an array of exactly the grid's size,
// so a tile outside the grid fails under the sanitizers as well.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "barlow_plan.h"
#include "vicreg_plan.h"

#define CHECK(c)                                                                                  \
  do {                                                                                            \
    if (!(c)) {                                                                                   \
      fprintf(stderr, "%s:%d: CHECK failed: %s  [%s]\n", __FILE__, __LINE__, #c, g_case);         \
      exit(1);                                                                                    \
    }                                                                                             \
  } while (0)

namespace lg = sdx_lossgemm;

static char g_case[128];

// every logical tile of a rows x cols grid, walked in groups: a bijection, in the documented order
static void check_walk(int rows, int cols, int group) {
  snprintf(g_case, sizeof(g_case), "walk %d x %d group %d", rows, cols, group);
  std::vector<int> seen((size_t)rows * cols, 0);
  lg::TilePos prev{};
  for (int lt = 0; lt < rows * cols; ++lt) {
    const lg::TilePos t = lg::grouped_walk(lt, rows, cols, group);
    CHECK(t.row >= 0 && t.row < rows && t.col >= 0 && t.col < cols);
    CHECK(++seen[(size_t)t.row * cols + t.col] == 1);
    if (lt > 0) {
      const bool same_group = t.row / group == prev.row / group;
      if (same_group && t.col == prev.col) CHECK(t.row == prev.row + 1);                  // down the column,
      else if (same_group) CHECK(t.col == prev.col + 1 && t.row == t.row / group * group);   // the group's next column,
      else CHECK(t.col == 0 && t.row == (prev.row / group + 1) * group && prev.col == cols - 1);   // the next group
    }
    prev = t;
  }
}

// the cov launch of one view at dimension d: fold_h x fold_w logical tiles onto the triangle of T
static void check_fold(int d) {
  snprintf(g_case, sizeof(g_case), "fold D %d", d);
  sdx_vicreg::Plan pl{};
  CHECK(sdx_vicreg::make_plan(2, d, &pl));
  const int T = pl.c_t;
  CHECK(T == (int)lg::ceil_div(d, lg::kTile) && pl.c_tiles == T * (T + 1) / 2);
  CHECK(pl.c_fold_w * pl.c_fold_h == pl.c_tiles);
  std::vector<int> seen((size_t)T * T, 0);
  for (int lt = 0; lt < pl.c_tiles; ++lt) {   // as vic_cov_kernel finds its tile
    const lg::TilePos rc = lg::grouped_walk(lt, pl.c_fold_h, pl.c_fold_w, lg::kGroup);
    CHECK(rc.row >= 0 && rc.row < pl.c_fold_h && rc.col >= 0 && rc.col < pl.c_fold_w);
    const lg::TilePos t = lg::tri_fold(rc.row, rc.col, T);
    CHECK(t.row >= 0 && t.row <= t.col && t.col < T);
    CHECK(++seen[(size_t)t.row * T + t.col] == 1);
  }
  for (int ti = 0; ti < T; ++ti)
    for (int tj = 0; tj < T; ++tj) CHECK(seen[(size_t)ti * T + tj] == (ti <= tj ? 1 : 0));
}

int main() {
  int n = 0;
  for (int T = 1; T <= lg::kMaxD / lg::kTile; ++T, ++n) check_fold(lg::kTile * T);
  for (int d : {64, 192, 320}) {   // the last tile half empty
    check_fold(d);
    ++n;
  }
  for (int rows = 1; rows <= 17; ++rows)
    for (int cols = 1; cols <= 9; ++cols, ++n) check_walk(rows, cols, lg::kGroup);
  // both plans fill the shared part alike, and their grids are the ones the walks are checked for
  snprintf(g_case, sizeof(g_case), "plans");
  for (int d : {64, 192, 320, 2048, 8192})
    for (int rows : {1, 2, 8, 40, 264, 1024}) {
      sdx_barlow::Plan b{};
      sdx_vicreg::Plan v{};
      CHECK(sdx_barlow::make_plan(rows, d, &b) && sdx_vicreg::make_plan(rows, d, &v));
      CHECK(b.n == rows && b.d == d && v.n == rows && v.d == d);
      CHECK(b.b_tiles_m == v.b_tiles_m && b.b_tiles_n == v.b_tiles_n && b.b_tiles == v.b_tiles &&
            b.b_chunks == v.b_chunks && b.stat_blocks == v.stat_blocks);
      CHECK(b.b_tiles == b.b_tiles_m * b.b_tiles_n && b.b_tiles_m * lg::kTileMB >= rows && b.b_tiles_n * lg::kTile >= d);
      CHECK(b.b_chunks * lg::kChunk == d && b.stat_blocks * lg::kStatCols == d);
      CHECK(b.x_tiles == b.x_tiles_m * b.x_tiles_n && b.x_tiles_m == v.c_t && b.x_chunks == v.c_chunks);
      CHECK(b.x_chunks * lg::kChunk >= rows && b.loss_blocks * lg::kLossRows == d && v.loss_blocks == 2 * b.loss_blocks);
      check_walk(b.b_tiles_m, b.b_tiles_n, lg::kGroup);
      check_walk(b.x_tiles_m, b.x_tiles_n, lg::kGroup);
      ++n;
    }
  CHECK(!lg::supported(0, 64) && !lg::supported(2, 32) && !lg::supported(2, 8256) && !lg::supported(2, 96));
  CHECK(!lg::supported(1 << 18, 8192) && lg::supported((1 << 18) - 1, 8192));   // n·d < 2^31
  printf("LOSS-GEMM-PLAN-OK %d cases\n", n);
  return 0;
}
