// The level-wise sparse histogram's planner of xfl_amd/csrc/paths.hpp
// (level_sparse_tile, level_sparse_tiles_max, level_sparse). Host-only, its own
// main; tests/test_level_sparse_plan.py builds it with
// -fsanitize=address,undefined and runs it. Exit status 0 = every check held; a
// failed check prints its line.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../xfl_amd/csrc/paths.hpp"

using namespace xhe::paths;

static int failed = 0;
#define CHECK(cond)                                        \
  do {                                                     \
    if (!(cond)) {                                         \
      printf("line %d: %s\n", __LINE__, #cond);            \
      ++failed;                                            \
    }                                                      \
  } while (0)

int main() {
  // config 5 at 5 % (320 k kept entries), 257 internal bins. 64 nodes: 4096 groups of 79 on average, the tile is
  // capped at that mean's power of two; 2 nodes: 128 groups of 2500, hist_tile's fill rule decides
  CHECK(level_sparse_tile(320000, 64, 64, 256) == 128);
  CHECK(level_sparse_tiles_max(320000, 64, 64, 128) == 2500 + 4096);
  CHECK(level_sparse_tile(320000, 2, 64, 256) == 512);
  CHECK(level_sparse_tiles_max(320000, 2, 64, 512) == 625 + 128);
  // one node is the node-wise call's plan
  CHECK(level_sparse_tile(320000, 1, 64, 256) == sparse_tile(320000, 64, 256));
  CHECK(level_sparse_tiles_max(320000, 1, 64, 512) == sparse_tiles_max(320000, 64, 512));
  // the clamps: no entry at all, the deepest level (mean under one entry), the largest tile
  CHECK(level_sparse_tile(0, 64, 64, 256) == 64 && level_sparse_tiles_max(0, 64, 64, 64) == 4096);
  CHECK(level_sparse_tile(1000, 4096, 64, 256) == 64 && level_sparse_tiles_max(1000, 4096, 64, 64) == 15 + 262144);
  CHECK(level_sparse_tile((int64_t)1 << 40, 1, 1, 4095) == 8192);
  CHECK(level_sparse_tiles_max(63, 1, 1, 64) == 1 && level_sparse_tiles_max(64, 1, 1, 64) == 2);
  // the route on config 5 (100 k x 64 x 256), the measured model of paths.hpp: direct = 6.4 M + 2 x 256 groups;
  // sparse = 1.16 nnz + 0.9 x 257 slots + 4 groups + 930 k (+ 1.7 M without totals); sparse at 1.05 and above
  CHECK(kLevelSparseMinSaving == 1.05 && kLevelSparseNodesMeasured == 256);
  CHECK(level_sparse(100000, 64, 64, 256, 320000, true));    // 2.99
  CHECK(level_sparse(100000, 64, 64, 256, 320000, false));   // 1.87
  CHECK(level_sparse(100000, 64, 64, 256, 1280000, true));   // 2.15
  CHECK(level_sparse(100000, 2, 64, 256, 3200000, true));    // 1.36
  CHECK(level_sparse(100000, 256, 64, 256, 1279372, false)); // 1.44
  CHECK(level_sparse(100000, 64, 64, 256, 3197658, false));  // 1.059: the lowest ratio taken, measured 1.48 x faster
  // measured ties and losses stay dense: 2 nodes at d = 0.5 without totals (1.001), 2 nodes at d = 0.8 (0.918)
  CHECK(!level_sparse(100000, 2, 64, 256, 3197658, false) && !level_sparse(100000, 2, 64, 256, 5118191, true));
  CHECK(!level_sparse(100000, 16, 64, 256, 3197658, false));  // 1.024: measured faster, left to sparse=True
  // every entry outside its zero bin never routes sparse, at any level, with or without totals (0.63 to 0.98)
  for (int nn : {1, 2, 4, 16, 64, 256})
    CHECK(!level_sparse(100000, nn, 64, 256, 6400000, true) && !level_sparse(100000, nn, 64, 256, 6400000, false));
  for (int nn : {1, 2, 4}) CHECK(!level_sparse(100000, nn, 64, 256, 5120000, true));  // d = 0.8 at shallow levels
  CHECK(!level_sparse(100000, 64, 64, 256, 6400001, true));  // more than the call holds
  // a small call does not pay for the fixed 3 ms: 1000 rows x 4 features, nothing outside the zero bins
  CHECK(!level_sparse(1000, 2, 4, 16, 0, true) && !level_sparse(10000, 2, 64, 256, 0, true));
  // beyond the node counts measured the dense call runs
  CHECK(level_sparse(100000, 256, 64, 256, 0, true) && !level_sparse(100000, 257, 64, 256, 0, true));
  CHECK(!level_sparse(100000, 4096, 64, 256, 0, true));
  CHECK(!level_sparse(100000, 64, 64, 256, -1, true) && !level_sparse(0, 64, 64, 256, 0, true));
  CHECK(!level_sparse(100000, 64, 64, 4096, 0, true) && level_sparse(100000, 2, 64, 4095, 0, true));
  CHECK(!level_sparse(100000, 0, 64, 256, 0, true) && !level_sparse(100000, 4097, 64, 256, 0, true));
  // the totals' products only ever count against the sparse call
  for (int64_t nnz = 0; nnz <= 6400000; nnz += 99991)
    for (int nn : {1, 2, 16, 64, 256})
      CHECK(!level_sparse(100000, nn, 64, 256, nnz, false) || level_sparse(100000, nn, 64, 256, nnz, true));
  if (!failed) printf("ok\n");
  return failed ? 1 : 0;
}
