// The level-histogram planner of xfl_amd/csrc/paths.hpp (level_tile,
// level_tiles_max, level_fold_passes). Host-only, its own main;
// tests/test_level_plan.py builds it with -fsanitize=address,undefined and
// runs it. Exit status 0 = every check held; a failed check prints its line.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

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

// the slots the nodes take at this tile against the bound the host sizes by
static void bound(std::vector<int64_t> counts, int tile) {
  int64_t rows = 0, slots = 0;
  for (int64_t c : counts) {
    rows += c;
    slots += (c + tile - 1) / tile;
  }
  CHECK(slots <= level_tiles_max(rows, (int)counts.size(), tile));
}

int main() {
  for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)100, (int64_t)100000, (int64_t)100000000})
    for (int nodes : {1, 2, 64, 4096})
      for (int nbins : {1, 256, 4096})
        for (int nfeat : {1, 64}) {
          const int t = level_tile(n, nodes, nfeat, nbins);
          CHECK(hist_tile_ok(t) && t <= hist_tile(n, nfeat, nbins));
        }
  // config 5: one node keeps hist_tile's 8192; 64 nodes of 1563 rows on average take 2048
  CHECK(level_tile(100000, 1, 64, 256) == 8192 && level_tile(100000, 64, 64, 256) == 2048);
  CHECK(level_tile(100, 4096, 1, 2) == 64);
  for (int tile : {64, 2048}) {
    bound({65, 0, 1, 64}, tile);
    bound({0, 0, 0}, tile);
    bound({1, 1, 1, 1, 1}, tile);
    bound({64, 64, 64}, tile);
    bound({90000, 300, 300, 9400}, tile);
  }
  CHECK(level_fold_passes(2048, 64, 32) == 0 && level_fold_passes(2049, 64, 32) == 1);
  CHECK(level_fold_passes(64 * 1024, 64, 32) == 1 && level_fold_passes(64 * 1024 + 1, 64, 32) == 2);
  if (!failed) printf("ok\n");
  return failed ? 1 : 0;
}
