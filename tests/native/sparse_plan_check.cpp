// The sparse-aware histogram's planner of xfl_amd/csrc/paths.hpp (sparse_tile,
// sparse_tiles_max, hist_sparse). Host-only, its own main;
// tests/test_sparse_plan.py builds it with -fsanitize=address,undefined and
// runs it. Exit status 0 = every check held; a failed check prints its line.
#include <cstdint>
#include <cstdio>

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
  // the tile: hist_tile for the mean list, 257 internal bins; config 5 at 5 % (mean 5000: ten slots a feature)
  CHECK(sparse_tile(320000, 64, 256) == 512);
  CHECK(sparse_tiles_max(320000, 64, 512) == 689);
  // the clamps: no entry at all, the cap at the mean's power of two, the largest tile
  CHECK(sparse_tile(0, 64, 256) == 64 && sparse_tiles_max(0, 64, 64) == 64);
  CHECK(sparse_tile(102400, 1024, 256) == 128);  // mean 100 caps hist_tile's 8192
  CHECK(sparse_tiles_max(102400, 1024, 128) == 1824);
  CHECK(sparse_tile((int64_t)1 << 40, 1, 4095) == 8192);
  CHECK(sparse_tile(6400000, 64, 1) == 2048);  // every feature dense, 2 internal bins: 32 x 64 rows
  CHECK(sparse_tiles_max(63, 1, 64) == 1 && sparse_tiles_max(64, 1, 64) == 2);
  // the route on config 5 (100 k x 64 x 256), T given: direct = 6.4 M products;
  // sparse = nnz + 257 (nnz / tile + 64) + 64 x 260
  // (6.4 M >= 1.86 x sparse: sparse <= 3,440,860; tile 4096 there, 257 x (nnz / 4096 + 64) + 16,640 + nnz)
  const int64_t kRouteLast = 3206798, kRouteLastNoTotal = 3112709;
  CHECK(kSparseMinSaving >= 1.0);
  CHECK(hist_sparse(100000, 64, 256, 0, true));         // nothing outside the zero bins
  CHECK(hist_sparse(100000, 64, 256, 0, false));        // 100 k products for T
  CHECK(!hist_sparse(100000, 64, 256, 6400000, true));  // nnz = nfeat count: the dense call's products and more
  CHECK(!hist_sparse(100000, 64, 256, 6400000, false));
  CHECK(!hist_sparse(100000, 64, 256, 6400001, true));  // more than the call holds
  CHECK(!hist_sparse(100000, 64, 256, -1, true) && !hist_sparse(0, 64, 256, 0, true));
  CHECK(!hist_sparse(100000, 64, 4096, 0, true) && hist_sparse(100000, 64, 4095, 0, true));
  // at and around the threshold: the last nnz routed sparse with T, and what the T products cost
  CHECK(hist_sparse(100000, 64, 256, kRouteLast, true) && !hist_sparse(100000, 64, 256, kRouteLast + 1, true));
  CHECK(!hist_sparse(100000, 64, 256, kRouteLast, false));
  CHECK(hist_sparse(100000, 64, 256, kRouteLastNoTotal, false) &&
        !hist_sparse(100000, 64, 256, kRouteLastNoTotal + 1, false));
  // monotone in nnz between the tile's steps is not promised; beyond the threshold nothing routes sparse
  for (int64_t nnz = kRouteLast + 1; nnz <= 6400000; nnz += 9973) CHECK(!hist_sparse(100000, 64, 256, nnz, true));
  if (!failed) printf("ok\n");
  return failed ? 1 : 0;
}
