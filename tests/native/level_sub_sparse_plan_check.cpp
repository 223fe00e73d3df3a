// The planner of the subtraction on the sparse level histogram in
// xfl_amd/csrc/paths.hpp (sub_sparse_list, level_sub_sparse). Host-only, its
// own main; tests/test_level_sub_sparse_plan.py builds it with
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
  // the inversion list: the listed cells are no more than the cells nor than the entries; then a Q per group, a T per pair
  CHECK(sub_sparse_list(15, 40, 3, 1) == 15 + 3 + 1);
  CHECK(sub_sparse_list(15, 7, 3, 1) == 7 + 3 + 1 && sub_sparse_list(15, 0, 3, 1) == 4);
  // config 5 at 64 nodes: 32 pairs, 2048 groups, 524,288 cells; 320 k entries bound the listed cells
  CHECK(sub_sparse_list((int64_t)32 * 64 * 256, 320000, 32 * 64, 32) == 320000 + 2048 + 32);
  // the chains' chunks cover the bound: at most kSibChunkMax entries each, whatever the list's real length
  for (int64_t n : {(int64_t)2, (int64_t)19, (int64_t)163840, (int64_t)2000000, (int64_t)1 << 30}) {
    const int c = sib_chunk(n);
    const int64_t nchunks = (n + c - 1) / c;
    CHECK(c >= kSibChunkMin && c <= kSibChunkMax && nchunks * c >= n);
    for (int64_t len : {(int64_t)0, n / 3, n}) CHECK((len + nchunks - 1) / nchunks <= c);  // chunk 0's entries of a shorter list
  }
  // the build's slot bound takes the whole nnz_bound with the pairs as nodes
  CHECK(level_sparse_tiles_max(320000, 32, 64, level_sparse_tile(320000, 32, 64, 256)) >= 320000 / 8192 + 32 * 64);

  // the route on config 5 (100 k x 64 x 256) at the measured points (profiles/r30/hist_level_sub_sparse/): nnz of d =
  // 0.05, 0.2, 0.5, 0.8. Taken: the five measured faster than both others by 5 % and more with even and with skewed
  // children; every point measured slower than either stays where it was
  const int64_t d05 = 320134, d20 = 1279372, d50 = 3197658, d80 = 5118191;
  CHECK(level_sub_sparse(100000, 2, 64, 256, d20, true) && level_sub_sparse(100000, 2, 64, 256, d50, true));
  CHECK(level_sub_sparse(100000, 16, 64, 256, d50, true));
  CHECK(level_sub_sparse(100000, 64, 64, 256, d05, true) && level_sub_sparse(100000, 64, 64, 256, d05, false));
  CHECK(!level_sub_sparse(100000, 2, 64, 256, d05, true) && !level_sub_sparse(100000, 2, 64, 256, d05, false));    // a tie, slower
  CHECK(!level_sub_sparse(100000, 16, 64, 256, d05, true) && !level_sub_sparse(100000, 16, 64, 256, d05, false));  // the sparse call
  CHECK(!level_sub_sparse(100000, 16, 64, 256, d20, true) && !level_sub_sparse(100000, 16, 64, 256, d20, false));  // the sparse call
  CHECK(!level_sub_sparse(100000, 2, 64, 256, d80, true));  // the subtraction with skewed children
  for (int nn : {2, 16, 64}) CHECK(!level_sub_sparse(100000, nn, 64, 256, d80, false));  // the subtraction
  CHECK(!level_sub_sparse(100000, 2, 64, 256, d50, false));                              // the subtraction
  CHECK(!level_sub_sparse(100000, 2, 64, 256, d20, false) && !level_sub_sparse(100000, 16, 64, 256, d50, false));  // skewed: the subtraction
  // outside the measured range: odd or too few nodes, more than 64, densities below 5 % and above 80 %
  for (bool t : {true, false})
    for (int64_t nnz : {(int64_t)0, d05, d20, d50, d80, (int64_t)6400000})
      for (int nn : {0, 1, 3, 63, 65, 66, 128, 256, 257, 4096}) CHECK(!level_sub_sparse(100000, nn, 64, 256, nnz, t));
  for (int nn : {2, 16, 64}) {
    CHECK(!level_sub_sparse(100000, nn, 64, 256, 319999, true) && !level_sub_sparse(100000, nn, 64, 256, 5120001, true));
    CHECK(!level_sub_sparse(100000, nn, 64, 256, 0, true) && !level_sub_sparse(100000, nn, 64, 256, -1, true));
  }
  CHECK(!level_sub_sparse(0, 2, 64, 256, 0, true) && !level_sub_sparse(100000, 2, 64, 4096, d20, true));
  CHECK(!level_sub_sparse(1000, 2, 4, 16, 800, true));  // a small call does not pay for the fixed cost
  // monotone in nnz on both sides of one window: with rising nnz the route is taken up at most once and, once given
  // up, never taken again (below the window the sparse call has nothing worth halving or the range ends, above it the
  // subtraction's dense build is the cheaper one)
  int windows = 0;
  for (bool t : {true, false})
    for (int nn : {2, 4, 8, 16, 32, 64}) {
      bool prev = false, lost = false;
      for (int64_t nnz = 0; nnz <= 6400000; nnz += 9999) {
        const bool route = level_sub_sparse(100000, nn, 64, 256, nnz, t);
        CHECK(!(lost && route));
        lost = lost || (prev && !route);
        windows += route && !prev;
        prev = route;
      }
    }
  CHECK(windows >= 4);  // (the loop above looked at a live route)
  // the totals' products only ever count against the combined call
  for (int nn : {2, 16, 64})
    for (int64_t nnz = d05; nnz <= d80; nnz += 99991) {
      CHECK(level_sub_sparse_cost(100000, nn, 64, 256, nnz, false) > level_sub_sparse_cost(100000, nn, 64, 256, nnz, true));
      CHECK(nn == 64 || !level_sub_sparse(100000, nn, 64, 256, nnz, false) || level_sub_sparse(100000, nn, 64, 256, nnz, true));
    }
  if (!failed) printf("ok\n");
  return failed ? 1 : 0;
}
