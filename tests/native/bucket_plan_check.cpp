// The bucket planner of xfl_amd/csrc/paths.hpp (bucket_window, bucket_cost,
// multiexp_route) against its header's formula and the routes the shapes in
// use must keep. Host-only, its own main; tests/test_bucket_plan.py builds it
// with -fsanitize=address,undefined and runs it. Exit status 0 = every check
// held; a failed check prints its line.
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

// cost(c) = nwin (nterms + nbins T) + nwin 2 2^c with the tile count spelled out
static double formula(int64_t nterms, int nwin, int nbins, int64_t T, int c) {
  return (double)nwin * ((double)nterms + (double)nbins * (double)T) + (double)nwin * 2.0 * (double)(1 << c);
}

int main() {
  const int s4 = 152;  // the 2048-bit batch shape's row
  for (int64_t nterms : {(int64_t)1, (int64_t)63, (int64_t)300, (int64_t)8192, (int64_t)1000000, (int64_t)100000000})
    for (int64_t ncols : {(int64_t)1, (int64_t)16, (int64_t)4096})
      for (int kbits : {1, 24, 70, 2048})
        for (int sgn = 0; sgn < 2; ++sgn) {
          const int c = bucket_window(nterms, ncols, kbits, sgn != 0);
          CHECK(c >= 1 && c <= kBucketWinMax);
          CHECK(bucket_nbins(c, sgn != 0) <= 4094);
        }
  CHECK(bucket_nbins(11, true) == 4094 && bucket_nbins(11, false) == 2047 && bucket_nbins(1, true) == 2);
  // the LR step stays on Straus, the Pearson shape goes to buckets
  CHECK(multiexp_route(2048, 15, 60, 2048, s4) == MexpRoute::STRAUS);
  CHECK(multiexp_route(2048, 15, 60, 0, s4) == MexpRoute::STRAUS);
  CHECK(multiexp_route(1000000, 16, 24, 1000000, s4) == MexpRoute::BUCKETS);
  CHECK(multiexp_route(kBucketMinTerms - 1, 16, 24, kBucketMinTerms - 1, s4) == MexpRoute::STRAUS);
  // three shapes by hand. 1 M x 16 x 24 bits signed, c = 8: 3 windows, 510
  // bins, 48 features: the tile stays 8192 (48 x 123 blocks fill the chip)
  CHECK(hist_tile(1000000, 48, 510) == 8192);
  CHECK(bucket_cost(1000000, 16, 24, true, 8) == formula(1000000, 3, 510, 123, 8));
  // 300 x 3 x 24 bits unsigned, c = 3: 8 windows, 7 bins, 24 features: tile 64, 5 tiles
  CHECK(hist_tile(300, 24, 7) == 64);
  CHECK(bucket_cost(300, 3, 24, false, 3) == formula(300, 8, 7, 5, 3));
  // 100 k x 16 x 24 bits signed, c = 6: 4 windows, 126 bins, 64 features:
  // 32 x 126 rounds up to 4096, and 64 x 25 blocks fill the chip
  CHECK(hist_tile(100000, 64, 126) == 4096);
  CHECK(bucket_cost(100000, 16, 24, true, 6) == formula(100000, 4, 126, 25, 6));
  if (!failed) printf("ok kBucketMinTerms=%lld\n", (long long)kBucketMinTerms);
  return failed ? 1 : 0;
}
