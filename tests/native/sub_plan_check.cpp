// The histogram-subtraction planner of xfl_amd/csrc/paths.hpp (level_sub,
// sib_chunk). Host-only, its own main; tests/test_sub_plan.py builds it with
// -fsanitize=address,undefined and runs it. Exit status 0 = every check held;
// a failed check prints its line.
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
  // monotone in n_rows: once the route subtracts it keeps subtracting (odd and even counts alike)
  for (int nodes : {2, 4, 64, 4096})
    for (int nbins : {1, 3, 256, 4096})
      for (int nfeat : {1, 64}) {
        bool on = false;
        for (int64_t n = 0; n < 3000; ++n) {
          const bool now = level_sub(n, nodes, nfeat, nbins);
          CHECK(now || !on);
          on = now;
        }
        for (int64_t n = 4096; n <= ((int64_t)1 << 40); n <<= 1) {
          const bool now = level_sub(n, nodes, nfeat, nbins);
          CHECK(now || !on);
          on = now;
        }
        CHECK(on);  // enough rows always pay
      }
  for (int64_t n : {(int64_t)0, (int64_t)100, (int64_t)1 << 40})
    for (int nodes : {-2, 0, 1, 3, 65}) CHECK(!level_sub(n, nodes, 64, 256));
  CHECK(kSubMinSaving > 1.0 && kSubMinSaving < 2.0);  // (2 is the model's limit: no shape would subtract)
  // config 5 (100 k x 64 x 256): two nodes subtract, 1024 do not
  CHECK(level_sub(100000, 2, 64, 256) && !level_sub(100000, 1024, 64, 256));
  for (int64_t M : {(int64_t)1, (int64_t)3, (int64_t)4, (int64_t)5, (int64_t)16384, (int64_t)131071, (int64_t)131072,
                    (int64_t)524288, (int64_t)1 << 20, (int64_t)1 << 31, (int64_t)1 << 40}) {
    const int c = sib_chunk(M);
    CHECK(c >= kSibChunkMin && c <= kSibChunkMax);
    const int64_t nchunks = (M + c - 1) / c;
    CHECK(nchunks >= 1 && nchunks <= M && nchunks * c >= M);  // every chunk holds a row, the chunks cover M
    CHECK((M + nchunks - 1) / nchunks <= c);                  // the longest interleaved chunk
  }
  CHECK(sib_chunk(1) == kSibChunkMin && sib_chunk((int64_t)1 << 40) == kSibChunkMax);
  if (!failed) printf("ok\n");
  return failed ? 1 : 0;
}
