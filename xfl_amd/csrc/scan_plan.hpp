// The plan of a segmented inclusive scan (xhe_segscan): every chunk of every
// level as (first row, length, total column, carry column). Host-only and
// pure - standard headers, no HIP call - so it runs, and is tested
// (tests/test_scan_plan.py), on any machine. xhe.hip uploads Plan::chunks in
// one copy and launches k_segscan_chunk / k_segscan_apply per level.
//
// Level 0 holds the call's elements, cut per segment into chunks of at most C
// consecutive rows; a chunk never crosses a segment boundary and an empty
// segment has no chunk. The totals of the chunks of every segment that has
// more than one chunk are the rows of the next level, one segment per such
// segment, in order; a segment of one chunk is finished at its level and
// sends nothing up. The levels end when no segment has a second chunk.
//
// A chunk's carry is what its rows are still missing after the chunk pass:
// the inclusive total of the chunks before it in its segment. That is the
// scanned row of the previous chunk one level up, so
//   total column = the chunk's row in the next level (-1: one-chunk segment),
//   carry column = total column - 1 (-1: the segment's first chunk).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace xhe {
namespace scan {

// The chunk length is fixed and short. A chunk is a chain of dependent
// products, so its length is the latency of a level; 16 keeps three levels
// within 4,097 rows (every level count a test can reach in seconds) and
// spends 1/16 + 1/256 + ... of the element count on the upper levels. Longer
// chunks would save at most that share. Bounded by the fix-up rows the keys
// hold: R^j for j <= kRawChunk + 1 = 33, and row u of a chunk needs R^(u+2).
constexpr int64_t kChunkLen = 16;

inline int64_t chunk_len(int64_t /*count*/) { return kChunkLen; }

constexpr int kFields = 4;  // int64 per chunk: first, len, total, carry
enum Field { FIRST = 0, LEN = 1, TOTAL = 2, CARRY = 3 };

struct Level {
  int64_t rows;         // rows of this level (level 0: the element count)
  int64_t chunk0;       // index of its first chunk in Plan::chunks (in chunks, not words)
  int64_t nchunks;
};

struct Plan {
  std::vector<int64_t> chunks;  // kFields per chunk, the levels back to back
  std::vector<Level> levels;    // empty when there is no row at all
};

// seg: nseg + 1 non-decreasing offsets, seg[0] == 0 (checked by the caller).
inline Plan make_plan(const int64_t* seg, int64_t nseg, int64_t C) {
  Plan p;
  std::vector<int64_t> cur(seg, seg + nseg + 1), nxt;
  while (cur.back() > 0) {
    Level lv{cur.back(), (int64_t)(p.chunks.size() / kFields), 0};
    nxt.assign(1, 0);
    for (size_t s = 0; s + 1 < cur.size(); ++s) {
      const int64_t len = cur[s + 1] - cur[s];
      const int64_t nch = (len + C - 1) / C;
      for (int64_t t = 0; t < nch; ++t) {
        const int64_t total = nch > 1 ? nxt.back() + t : -1;
        p.chunks.push_back(cur[s] + t * C);
        p.chunks.push_back(t + 1 < nch ? C : len - t * C);
        p.chunks.push_back(total);
        p.chunks.push_back(t > 0 ? total - 1 : -1);
      }
      lv.nchunks += nch;
      if (nch > 1) nxt.push_back(nxt.back() + nch);
    }
    p.levels.push_back(lv);
    cur.swap(nxt);
  }
  return p;
}

}  // namespace scan
}  // namespace xhe
