// Level-wise ciphertext histogram (xhe_hist_level): every (node, feature, bin)
// product of a tree level from one pass over the level's rows.
//
//   order   k_level_count, k_level_plan, k_level_scatter: the row ids are
//           ordered by node into tile slots of tile_rows ids, every slot
//           inside one node. Ciphertext rows do not move. The node counts are
//           taken in per-block LDS counters and flushed with one global atomic
//           per (block, node); one block turns them into tile_begin (the
//           exclusive prefix of ceil(count / tile) over the nodes) and
//           tile_node (the node of every slot, -1 behind the used ones); the
//           scatter counts its block's rows again, reserves a range per
//           (block, node) with one global atomic and places the ids by LDS
//           cursors. The order inside a node is the atomics': the product is
//           commutative and every output the canonical residue, so the
//           outputs are the same bits whatever it is.
//           A node's ids are contiguous from its first slot, so slot j of a
//           node holds min(tile, count - j tile) of them: stage A takes that
//           number from the counts, and the padding behind a node's last id
//           is never written and never read.
//   stage A k_level_tile, one block per (slot, feature): hist_tile_block
//           (hist_dev.hpp) with `order` as its row ids. A slot lies inside
//           one node, so LDS holds nbins counters as in k_hist_tile. The
//           partial rows are slot-major - column t * (gf nbins) + fl nbins +
//           b of [S4][gf nbins Tmax] - so that a block's lane groups write
//           neighbouring columns and the fold's read neighbouring columns.
//   stage B k_level_fold: one lane group per (node, feature, bin) multiplies
//           the node's slots, leaves Montgomery form and packs the words; a
//           node without rows gives 1. With the planner's tile most nodes are
//           one slot and this is a copy. A node with more than kRawChunk
//           slots is first folded in place by k_level_fold_pass (chunk j of
//           nch reads slots j, j + nch, ... and writes slot j, which no other
//           chunk reads) until kRawChunk or fewer are left: no lane group
//           walks more than kRawChunk dependent products. The host knows the
//           number of passes from ceil(n_rows / tile) alone; a pass's lane
//           groups are indexed by slot and return at once where nothing is
//           left to fold.
#pragma once
#include "hist_dev.hpp"

namespace xhe {

constexpr int kLevelBlockRows = 4096;  // rows per block of the count and the scatter

// node_cnt[v] += rows of the block with node id v (zeroed before the launch).
// LDS: nnodes counters.
__global__ void __launch_bounds__(256) k_level_count(const uint16_t* __restrict__ node, int64_t n_rows, int nnodes,
                                                     int32_t* __restrict__ node_cnt) {
  extern __shared__ uint32_t level_lds[];
  const int tid = threadIdx.x;
  for (int v = tid; v < nnodes; v += 256) level_lds[v] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kLevelBlockRows;
  const int64_t r1 = r0 + kLevelBlockRows < n_rows ? r0 + kLevelBlockRows : n_rows;
  for (int64_t r = r0 + tid; r < r1; r += 256) {
    const uint32_t v = node[r];
    if (v < (uint32_t)nnodes) atomicAdd(&level_lds[v], 1u);
  }
  __syncthreads();
  for (int v = tid; v < nnodes; v += 256) {
    const uint32_t n = level_lds[v];
    if (n) atomicAdd(&node_cnt[v], (int)n);
  }
}

// One block: tile_begin[v] = sum over u < v of ceil(node_cnt[u] / tile_rows)
// (nnodes + 1 entries), tile_node[t] for t < tmax. LDS: nnodes + 1 words.
__global__ void __launch_bounds__(256) k_level_plan(const int32_t* __restrict__ node_cnt, int nnodes, int tile_rows,
                                                    int64_t tmax, int32_t* __restrict__ tile_begin,
                                                    int32_t* __restrict__ tile_node) {
  extern __shared__ uint32_t level_lds[];
  int32_t* tb = reinterpret_cast<int32_t*>(level_lds);
  __shared__ int32_t s_part[256];
  const int tid = threadIdx.x;
  const int per = (nnodes + 255) / 256;
  const int lo = tid * per < nnodes ? tid * per : nnodes, hi = lo + per < nnodes ? lo + per : nnodes;
  auto tiles = [&](int v) { return (node_cnt[v] + tile_rows - 1) / tile_rows; };
  int32_t sum = 0;
  for (int v = lo; v < hi; ++v) sum += tiles(v);
  s_part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int32_t run = 0;
    for (int i = 0; i < 256; ++i) {
      const int32_t n = s_part[i];
      s_part[i] = run;
      run += n;
    }
    tb[nnodes] = run;
  }
  __syncthreads();
  int32_t run = s_part[tid];
  for (int v = lo; v < hi; ++v) {
    tb[v] = run;
    run += tiles(v);
  }
  __syncthreads();
  for (int v = tid; v <= nnodes; v += 256) tile_begin[v] = tb[v];
  const int32_t total = tb[nnodes];
  for (int64_t t = tid; t < tmax; t += 256) {
    int32_t v = -1;
    if (t < total) {  // the node whose slots hold t: the first i with tb[i] > t, less one
      int a = 0, b = nnodes;
      while (a < b) {
        const int mid = (a + b) / 2;
        if (tb[mid] > t) b = mid;
        else a = mid + 1;
      }
      v = a - 1;
    }
    tile_node[t] = v;
  }
}

// order[tile_begin[v] * tile_rows + i] = the i-th row id of node v (cursor:
// zeroed before the launch). LDS: 2 nnodes words.
__global__ void __launch_bounds__(256) k_level_scatter(const uint16_t* __restrict__ node, int64_t n_rows, int nnodes,
                                                       int tile_rows, const int32_t* __restrict__ tile_begin,
                                                       int32_t* __restrict__ cursor, int32_t* __restrict__ order) {
  extern __shared__ uint32_t level_lds[];
  uint32_t* cnt = level_lds;       // the block's rows per node, then the cursor inside the block's range
  uint32_t* first = cnt + nnodes;  // the block's range in the node's ids
  const int tid = threadIdx.x;
  for (int v = tid; v < nnodes; v += 256) cnt[v] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kLevelBlockRows;
  const int64_t r1 = r0 + kLevelBlockRows < n_rows ? r0 + kLevelBlockRows : n_rows;
  for (int64_t r = r0 + tid; r < r1; r += 256) {
    const uint32_t v = node[r];
    if (v < (uint32_t)nnodes) atomicAdd(&cnt[v], 1u);
  }
  __syncthreads();
  for (int v = tid; v < nnodes; v += 256) {
    const uint32_t n = cnt[v];
    if (n) first[v] = (uint32_t)atomicAdd(&cursor[v], (int)n);
    cnt[v] = 0;
  }
  __syncthreads();
  for (int64_t r = r0 + tid; r < r1; r += 256) {
    const uint32_t v = node[r];
    if (v < (uint32_t)nnodes)
      order[(int64_t)tile_begin[v] * tile_rows + first[v] + atomicAdd(&cnt[v], 1u)] = (int32_t)r;
  }
}

// Block x = t * gf + fl: slot t of feature f0 + fl. part: [S4][ncols = gf *
// nbins * tmax] strided rows, column t * (gf nbins) + fl nbins + b. cnt_out:
// [nnodes][nfeat][nbins], zeroed before the launch, or null.
template <class MN2, int PW>
__global__ void __launch_bounds__(256, hist_waves<MN2>())
    k_level_tile(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ words,
                 const uint16_t* __restrict__ bins, int64_t bins_stride, int nbins, const int32_t* __restrict__ order,
                 const int32_t* __restrict__ node_cnt, const int32_t* __restrict__ tile_begin,
                 const int32_t* __restrict__ tile_node, int tile_rows, int f0, int gf, int nfeat, int ncols,
                 uint32_t* __restrict__ part, uint32_t* park, int32_t* __restrict__ cnt_out) {
  const int64_t t = blockIdx.x / gf;
  const int fl = (int)(blockIdx.x - t * gf);
  const int v = tile_node[t];
  if (v < 0) return;  // (uniform: a slot behind the used ones)
  const int64_t left = (int64_t)node_cnt[v] - (t - tile_begin[v]) * tile_rows;
  const int m = (int)(left < tile_rows ? left : tile_rows);
  hist_tile_block<MN2, PW>(key, Nn2, words, bins + (size_t)(f0 + fl) * bins_stride, nbins, order, t * tile_rows, m,
                           tile_rows, part + (t * gf + fl) * nbins, 1, ncols,
                           park + (size_t)blockIdx.x * (tile_rows / kHistParkDiv) * MN2::S4,
                           cnt_out ? cnt_out + ((size_t)v * nfeat + f0 + fl) * nbins : nullptr);
}

// Partial rows of a node still to fold after `passes` passes over `len` slots
XHE_DEV int level_left(int len, int passes) {
  for (int p = 0; p < passes; ++p) len = len > kRawChunk ? (len + kRawChunk - 1) / kRawChunk : len;
  return len;
}

// Pass `pass` over the nodes with more than kRawChunk rows left. Lane group
// (t, c): column c < gn = gf * nbins of slot t, chunk j = t - tile_begin[v] of
// its node; in place.
template <class MN2>
__global__ void __launch_bounds__(256, hist_waves<MN2>()) k_level_fold_pass(KeyDev key, const uint32_t* __restrict__ Nn2,
                                                            uint32_t* part, int ncols, int gn, int64_t tmax,
                                                            const int32_t* __restrict__ tile_begin,
                                                            const int32_t* __restrict__ tile_node, int pass) {
  const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  if (g >= tmax * gn) return;
  const int64_t t = g / gn;
  const int c = (int)(g - t * gn);
  const int v = tile_node[t];
  if (v < 0) return;
  const int lo = tile_begin[v], j = (int)t - lo;
  const int len = level_left(tile_begin[v + 1] - lo, pass);
  if (len <= kRawChunk) return;
  const int nch = (len + kRawChunk - 1) / kRawChunk;
  if (j >= nch) return;
  const int cnt = (len - j + nch - 1) / nch;
  MN2 M;
  M.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  uint32_t* r0 = part + (int64_t)(lo + j) * gn + c;
  M.load_strided(b, r0, ncols);
#pragma unroll 1
  for (int u = 1; u < cnt; ++u) M.mul(b, AStrided{r0 + (int64_t)u * nch * gn, ncols});
  M.reduce_once(b);
  M.store_strided(b, r0, ncols);
}

// Lane group (v, c): the product of node v's rows left after `passes` passes
// in column c = fl * nbins + b, out of Montgomery form, as words at
// out[((v * nfeat + f0 + fl) * nbins + b) * n2w].
template <class MN2>
__global__ void __launch_bounds__(256, hist_waves<MN2>()) k_level_fold(KeyDev key, const uint32_t* __restrict__ Nn2,
                                                       const uint32_t* __restrict__ part, int ncols, int gn, int nbins,
                                                       int nnodes, int f0, int nfeat,
                                                       const int32_t* __restrict__ tile_begin, int passes,
                                                       uint32_t* __restrict__ out) {
  const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  if (g >= (int64_t)nnodes * gn) return;
  const int v = (int)(g / gn), c = (int)(g - (int64_t)v * gn);
  const int fl = c / nbins, bin = c - fl * nbins;
  const int lo = tile_begin[v];
  const int len = level_left(tile_begin[v + 1] - lo, passes);
  MN2 M;
  M.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  if (len == 0) {  // a node without rows: Montgomery one
    M.load_row(b, n2dev<MN2>(key).R1);
    M.reduce_once(b);
  } else {
    const uint32_t* r0 = part + (int64_t)lo * gn + c;
    M.load_strided(b, r0, ncols);
#pragma unroll 1
    for (int u = 1; u < len; ++u) M.mul(b, AStrided{r0 + (int64_t)u * gn, ncols});
  }
  M.mul(b, AOne{});
  M.reduce_once(b);
  M.store_words(b, out + (((size_t)v * nfeat + f0 + fl) * nbins + bin) * key.n2w, key.n2w);
}

}  // namespace xhe
