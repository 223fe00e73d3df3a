// Level-wise sparse histogram (xhe_hist_level_sparse): xhe_hist_sparse's design
// with the group g = v * nfeat + f - node v, feature f - in the feature's
// place. Of every group whose feature has a zero bin z_f only the entries
// outside that bin are multiplied, and
//   H[v][f][z_f] = T_v / Q_g mod n^2,  Q_g = prod of g's folded rows other than z_f
// (the hidden bin included), T_v the product of node v's rows.
//
//   order   k_lsp_count, k_sparse_plan (over the groups), k_lsp_scatter: the
//           row ids of the entries kept for g are compacted into g's range of
//           one list, the ranges back to back in group order, and cut into
//           slots of tile_rows ids inside one group. A level has up to 2^18
//           groups, so no block per group: block (x, y) takes kLspBlockRows
//           rows and the features y * fc .. of a chunk of fc, with nnodes * fc
//           LDS counters (lsp_feat_chunk: at most kLspLdsCounters of them). A
//           thread loads the node ids of its rows once and keeps them in
//           registers for the chunk's features - the node array is read once
//           per row and feature chunk, one chunk up to 64 nodes x 64 features
//           - and the block flushes one global atomic per group that has any.
//           The scatter counts again, reserves a range per (block, group) on
//           the group's cursor and places the ids by LDS cursors. A row whose
//           node id is nnodes or more is in no group. The plan is
//           k_sparse_plan's: the bound check and the empty plan past it.
//   tile    k_lsp_tile, one block per slot: hist_tile_block<Hidden> on the
//           slot's ids with nbins + 1 bins and the bins of feature g % nfeat.
//   fold    k_sparse_fold_pass on the slot ranges (it only knows groups), then
//           k_lsp_acc. The slots are group-ordered, so a launch group of gt
//           slots touches the groups tile_node[t0] .. tile_node[t0 + gt - 1]
//           only: the accumulate pass is indexed by slot - the first slot a
//           group has in the launch group takes the group - and not by all
//           nnodes * nfeat * (nbins + 1) accumulator rows as k_sparse_acc is,
//           which a level would walk once per launch group.
//           A group starts its accumulator rows in the launch group that holds
//           its first slot; a group without slots never writes them and
//           k_lsp_out takes the one instead.
//   out     k_lsp_out: the bins other than z_f as words and counts, the kept
//           counts summed per group, the Montgomery one into the columns Q_g
//           leaves out.
//   zero    reduce_segments to Q_g, invert_impl over the nnodes * nfeat rows
//           (the call's one synchronisation), k_lsp_zero stores T_v Q_g^-1 and
//           count_v - kept_g at (v, f, z_f).
#pragma once
#include "hist_sparse_dev.hpp"

namespace xhe {

constexpr int kLspBlockRows = 2048;        // rows per block of the count and the scatter
constexpr int kLspRowsPerThread = kLspBlockRows / 256;
constexpr int kLspLdsCounters = 4096;      // LDS counters of a count block (the scatter takes two words each)

// Features per block of the order kernels
inline int lsp_feat_chunk(int nnodes, int nfeat) {
  const int fc = kLspLdsCounters / nnodes;
  return fc < 1 ? 1 : fc > nfeat ? nfeat : fc;
}

// The block's rows of a thread: ids r0 + tid + 256 i, node id 0xFFFFFFFF where
// the row is past the end or in no node
XHE_DEV void lsp_load_nodes(const uint16_t* __restrict__ node, int64_t n_rows, int nnodes, int64_t r0, int tid,
                            uint32_t (&v)[kLspRowsPerThread]) {
#pragma unroll
  for (int i = 0; i < kLspRowsPerThread; ++i) {
    const int64_t r = r0 + tid + 256 * i;
    const uint32_t id = r < n_rows ? (uint32_t)node[r] : 0xFFFFFFFFu;
    v[i] = id < (uint32_t)nnodes ? id : 0xFFFFFFFFu;
  }
}

// Block (x, y): nnz[v * nfeat + f] += kept entries of node v among rows x *
// kLspBlockRows .. for the features f of chunk y (zeroed before the launch).
// LDS: nnodes * fc counters, counter v * fc + fl.
__global__ void __launch_bounds__(256) k_lsp_count(const uint16_t* __restrict__ bins, int64_t bins_stride, int nfeat,
                                                   int nbins, const uint16_t* __restrict__ zero_bin,
                                                   const uint16_t* __restrict__ node, int64_t n_rows, int nnodes,
                                                   int fc, int32_t* __restrict__ nnz) {
  extern __shared__ uint32_t lsp_lds[];
  const int tid = threadIdx.x;
  const int f0 = blockIdx.y * fc, nf = nfeat - f0 < fc ? nfeat - f0 : fc;
  const int64_t r0 = (int64_t)blockIdx.x * kLspBlockRows;
  for (int i = tid; i < nnodes * fc; i += 256) lsp_lds[i] = 0;
  uint32_t v[kLspRowsPerThread];
  lsp_load_nodes(node, n_rows, nnodes, r0, tid, v);
  __syncthreads();
  for (int fl = 0; fl < nf; ++fl) {
    const uint32_t z = zero_bin[f0 + fl];
    const uint16_t* fb = bins + (size_t)(f0 + fl) * bins_stride;
#pragma unroll
    for (int i = 0; i < kLspRowsPerThread; ++i)
      if (v[i] != 0xFFFFFFFFu && sparse_keep(fb[r0 + tid + 256 * i], z, nbins)) atomicAdd(&lsp_lds[v[i] * fc + fl], 1u);
  }
  __syncthreads();
  for (int i = tid; i < nnodes * fc; i += 256) {
    const uint32_t n = lsp_lds[i];
    const int u = i / fc, fl = i - u * fc;
    if (n) atomicAdd(&nnz[(int64_t)u * nfeat + f0 + fl], (int)n);  // (fl < nf: the others stayed zero)
  }
}

// Block (x, y): list[list_base[g] + ...] = the row ids of the block's entries
// kept for g (cursor: zeroed before the launch). LDS: 2 * nnodes * fc words.
__global__ void __launch_bounds__(256) k_lsp_scatter(const uint16_t* __restrict__ bins, int64_t bins_stride, int nfeat,
                                                     int nbins, const uint16_t* __restrict__ zero_bin,
                                                     const uint16_t* __restrict__ node, int64_t n_rows, int nnodes,
                                                     int fc, const int32_t* __restrict__ list_base,
                                                     int32_t* __restrict__ cursor, const int32_t* __restrict__ flag,
                                                     int32_t* __restrict__ list) {
  if (*flag) return;  // (uniform) past the bound nothing is placed: list holds nnz_bound ids
  extern __shared__ uint32_t lsp_lds[];
  uint32_t* cnt = lsp_lds;             // the block's entries per group, then the cursor inside the block's range
  uint32_t* first = cnt + nnodes * fc;  // where the block's range starts in the group's list
  const int tid = threadIdx.x;
  const int f0 = blockIdx.y * fc, nf = nfeat - f0 < fc ? nfeat - f0 : fc;
  const int64_t r0 = (int64_t)blockIdx.x * kLspBlockRows;
  for (int i = tid; i < nnodes * fc; i += 256) cnt[i] = 0;
  uint32_t v[kLspRowsPerThread];
  lsp_load_nodes(node, n_rows, nnodes, r0, tid, v);
  __syncthreads();
  for (int fl = 0; fl < nf; ++fl) {
    const uint32_t z = zero_bin[f0 + fl];
    const uint16_t* fb = bins + (size_t)(f0 + fl) * bins_stride;
#pragma unroll
    for (int i = 0; i < kLspRowsPerThread; ++i)
      if (v[i] != 0xFFFFFFFFu && sparse_keep(fb[r0 + tid + 256 * i], z, nbins)) atomicAdd(&cnt[v[i] * fc + fl], 1u);
  }
  __syncthreads();
  for (int i = tid; i < nnodes * fc; i += 256) {
    const uint32_t n = cnt[i];
    const int u = i / fc, fl = i - u * fc;
    const int64_t g = (int64_t)u * nfeat + f0 + fl;
    if (n) first[i] = (uint32_t)list_base[g] + (uint32_t)atomicAdd(&cursor[g], (int)n);
    cnt[i] = 0;
  }
  __syncthreads();
  for (int fl = 0; fl < nf; ++fl) {
    const uint32_t z = zero_bin[f0 + fl];
    const uint16_t* fb = bins + (size_t)(f0 + fl) * bins_stride;
#pragma unroll
    for (int i = 0; i < kLspRowsPerThread; ++i) {
      const int64_t r = r0 + tid + 256 * i;
      if (v[i] != 0xFFFFFFFFu && sparse_keep(fb[r], z, nbins)) {
        const uint32_t a = v[i] * fc + fl;
        list[first[a] + atomicAdd(&cnt[a], 1u)] = (int32_t)r;
      }
    }
  }
}

// Block x: slot t0 + x of group g = tile_node[t0 + x]. part: [S4][ncols = gt *
// nb] strided rows, column x * nb + b, nb = nbins + 1. hcnt: [ngroups][nb]
// counts, zeroed before the launch.
template <class MN2, int PW>
__global__ void __launch_bounds__(256, hist_waves<MN2>())
    k_lsp_tile(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ words,
               const uint16_t* __restrict__ bins, int64_t bins_stride, int nfeat, int nb,
               const int32_t* __restrict__ list, const int32_t* __restrict__ nnz, const int32_t* __restrict__ tile_begin,
               const int32_t* __restrict__ list_base, const int32_t* __restrict__ tile_node, int tile_rows, int64_t t0,
               int ncols, uint32_t* __restrict__ part, uint32_t* park, int32_t* __restrict__ hcnt) {
  const int64_t t = t0 + blockIdx.x;
  const int g = tile_node[t];
  if (g < 0) return;  // (uniform: a slot behind the used ones, or the empty plan)
  const int f = g % nfeat;
  const int64_t j = t - tile_begin[g];
  const int64_t left = (int64_t)nnz[g] - j * tile_rows;
  const int m = (int)(left < tile_rows ? left : tile_rows);
  hist_tile_block<MN2, PW, true>(key, Nn2, words, bins + (size_t)f * bins_stride, nb, list,
                                 (int64_t)list_base[g] + j * tile_rows, m, tile_rows, part + (int64_t)blockIdx.x * nb,
                                 1, ncols, park + (size_t)blockIdx.x * (tile_rows / kHistParkDiv) * MN2::S4,
                                 hcnt + (size_t)g * nb);
}

// Lane group (x, c): slot t0 + x where it is the first slot its group g has in
// the launch group [t0, t0 + gt), column c < nb. acc[g * nb + c] is the rows g
// has left in the launch group after `passes` passes, times what acc held
// unless g's first slot lies in this launch group. acc: [S4][nacc].
template <class MN2>
__global__ void __launch_bounds__(256, hist_waves<MN2>())
    k_lsp_acc(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ part, int ncols, int nb,
              int64_t nacc, int64_t t0, int gt, const int32_t* __restrict__ tile_begin,
              const int32_t* __restrict__ tile_node, int passes, uint32_t* acc) {
  const int64_t y = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  if (y >= (int64_t)gt * nb) return;
  const int64_t x = y / nb;
  const int c = (int)(y - x * nb);
  const int g = tile_node[t0 + x];
  if (g < 0) return;  // a slot behind the used ones, or the empty plan
  int lo, hi;
  sparse_range(tile_begin, g, t0, gt, lo, hi);
  if (t0 + x != lo) return;  // (another lane group has g)
  const int len = level_left(hi - lo, passes);
  const bool first = tile_begin[g] >= t0;
  const int64_t col = (int64_t)g * nb + c;
  MN2 M;
  M.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  const uint32_t* r0 = part + x * nb + c;
  if (first) M.load_strided(b, r0, ncols);
  else M.load_strided(b, acc + col, nacc);
#pragma unroll 1
  for (int u = first ? 1 : 0; u < len; ++u) M.mul(b, AStrided{r0 + (int64_t)u * nb, ncols});
  M.reduce_once(b);
  M.store_strided(b, acc + col, nacc);
}

// Lane group (g, c): column c of group g out of Montgomery form to out and cnt
// unless it is the zero bin or the hidden one (a group without slots: the
// one); nzsum[g] += the counts of the columns other than z_f (zeroed before
// the launch); the Montgomery one into the columns Q_g leaves out. With the
// flag raised every column gets the one and nothing else is written.
template <class MN2>
__global__ void __launch_bounds__(256, hist_waves<MN2>())
    k_lsp_out(KeyDev key, const uint32_t* __restrict__ Nn2, uint32_t* acc, int64_t ngroups, int nfeat, int nbins,
              const uint16_t* __restrict__ zero_bin, const int32_t* __restrict__ tile_begin,
              const int32_t* __restrict__ hcnt, const int32_t* __restrict__ flag, uint32_t* __restrict__ out,
              int32_t* __restrict__ cnt, int32_t* __restrict__ nzsum) {
  const int64_t x = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  const int nb = nbins + 1;
  const int64_t nacc = ngroups * nb;
  if (x >= nacc) return;
  const int64_t g = x / nb;
  const int c = (int)(x - g * nb);
  const uint32_t z = zero_bin[g % nfeat];
  const bool over = *flag != 0, sparse = z < (uint32_t)nbins, lane0 = MN2::G::g() == 0;
  const bool empty = over || tile_begin[g + 1] == tile_begin[g];  // acc was never written
  MN2 M;
  M.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  if (!over && c < nbins && !(sparse && (uint32_t)c == z)) {
    if (empty) M.load_row(b, n2dev<MN2>(key).R1);
    else M.load_strided(b, acc + x, nacc);
    M.mul(b, AOne{});
    M.reduce_once(b);
    M.store_words(b, out + ((size_t)g * nbins + c) * key.n2w, key.n2w);
    if (cnt && lane0) cnt[(size_t)g * nbins + c] = hcnt[x];
  }
  if (!over && sparse && (uint32_t)c != z && lane0) {
    const int32_t h = hcnt[x];
    if (h) atomicAdd(&nzsum[g], h);
  }
  if (empty || !sparse || (uint32_t)c == z) {
    M.load_row(b, n2dev<MN2>(key).R1);
    M.reduce_once(b);
    M.store_strided(b, acc + x, nacc);
  }
}

// Lane group g = v * nfeat + f: out[v][f][z_f] = total[v] * inv[g] mod n^2
// (inv[g] = Q_g^-1 as words, total[v] any value its words hold), cnt[v][f][z_f]
// = node_cnt[v] - nzsum[g].
template <class MN2, int PW>
__global__ void __launch_bounds__(256, hist_waves<MN2>())
    k_lsp_zero(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ inv,
               const uint32_t* __restrict__ total, int64_t ngroups, int nfeat, int nbins,
               const uint16_t* __restrict__ zero_bin, const int32_t* __restrict__ node_cnt,
               const int32_t* __restrict__ nzsum, uint32_t* __restrict__ out, int32_t* __restrict__ cnt) {
  const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  if (g >= ngroups) return;
  const int64_t v = g / nfeat;
  const uint32_t z = zero_bin[g - v * nfeat];
  if (z >= (uint32_t)nbins) return;
  MN2 M;
  M.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  M.load_words(b, inv + (size_t)g * PW, PW);
  M.mul(b, ARowPacked<MN2::W, PW>{total + (size_t)v * PW});    // inv T / R
  M.mul(b, ARow{n2dev<MN2>(key).Rpow + (size_t)2 * MN2::S4});  // times R^2 / R
  M.reduce_once(b);
  M.store_words(b, out + ((size_t)g * nbins + z) * key.n2w, key.n2w);
  if (cnt && MN2::G::g() == 0) cnt[(size_t)g * nbins + z] = node_cnt[v] - nzsum[g];
}

}  // namespace xhe
