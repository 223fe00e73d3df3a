// Sparse-aware ciphertext histogram (xhe_hist_sparse): of every feature f
// with a zero bin z_f only the entries outside that bin are multiplied; the
// zero bin is what is left of the product T of all the call's elements,
//   H_f[z_f] = T / Q_f mod n^2,  Q_f = prod of f's folded rows other than z_f,
// the hidden bin included (bin nbins of the nbins + 1 internal ones: the
// entries with an id >= nbins, which xhe_hist drops but T holds).
//
//   order   k_sparse_count, k_sparse_plan, k_sparse_scatter: the row ids of
//           the entries kept for f (id != z_f; every entry of a dense feature,
//           z_f >= nbins) are compacted into f's range of one list, the ranges
//           back to back in feature order, and cut into slots of tile_rows ids
//           that each lie inside one feature. One block per (4096 elements,
//           feature) counts in LDS and adds once into nnz[f]; one block turns
//           the counts into tile_begin (the exclusive prefix of ceil(nnz /
//           tile) over the features), list_base (the prefix of nnz) and
//           tile_node (the feature of every slot, -1 behind the used ones),
//           and compares the sum with the caller's bound, which sized the list
//           and the slot table: past it the flag is raised and the plan is
//           the empty one, so that nothing below indexes by a count the bound
//           does not cover. The scatter counts its block again, reserves a
//           range with one atomic on the feature's cursor and places the ids
//           by an LDS cursor. The order inside a feature is the atomics'.
//   tile    k_sparse_tile, one block per slot: hist_tile_block<Hidden> on the
//           slot's ids with nbins + 1 bins. At 5 % density a slot still holds
//           tile_rows entries of one feature: the lane groups are as full as
//           the dense call's. Partial rows slot-major, column tl (nbins + 1) +
//           b of the slot group's [S4][gt (nbins + 1)].
//   fold    k_sparse_fold_pass (k_level_fold_pass with the feature in the
//           node's place and the slot range cut to the launch group), then
//           k_sparse_acc multiplies what is left into the call's accumulator
//           row of (f, b) - the slots run in launch groups under the launch
//           layer's row cap, and a feature's slots may span two of them - and
//           k_sparse_out writes the bins other than z_f as words with their
//           counts, adds those counts up per feature and puts the Montgomery
//           one into column z_f (every column of a dense feature), so that the
//           product of a feature's nbins + 1 columns is Q_f (1 when dense).
//   zero    the launch layer reduces the columns to Q_f (reduce_segments:
//           chunks of at most kRawChunk, further levels for the chunk totals)
//           and inverts the nfeat rows in one batch (invert_impl: the call's
//           one synchronisation); k_sparse_zero stores T Q_f^-1 and count -
//           (the other bins' counts) at (f, z_f).
#pragma once
#include "hist_level_dev.hpp"

namespace xhe {

constexpr int kSparseBlockElems = 4096;  // elements per block of the count and the scatter

// Whether an entry with this id is multiplied for a feature with zero bin z
XHE_DEV bool sparse_keep(uint32_t id, uint32_t z, int nbins) { return z >= (uint32_t)nbins || id != z; }

// Block (x, f): nnz[f] += kept entries among elements x * 4096 .. (zeroed before the launch)
__global__ void __launch_bounds__(256) k_sparse_count(const uint16_t* __restrict__ bins, int64_t bins_stride, int nbins,
                                                      const uint16_t* __restrict__ zero_bin,
                                                      const int32_t* __restrict__ rows_idx, int64_t count,
                                                      int32_t* __restrict__ nnz) {
  __shared__ uint32_t s_n;
  const int tid = threadIdx.x, f = blockIdx.y;
  const uint32_t z = zero_bin[f];
  const int64_t i0 = (int64_t)blockIdx.x * kSparseBlockElems;
  const int64_t i1 = i0 + kSparseBlockElems < count ? i0 + kSparseBlockElems : count;
  if (z >= (uint32_t)nbins) {  // (uniform) a dense feature keeps everything
    if (tid == 0) atomicAdd(&nnz[f], (int)(i1 - i0));
    return;
  }
  if (tid == 0) s_n = 0;
  __syncthreads();
  const uint16_t* fb = bins + (size_t)f * bins_stride;
  uint32_t n = 0;
  for (int64_t i = i0 + tid; i < i1; i += 256) n += fb[rows_idx ? (int64_t)rows_idx[i] : i] != z ? 1u : 0u;
  if (n) atomicAdd(&s_n, n);
  __syncthreads();
  if (tid == 0 && s_n) atomicAdd(&nnz[f], (int)s_n);
}

// One block. tile_begin: nfeat + 1 entries, list_base: nfeat, tile_node: tmax.
// *flag = 1 and the empty plan when the counts add up to more than nnz_bound.
__global__ void __launch_bounds__(256) k_sparse_plan(const int32_t* __restrict__ nnz, int nfeat, int tile_rows,
                                                     int64_t nnz_bound, int64_t tmax, int32_t* tile_begin,
                                                     int32_t* __restrict__ list_base, int32_t* __restrict__ tile_node,
                                                     int32_t* __restrict__ flag) {
  __shared__ int64_t s_n[256];
  __shared__ int32_t s_t[256];
  __shared__ int s_over;
  const int tid = threadIdx.x;
  const int per = (nfeat + 255) / 256;
  const int lo = tid * per < nfeat ? tid * per : nfeat, hi = lo + per < nfeat ? lo + per : nfeat;
  auto tiles = [&](int f) { return (nnz[f] + tile_rows - 1) / tile_rows; };
  int64_t n = 0;
  int32_t t = 0;
  for (int f = lo; f < hi; ++f) {
    n += nnz[f];
    t += tiles(f);
  }
  s_n[tid] = n;
  s_t[tid] = t;
  __syncthreads();
  if (tid == 0) {
    int64_t rn = 0;
    int32_t rt = 0;
    for (int i = 0; i < 256; ++i) {
      const int64_t a = s_n[i];
      const int32_t b = s_t[i];
      s_n[i] = rn;
      s_t[i] = rt;
      rn += a;
      rt += b;
    }
    s_over = rn > nnz_bound || rt > tmax ? 1 : 0;  // (rt <= nnz_bound / tile + nfeat follows from the first)
    *flag = s_over;
    tile_begin[nfeat] = s_over ? 0 : rt;
  }
  __syncthreads();
  const bool over = s_over != 0;
  n = s_n[tid];
  t = s_t[tid];
  for (int f = lo; f < hi; ++f) {
    tile_begin[f] = over ? 0 : t;
    list_base[f] = over ? 0 : (int32_t)n;
    n += nnz[f];
    t += tiles(f);
  }
  __syncthreads();  // (tile_begin is read back below: written by this block, visible after the barrier)
  const int32_t total = tile_begin[nfeat];
  for (int64_t s = tid; s < tmax; s += 256) {
    int32_t f = -1;
    if (s < total) {  // the feature whose slots hold s: the first i with tile_begin[i] > s, less one
      int a = 0, b = nfeat;
      while (a < b) {
        const int mid = (a + b) / 2;
        if (tile_begin[mid] > s) b = mid;
        else a = mid + 1;
      }
      f = a - 1;
    }
    tile_node[s] = f;
  }
}

// Block (x, f): list[list_base[f] + ...] = the row ids of the block's kept
// entries (cursor: zeroed before the launch).
__global__ void __launch_bounds__(256) k_sparse_scatter(const uint16_t* __restrict__ bins, int64_t bins_stride,
                                                        int nbins, const uint16_t* __restrict__ zero_bin,
                                                        const int32_t* __restrict__ rows_idx, int64_t count,
                                                        const int32_t* __restrict__ list_base,
                                                        int32_t* __restrict__ cursor, const int32_t* __restrict__ flag,
                                                        int32_t* __restrict__ list) {
  if (*flag) return;
  __shared__ uint32_t s_n, s_first;
  const int tid = threadIdx.x, f = blockIdx.y;
  const uint32_t z = zero_bin[f];
  const int64_t i0 = (int64_t)blockIdx.x * kSparseBlockElems;
  const int64_t i1 = i0 + kSparseBlockElems < count ? i0 + kSparseBlockElems : count;
  const uint16_t* fb = bins + (size_t)f * bins_stride;
  auto row_of = [&](int64_t i) -> int64_t { return rows_idx ? (int64_t)rows_idx[i] : i; };
  const bool dense = z >= (uint32_t)nbins;
  if (tid == 0) s_n = 0;
  __syncthreads();
  uint32_t n = 0;
  if (!dense)
    for (int64_t i = i0 + tid; i < i1; i += 256) n += fb[row_of(i)] != z ? 1u : 0u;
  if (n) atomicAdd(&s_n, n);
  __syncthreads();
  if (tid == 0) {
    const uint32_t mine = dense ? (uint32_t)(i1 - i0) : s_n;
    s_first = mine ? (uint32_t)atomicAdd(&cursor[f], (int)mine) : 0u;
    s_n = 0;
  }
  __syncthreads();
  int32_t* dst = list + (int64_t)list_base[f] + s_first;
  for (int64_t i = i0 + tid; i < i1; i += 256) {
    const int64_t r = row_of(i);
    if (dense) dst[i - i0] = (int32_t)r;
    else if (fb[r] != z) dst[atomicAdd(&s_n, 1u)] = (int32_t)r;
  }
}

// Block x: slot t0 + x. part: [S4][ncols = gt * nb] strided rows, column x *
// nb + b, nb = nbins + 1. hcnt: [nfeat][nb] counts, zeroed before the launch.
template <class MN2, int PW>
__global__ void __launch_bounds__(256, hist_waves<MN2>())
    k_sparse_tile(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ words,
                  const uint16_t* __restrict__ bins, int64_t bins_stride, int nb, const int32_t* __restrict__ list,
                  const int32_t* __restrict__ nnz, const int32_t* __restrict__ tile_begin,
                  const int32_t* __restrict__ list_base, const int32_t* __restrict__ tile_node, int tile_rows,
                  int64_t t0, int ncols, uint32_t* __restrict__ part, uint32_t* park, int32_t* __restrict__ hcnt) {
  const int64_t t = t0 + blockIdx.x;
  const int f = tile_node[t];
  if (f < 0) return;  // (uniform: a slot behind the used ones, or the empty plan)
  const int64_t j = t - tile_begin[f];
  const int64_t left = (int64_t)nnz[f] - j * tile_rows;
  const int m = (int)(left < tile_rows ? left : tile_rows);
  hist_tile_block<MN2, PW, true>(key, Nn2, words, bins + (size_t)f * bins_stride, nb, list,
                                 (int64_t)list_base[f] + j * tile_rows, m, tile_rows, part + (int64_t)blockIdx.x * nb,
                                 1, ncols, park + (size_t)blockIdx.x * (tile_rows / kHistParkDiv) * MN2::S4,
                                 hcnt + (size_t)f * nb);
}

// The slots of feature f inside the launch group [t0, t0 + gt)
XHE_DEV void sparse_range(const int32_t* __restrict__ tile_begin, int f, int64_t t0, int gt, int& lo, int& hi) {
  const int64_t a = tile_begin[f], b = tile_begin[f + 1];
  lo = (int)(a > t0 ? a : t0);
  hi = (int)(b < t0 + gt ? b : t0 + gt);
}

// Pass `pass` over the features with more than kRawChunk rows left in the
// group. Lane group (x, c): column c < nb of slot t0 + x, chunk j of its
// feature's range; in place.
template <class MN2>
__global__ void __launch_bounds__(256, hist_waves<MN2>())
    k_sparse_fold_pass(KeyDev key, const uint32_t* __restrict__ Nn2, uint32_t* part, int ncols, int nb, int64_t t0,
                       int gt, const int32_t* __restrict__ tile_begin, const int32_t* __restrict__ tile_node,
                       const int32_t* __restrict__ flag, int pass) {
  const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  if (g >= (int64_t)gt * nb || *flag) return;
  const int64_t x = g / nb;
  const int c = (int)(g - x * nb);
  const int f = tile_node[t0 + x];
  if (f < 0) return;
  int lo, hi;
  sparse_range(tile_begin, f, t0, gt, lo, hi);
  const int j = (int)(t0 + x) - lo;
  const int len = level_left(hi - lo, pass);
  if (len <= kRawChunk) return;
  const int nch = (len + kRawChunk - 1) / kRawChunk;
  if (j >= nch) return;
  const int cnt = (len - j + nch - 1) / nch;
  MN2 M;
  M.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  uint32_t* r0 = part + (int64_t)(lo - t0 + j) * nb + c;
  M.load_strided(b, r0, ncols);
#pragma unroll 1
  for (int u = 1; u < cnt; ++u) M.mul(b, AStrided{r0 + (int64_t)u * nch * nb, ncols});
  M.reduce_once(b);
  M.store_strided(b, r0, ncols);
}

// Lane group (f, c): acc[f * nb + c] (times, unless `first`) the rows feature
// f has left in the group after `passes` passes. acc: [S4][nfeat * nb].
template <class MN2>
__global__ void __launch_bounds__(256, hist_waves<MN2>())
    k_sparse_acc(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ part, int ncols, int nb,
                 int nfeat, int64_t t0, int gt, const int32_t* __restrict__ tile_begin,
                 const int32_t* __restrict__ flag, int passes, int first, uint32_t* acc) {
  const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  const int nacc = nfeat * nb;
  if (g >= nacc || *flag) return;
  const int f = (int)(g / nb), c = (int)(g - (int64_t)f * nb);
  int lo, hi;
  sparse_range(tile_begin, f, t0, gt, lo, hi);
  const int len = hi > lo ? level_left(hi - lo, passes) : 0;
  if (len == 0 && !first) return;
  MN2 M;
  M.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  if (first) M.load_row(b, n2dev<MN2>(key).R1);  // the Montgomery one
  else M.load_strided(b, acc + g, nacc);
  const uint32_t* r0 = part + (int64_t)(lo - t0) * nb + c;
#pragma unroll 1
  for (int u = 0; u < len; ++u) M.mul(b, AStrided{r0 + (int64_t)u * nb, ncols});
  M.reduce_once(b);
  M.store_strided(b, acc + g, nacc);
}

// Lane group (f, c): column c of feature f out of Montgomery form to out and
// cnt unless it is the zero bin or the hidden one; nzsum[f] += the counts of
// the columns other than z_f (zeroed before the launch); the Montgomery one
// into the columns Q_f leaves out. With the flag raised every column gets the
// one and nothing else is written.
template <class MN2>
__global__ void __launch_bounds__(256, hist_waves<MN2>())
    k_sparse_out(KeyDev key, const uint32_t* __restrict__ Nn2, uint32_t* acc, int nfeat, int nbins,
                 const uint16_t* __restrict__ zero_bin, const int32_t* __restrict__ hcnt,
                 const int32_t* __restrict__ flag, uint32_t* __restrict__ out, int32_t* __restrict__ cnt,
                 int32_t* __restrict__ nzsum) {
  const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  const int nb = nbins + 1, nacc = nfeat * nb;
  if (g >= nacc) return;
  const int f = (int)(g / nb), c = (int)(g - (int64_t)f * nb);
  const uint32_t z = zero_bin[f];
  const bool over = *flag != 0, sparse = z < (uint32_t)nbins, lane0 = MN2::G::g() == 0;
  MN2 M;
  M.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  if (!over && c < nbins && !(sparse && (uint32_t)c == z)) {
    M.load_strided(b, acc + g, nacc);
    M.mul(b, AOne{});
    M.reduce_once(b);
    M.store_words(b, out + ((size_t)f * nbins + c) * key.n2w, key.n2w);
    if (cnt && lane0) cnt[(size_t)f * nbins + c] = hcnt[g];
  }
  if (!over && sparse && (uint32_t)c != z && lane0) {
    const int32_t h = hcnt[g];
    if (h) atomicAdd(&nzsum[f], h);
  }
  if (over || !sparse || (uint32_t)c == z) {
    M.load_row(b, n2dev<MN2>(key).R1);
    M.reduce_once(b);
    M.store_strided(b, acc + g, nacc);
  }
}

// Lane group f: out[f][z_f] = total * inv[f] mod n^2 (inv[f] = Q_f^-1 as
// words, total any value its words hold), cnt[f][z_f] = count - nzsum[f].
template <class MN2, int PW>
__global__ void __launch_bounds__(256, hist_waves<MN2>())
    k_sparse_zero(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ inv,
                  const uint32_t* __restrict__ total, int nfeat, int nbins, const uint16_t* __restrict__ zero_bin,
                  int64_t count, const int32_t* __restrict__ nzsum, uint32_t* __restrict__ out,
                  int32_t* __restrict__ cnt) {
  const int64_t f = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  if (f >= nfeat) return;
  const uint32_t z = zero_bin[f];
  if (z >= (uint32_t)nbins) return;
  MN2 M;
  M.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  M.load_words(b, inv + (size_t)f * PW, PW);
  M.mul(b, ARowPacked<MN2::W, PW>{total});                        // inv T / R
  M.mul(b, ARow{n2dev<MN2>(key).Rpow + (size_t)2 * MN2::S4});  // times R^2 / R
  M.reduce_once(b);
  M.store_words(b, out + ((size_t)f * nbins + z) * key.n2w, key.n2w);
  if (cnt && MN2::G::g() == 0) cnt[(size_t)f * nbins + z] = (int32_t)(count - nzsum[f]);
}

}  // namespace xhe
