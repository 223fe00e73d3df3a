// Fused multi-feature ciphertext histogram (xhe_hist): stage A, k_hist_tile.
//
// One block per (tile, feature): the tile's `tile_rows` elements are ordered
// by the feature's bin ids in LDS - nothing is sorted in global memory and no
// ciphertext row moves - and multiplied per bin straight from the caller's
// [n_rows][PW] ciphertext words. The block leaves one Montgomery row per
// (feature, bin, tile); stage B (reduce_segments over uniform segments of T
// tiles, then k_from_mont_rows) is the launch layer's.
//
//   1. order    count per bin (LDS atomics), give every bin a range of the
//               element list, scatter the local element indices (uint16)
//               into it. The ranges come from an atomic range allocation and
//               not a prefix scan: the order of the bins in the list does not
//               matter, only that each bin's elements are contiguous.
//   2. slices   a bin of n elements is cut into ns = ceil(n / kRawChunk)
//               slices, interleaved over the bin's list (slice j takes
//               elements j, j + ns, ...). A slice is the raw chain of
//               k_chunk_prod_words: load_words the first row, one product per
//               further row on operands unpacked where they are used, one
//               product by R^(len+1) back to Montgomery form. Work item b <
//               nbins is slice 0 of bin b (an empty bin: the Montgomery one);
//               the further slices are listed behind them.
//   3. combine  a bin with one slice writes its partial row directly. The
//               slices of the others are parked in the block's workspace rows
//               and combined in passes of chunks of kRawChunk, interleaved and
//               in place (chunk j of nch reads rows j, j + nch, ... and writes
//               row j, which no other chunk reads), until one row is left: no
//               lane group ever walks more than kRawChunk dependent products,
//               whether a tile's rows fall into one bin (8192 rows: 256
//               slices, 8 chunks, 1) or into 4096.
//
// LDS (dynamic, hist_lds_bytes): two words per bin (count | range start,
// cursor / first parked row), the work list (tile_rows / 32 words: a bin has
// ceil(n / 32) - 1 <= n / 32 further slices, and a combine pass one chunk per
// 33 or more elements) and the element list (2 tile_rows bytes): 50.2 KB at
// 8192 rows x 4096 bins, 19.5 KB at 8192 x 256. The bin ids are not parked:
// the scatter reads them a second time through L2 (with the row ids, 6 bytes
// per element against the 512+ of its ciphertext row), which keeps the
// largest shape below the 64 KB a launch gets without opting in.
// Parked rows: at most tile_rows / 16 per block (a bin with more than one
// slice has ceil(n / 32) < n / 16 of them), [row][S4] limbs in global memory,
// written and read by the same block only.
#pragma once
#include "xhe_kernels.hpp"

namespace xhe {

// A row of limbs this kernel wrote itself (no __restrict__: not read-only here)
struct ARowV {
  const uint32_t* p;
  XHE_DEV uint4 load4(int i) const { return *reinterpret_cast<const uint4*>(p + i); }
};

constexpr int kHistParkDiv = 16;  // parked rows per block: tile_rows / kHistParkDiv

__global__ void k_hist_zero(int32_t* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}

// Blocks per CU the kernel is compiled for: 2, except for the 57-limb shape
// (scan_waves' reason). The item loop makes the partial row's limb offsets
// ((g L + j) * ncols, a 64-bit pair per limb) loop-invariant, and hoisted out
// of it they spilled 111 VGPRs inside the product loop at 2048 bits: the
// stride is laundered per item (opaque_i), which keeps them where they are
// used. What is left at 2 blocks: at 2048 bits one 64-bit value in scratch
// (12 B), touched in the LDS phases and once per combine pass; at 8192 bits
// 44 B, reloaded in the item loop's store epilogue once per work item. No
// chain loop and no product holds a scratch access (DESIGN "Fused histogram").
template <class MN2>
constexpr int hist_waves() {
  return scan_waves<MN2>();
}

// One block's work, shared by k_hist_tile and k_level_tile (hist_level_dev.hpp):
// the m elements base .. base + m - 1 of the call (row rows_idx[base + i], or
// base + i without row ids) by the bin ids fb[row] of one feature. The bin's
// partial row goes to column bin * bin_stride of mypart ([S4][ncols] strided
// rows), its count is added to cnt_f[bin] (null: no counts); mypark: the
// block's tile_rows / kHistParkDiv parked rows. Hidden (the sparse histogram's
// lists, hist_sparse_dev.hpp): an id at or above nbins - 1 counts into the last
// bin instead of dropping the element.
template <class MN2, int PW, bool Hidden = false>
XHE_DEV void hist_tile_block(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ words,
                             const uint16_t* __restrict__ fb, int nbins, const int32_t* __restrict__ rows_idx,
                             int64_t base, int m, int tile_rows, uint32_t* mypart, int64_t bin_stride, int ncols,
                             uint32_t* mypark, int32_t* __restrict__ cnt_f) {
  extern __shared__ uint32_t hist_lds[];
  uint32_t* A = hist_lds;       // count | start << 16, later the bin's parked rows still to combine
  uint32_t* B = A + nbins;      // scatter cursor, later the bin's first parked row
  uint32_t* work = B + nbins;   // bin << 8 | slice (chunk) index
  uint16_t* list = reinterpret_cast<uint16_t*>(work + tile_rows / kRawChunk);
  __shared__ uint32_t s_total, s_nwork, s_nslots;

  constexpr int S4 = MN2::S4, NGRP = 256 / MN2::TPI;
  const int tid = threadIdx.x, grp = tid / MN2::TPI;
  auto row_of = [&](int i) -> int64_t { return rows_idx ? (int64_t)rows_idx[base + i] : base + i; };
  auto id_of = [&](int i) -> uint32_t {
    const uint32_t id = fb[row_of(i)];
    if constexpr (Hidden) return id < (uint32_t)nbins ? id : (uint32_t)nbins - 1u;
    else return id;
  };

  for (int b = tid; b < nbins; b += 256) A[b] = 0;
  if (tid == 0) s_total = s_nwork = s_nslots = 0;
  __syncthreads();
  for (int i = tid; i < m; i += 256) {
    const uint32_t id = id_of(i);
    if (id < (uint32_t)nbins) atomicAdd(&A[id], 1u);
  }
  __syncthreads();
  for (int b = tid; b < nbins; b += 256) {
    const uint32_t n = A[b];
    const uint32_t start = n ? atomicAdd(&s_total, n) : 0u;
    A[b] = n | (start << 16);  // n <= 8192 and start < 8192
    B[b] = start;
    if (cnt_f && n) atomicAdd(&cnt_f[b], (int)n);
  }
  __syncthreads();
  for (int i = tid; i < m; i += 256) {
    const uint32_t id = id_of(i);
    if (id < (uint32_t)nbins) list[atomicAdd(&B[id], 1u)] = (uint16_t)i;
  }
  __syncthreads();
  for (int b = tid; b < nbins; b += 256) {
    const uint32_t ns = ((A[b] & 0xFFFFu) + kRawChunk - 1) / kRawChunk;
    if (ns > 1) {
      B[b] = atomicAdd(&s_nslots, ns);
      const uint32_t w = atomicAdd(&s_nwork, ns - 1);
      for (uint32_t j = 1; j < ns; ++j) work[w + j - 1] = ((uint32_t)b << 8) | j;  // j <= 255
    }
  }
  __syncthreads();

  MN2 M;
  M.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  const uint32_t* rpow = n2dev<MN2>(key).Rpow;

  const int nitems = nbins + (int)s_nwork;
  for (int it = grp; it < nitems; it += NGRP) {
    int bin = it, j = 0;
    if (it >= nbins) {
      const uint32_t w = work[it - nbins];
      bin = (int)(w >> 8);
      j = (int)(w & 255u);
    }
    const uint32_t a = A[bin];
    const int n = (int)(a & 0xFFFFu), ns = n > kRawChunk ? (n + kRawChunk - 1) / kRawChunk : 1;
    if (n == 0) {  // empty (bin, tile): Montgomery one
      M.load_row(b, opaque(n2dev<MN2>(key).R1));  // (opaque: the row is not hoisted out of the item loop)
      M.reduce_once(b);
    } else {
      const int len = (n - j + ns - 1) / ns;
      const uint16_t* li = list + (a >> 16) + j;
      M.load_words(b, words + (size_t)row_of(li[0]) * PW, PW);
#pragma unroll 1
      for (int u = 1; u < len; ++u) M.mul(b, ARowPacked<MN2::W, PW>{words + (size_t)row_of(li[u * ns]) * PW});
      M.mul(b, ARow{rpow + (size_t)(len + 1) * S4});
      M.reduce_once(b);
    }
    if (ns == 1) M.store_strided(b, mypart + (int64_t)bin * bin_stride, opaque_i(ncols));
    else M.store_row(b, mypark + (size_t)(B[bin] + j) * S4);
  }
  __syncthreads();  // (every parked row is written)

  for (int bb = tid; bb < nbins; bb += 256) {
    const uint32_t ns = ((A[bb] & 0xFFFFu) + kRawChunk - 1) / kRawChunk;
    A[bb] = ns > 1 ? ns : 0u;
  }
  while (true) {
    if (tid == 0) s_nwork = 0;
    __syncthreads();
    for (int bb = tid; bb < nbins; bb += 256) {
      const uint32_t p = A[bb];
      if (p > 1) {
        const uint32_t nch = (p + kRawChunk - 1) / kRawChunk;
        const uint32_t w = atomicAdd(&s_nwork, nch);
        for (uint32_t j = 0; j < nch; ++j) work[w + j] = ((uint32_t)bb << 8) | j;
      }
    }
    __syncthreads();
    const int nw = (int)s_nwork;
    if (nw == 0) break;  // (uniform: every thread reads the same count)
    for (int it = grp; it < nw; it += NGRP) {
      const uint32_t w = work[it];
      const int bin = (int)(w >> 8), j = (int)(w & 255u);
      const int p = (int)A[bin], nch = (p + kRawChunk - 1) / kRawChunk, len = (p - j + nch - 1) / nch;
      uint32_t* r0 = mypark + (size_t)(B[bin] + j) * S4;
      M.load_row(b, r0);
#pragma unroll 1
      for (int u = 1; u < len; ++u) M.mul(b, ARowV{r0 + (size_t)u * nch * S4});
      M.reduce_once(b);
      if (nch == 1) M.store_strided(b, mypart + (int64_t)bin * bin_stride, opaque_i(ncols));
      else M.store_row(b, r0);
    }
    __syncthreads();
    for (int bb = tid; bb < nbins; bb += 256) {
      const uint32_t p = A[bb];
      if (p > 1) {
        const uint32_t nch = (p + kRawChunk - 1) / kRawChunk;
        A[bb] = nch > 1 ? nch : 0u;
      }
    }
  }
}

// Block x = t * gf + fl: tile t of feature f0 + fl (the features of one tile
// are neighbours, so the tile's ciphertext rows are read from HBM once and
// from L2 by the others). part: [S4][gf * nbins * T] strided rows, column
// (fl * nbins + b) * T + t. rows_idx: the caller's row ids (trusted < n_rows)
// or null (element i is row i). cnt_out: zeroed before the launch, or null.
template <class MN2, int PW>
__global__ void __launch_bounds__(256, hist_waves<MN2>())
    k_hist_tile(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ words,
                const uint16_t* __restrict__ bins, int64_t bins_stride, int nbins,
                const int32_t* __restrict__ rows_idx, int64_t count, int tile_rows, int f0, int gf, int64_t T,
                uint32_t* __restrict__ part, uint32_t* park, int32_t* __restrict__ cnt_out) {
  const int64_t t = blockIdx.x / gf;
  const int fl = (int)(blockIdx.x - t * gf);
  const int64_t base = t * tile_rows;
  const int m = (int)(count - base < tile_rows ? count - base : tile_rows);
  hist_tile_block<MN2, PW>(key, Nn2, words, bins + (size_t)(f0 + fl) * bins_stride, nbins, rows_idx, base, m,
                           tile_rows, part + (int64_t)fl * nbins * T + t, T, (int)((int64_t)gf * nbins * T),
                           park + (size_t)blockIdx.x * (tile_rows / kHistParkDiv) * MN2::S4,
                           cnt_out ? cnt_out + (size_t)(f0 + fl) * nbins : nullptr);
}

}  // namespace xhe
