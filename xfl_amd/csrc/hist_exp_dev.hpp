// Fused ciphertext histogram for rows of mixed exponents (xhe_hist_exp):
// cell (f, b) = prod c[r]^(2^(e[r] - emin)) over its rows, emin the cell's
// smallest exponent. Raising every row before it is multiplied in costs
// sum (e[r] - emin) squarings per cell; here the exponents are walked
// downwards, Horner's rule in the exponent:
//   acc = 1; for every entry in DESCENDING exponent: acc = acc^(2^drop) * c,
//   drop = the previous entry's exponent minus this one's,
// which leaves prod c^(2^(e - emin)) with (largest - smallest exponent)
// squarings for the whole walk, whatever the number of entries.
//
// Stage A, k_hexp_tile: one block per (tile, feature), as k_hist_tile.
//   1. order    every element gets the key  bin << 13 | (dmax - d),  d = its
//               exponent minus the tile's smallest (an LDS atomic min; d is
//               clamped to [0, dmax], so an exponent is never an address), a
//               dropped element and the padding the key 2^32 - 1. A bitonic
//               sort of (key, local index) in LDS - 91 passes at 8192
//               elements, a few thousand LDS operations per thread against
//               the millions of mads of the tile's products - leaves every
//               bin's elements contiguous and in descending exponent; a bin's
//               range is its count (LDS atomics) and the position where its
//               keys begin.
//   2. slices   a bin of n elements is cut into ceil(n / kRawChunk) slices of
//               CONSECUTIVE entries (k_hist_tile interleaves them; here a
//               slice must cover one range of exponents, so that the slices'
//               spreads add up to the bin's and not to slices x spread). A
//               slice walks its entries once. Entries of one exponent are
//               chained as plain residues, k_chunk_prod_words' raw chain, on
//               top of the Montgomery accumulator: A R, then k rows, is
//               A P R^(1-k), and one product by R^(k+1) returns A P R - k + 1
//               products for a group of k, n + 1 for a slice of one exponent
//               (k_hist_tile's count) and 2 n at worst.
//   3. combine  the slices of a bin with several are parked with their
//               (smallest) exponents and walked the same way in chunks of
//               kRawChunk consecutive rows, each chunk leaving its result in
//               its own first row, pass after pass (row stride 1, 32, 1024)
//               until one row is left.
//   The block writes, per bin, a Montgomery row, the row's exponent and the
//   bin's element count (empty: Montgomery one, 0, 0).
// A squaring is the product of the accumulator with its own copy, as in
// k_align_mont and k_mulmod_n2: the copy is a row of the lane group in global
// memory. (SqLds would want 38 to 57 KB of LDS per block in the 2048- and
// 3072-bit shapes, next to up to 51 KB of sort keys.)
//
// Stage B, k_hexp_fold: the T partials of a cell carry different exponents;
// a lane group takes up to 32 of them (interleaved over the cell's tiles, as
// k_chunk_prod), skips the empty ones, and walks the others from the largest
// exponent down (a selection by exponent over a 32-bit mask: 32^2 / 2
// compares against 32 products of 10^4 mads each), squaring through SqLds as
// k_pack_n2 does. Levels repeat until a cell has one row; the last level
// writes the caller's exponents and counts, k_from_mont_rows its words.
//
// LDS of stage A (dynamic, hist_exp_lds_bytes): keys (4 B), indices (2 B) per
// element of the tile, two words per bin, the work list (tile_rows / 32
// words), the parked rows' exponents (tile_rows / 16 x 2 B).
#pragma once
#include "hist_dev.hpp"

namespace xhe {

constexpr uint32_t kHexpPad = 0xFFFFFFFFu;  // sort key of padding and dropped elements
constexpr int kHexpDBits = 13;              // key bits of the exponent field: dmax <= 8190

// b <- b^2 R^-1 through the lane group's own row `sq` ([S4] limbs, global)
template <class MN2>
XHE_DEV void hexp_square(const MN2& M, uint32_t (&b)[MN2::L], uint32_t* sq) {
  M.store_row(b, sq);
  wave_sync_mem_();
  M.mul(b, ARowV{sq});
}

// Block x = t * gf + fl: tile t of feature f0 + fl (k_hist_tile's grid). part:
// [S4][gf * nbins * T] strided rows, column (fl * nbins + b) * T + t, pexp and
// pcnt the columns' exponents and counts. ex: the rows' exponents or null (all
// 0). park: tile_rows / kHistParkDiv rows per block; sqws: 256 / TPI per block.
template <class MN2, int PW>
__global__ void __launch_bounds__(256, hist_waves<MN2>())
    k_hexp_tile(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ words,
                const int32_t* __restrict__ ex, const uint16_t* __restrict__ bins, int64_t bins_stride, int nbins,
                const int32_t* __restrict__ rows_idx, int64_t count, int dmax, int tile_rows, int f0, int gf, int64_t T,
                uint32_t* __restrict__ part, int32_t* __restrict__ pexp, int32_t* __restrict__ pcnt, uint32_t* park,
                uint32_t* sqws) {
  extern __shared__ uint32_t hist_lds[];
  uint32_t* skey = hist_lds;                 // bin << 13 | (dmax - d), sorted ascending
  uint32_t* A = skey + tile_rows;            // count | start << 16, later the bin's parked rows still to combine
  uint32_t* B = A + nbins;                   // the bin's first parked row
  uint32_t* work = B + nbins;                // bin << 8 | slice (chunk) index
  uint16_t* sidx = reinterpret_cast<uint16_t*>(work + tile_rows / kRawChunk);  // local element index, sorted with skey
  uint16_t* pd = sidx + tile_rows;           // d of a parked row
  __shared__ uint32_t s_nwork, s_nslots;
  __shared__ int s_emin;

  constexpr int S4 = MN2::S4, NGRP = 256 / MN2::TPI;
  constexpr uint32_t DM = (1u << kHexpDBits) - 1u;
  const int tid = threadIdx.x, grp = tid / MN2::TPI;
  const bool lead = MN2::G::g() == 0;
  const int64_t t = blockIdx.x / gf;
  const int fl = (int)(blockIdx.x - t * gf);
  const int64_t base = t * tile_rows;
  const int m = (int)(count - base < tile_rows ? count - base : tile_rows);
  const uint16_t* fb = bins + (size_t)(f0 + fl) * bins_stride;
  const int ncols = (int)((int64_t)gf * nbins * T);
  const int64_t col0 = (int64_t)fl * nbins * T + t;  // bin b: column col0 + b * T
  uint32_t* mypark = park + (size_t)blockIdx.x * (tile_rows / kHistParkDiv) * S4;
  uint32_t* mysq = sqws + ((size_t)blockIdx.x * NGRP + grp) * S4;
  auto row_of = [&](int i) -> int64_t { return rows_idx ? (int64_t)rows_idx[base + i] : base + i; };

  // 1. order
  int P = 2;  // the sorted length: a power of two >= m, at most tile_rows
  while (P < m) P <<= 1;
  for (int b = tid; b < nbins; b += 256) A[b] = 0;
  if (tid == 0) {
    s_nwork = s_nslots = 0;
    s_emin = INT32_MAX;
  }
  __syncthreads();
  if (ex)
    for (int i = tid; i < m; i += 256) atomicMin(&s_emin, ex[row_of(i)]);
  __syncthreads();
  const int emin = ex && m ? s_emin : 0;
  for (int i = tid; i < P; i += 256) {
    uint32_t k = kHexpPad;
    if (i < m) {
      const int64_t r = row_of(i);
      const uint32_t id = fb[r];
      if (id < (uint32_t)nbins) {
        uint32_t d = ex ? (uint32_t)ex[r] - (uint32_t)emin : 0u;
        if (d > (uint32_t)dmax) d = (uint32_t)dmax;
        k = (id << kHexpDBits) | ((uint32_t)dmax - d);
        atomicAdd(&A[id], 1u);
      }
    }
    skey[i] = k;
    sidx[i] = (uint16_t)i;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int q = tid; q < P / 2; q += 256) {
        const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
        const uint32_t a = skey[i], c = skey[l];
        if ((a > c) == ((i & k) == 0)) {
          skey[i] = c;
          skey[l] = a;
          const uint16_t ia = sidx[i];
          sidx[i] = sidx[l];
          sidx[l] = ia;
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < P; i += 256) {
    const uint32_t k = skey[i];
    if (k != kHexpPad && (i == 0 || (skey[i - 1] >> kHexpDBits) != (k >> kHexpDBits)))
      A[k >> kHexpDBits] |= (uint32_t)i << 16;  // (the bin's one writer; n <= 8192 and start < 8192)
  }
  __syncthreads();
  for (int b = tid; b < nbins; b += 256) {
    const uint32_t n = A[b] & 0xFFFFu, ns = (n + kRawChunk - 1) / kRawChunk;
    pcnt[col0 + (int64_t)b * T] = (int32_t)n;
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

  // 2. slices
  const int nitems = nbins + (int)s_nwork;
  for (int it = grp; it < nitems; it += NGRP) {
    int bin = it, j = 0;
    if (it >= nbins) {
      const uint32_t w = work[it - nbins];
      bin = (int)(w >> 8);
      j = (int)(w & 255u);
    }
    const uint32_t a = A[bin];
    const int n = (int)(a & 0xFFFFu), ns = (n + kRawChunk - 1) / kRawChunk;
    int cur = 0;  // d of the entry the walk stands on
    if (n == 0) {  // empty (bin, tile): Montgomery one at exponent 0
      M.load_row(b, opaque(n2dev<MN2>(key).R1));
      M.reduce_once(b);
    } else {
      const int p0 = (int)(a >> 16) + j * kRawChunk, len = n - j * kRawChunk < kRawChunk ? n - j * kRawChunk : kRawChunk;
      const uint32_t* kp = skey + p0;
      const uint16_t* li = sidx + p0;
      cur = dmax - (int)(kp[0] & DM);
      int u = 1, k = 1;  // k: the rows of the present exponent chained so far
      M.load_words(b, words + (size_t)row_of(li[0]) * PW, PW);
#pragma unroll 1
      while (u < len) {
        const int d = dmax - (int)(kp[u] & DM);
        if (d != cur) {  // (below cur: the keys ascend)
          M.mul(b, ARow{rpow + (size_t)(k + 1) * S4});
#pragma unroll 1
          for (int sq = cur - d; sq > 0; --sq) hexp_square(M, b, mysq);
          cur = d;
          k = 0;
        }
        M.mul(b, ARowPacked<MN2::W, PW>{words + (size_t)row_of(li[u]) * PW});
        ++k;
        ++u;
      }
      M.mul(b, ARow{rpow + (size_t)(k + 1) * S4});
      M.reduce_once(b);
    }
    if (ns <= 1) {
      M.store_strided(b, part + col0 + (int64_t)bin * T, opaque_i(ncols));
      if (lead) pexp[col0 + (int64_t)bin * T] = n ? (int32_t)((uint32_t)emin + (uint32_t)cur) : 0;
    } else {
      M.store_row(b, mypark + (size_t)(B[bin] + j) * S4);
      if (lead) pd[B[bin] + j] = (uint16_t)cur;
    }
  }
  __syncthreads();  // (every parked row and its exponent are written)

  // 3. combine
  for (int bb = tid; bb < nbins; bb += 256) {
    const uint32_t ns = ((A[bb] & 0xFFFFu) + kRawChunk - 1) / kRawChunk;
    A[bb] = ns > 1 ? ns : 0u;
  }
  for (int stride = 1;; stride *= kRawChunk) {
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
      const int p = (int)A[bin], nch = (p + kRawChunk - 1) / kRawChunk;
      const int len = p - j * kRawChunk < kRawChunk ? p - j * kRawChunk : kRawChunk;
      const int s0 = (int)B[bin] + j * kRawChunk * stride;  // the chunk's first row, and its result's
      uint32_t* r0 = mypark + (size_t)s0 * S4;
      int cur = pd[s0];
      M.load_row(b, r0);
#pragma unroll 1
      for (int u = 1; u < len; ++u) {
        const int d = pd[s0 + u * stride];
#pragma unroll 1
        for (int sq = cur - d; sq > 0; --sq) hexp_square(M, b, mysq);
        cur = d;
        M.mul(b, ARowV{r0 + (size_t)u * stride * S4});
      }
      M.reduce_once(b);
      if (nch == 1) {
        M.store_strided(b, part + col0 + (int64_t)bin * T, opaque_i(ncols));
        if (lead) pexp[col0 + (int64_t)bin * T] = (int32_t)((uint32_t)emin + (uint32_t)cur);
      } else {
        M.store_row(b, r0);
        if (lead) pd[s0] = (uint16_t)cur;
      }
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

// One fold level: lane group j = cell * nch + c takes the partials c, c + nch,
// ... of its cell's t_in (rows [S4][n_in], column cell * t_in + t, with their
// exponents ein and counts cin; at most 32 per group) and leaves row j of outp
// ([S4][n_out]), its exponent - the smallest of the non-empty partials, 0 when
// there is none - in eo[j] and the sum of the counts in co[j] (null: no
// counts). A drop is clamped to dmax: the exponents only count squarings.
template <class MN2>
__global__ void __launch_bounds__(256, 2)
    k_hexp_fold(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ in,
                const int32_t* __restrict__ ein, const int32_t* __restrict__ cin, int64_t n_in, int64_t t_in,
                int64_t nch, int64_t n_out, int dmax, uint32_t* __restrict__ outp, int32_t* __restrict__ eo,
                int32_t* __restrict__ co) {
  __shared__ __attribute__((aligned(16))) uint32_t sq_img[4][SqLds<MN2>::WORDS_PER_WAVE];  // 256-thread blocks
  const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  if (j >= n_out) return;
  const SqLds<MN2> L(sq_img[(threadIdx.x >> 6) & 3]);
  const int64_t cell = j / nch, c = j - cell * nch, first = cell * t_in + c;
  const int len = (int)((t_in - c + nch - 1) / nch);
  uint32_t mask = 0;
  int total = 0;
  for (int u = 0; u < len; ++u) {
    const int n = cin[first + u * nch];
    total += n;
    if (n > 0) mask |= 1u << u;
  }
  MN2 M;
  M.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  int cur = 0;
  if (!mask) {
    M.load_row(b, n2dev<MN2>(key).R1);
  } else {
    bool started = false;
#pragma unroll 1
    while (mask) {
      int best = 0, be = 0;
      bool any = false;
      for (uint32_t mm = mask; mm; mm &= mm - 1) {
        const int u = __builtin_ctz(mm), e = ein[first + u * nch];
        if (!any || e > be) {
          best = u;
          be = e;
          any = true;
        }
      }
      mask &= ~(1u << best);
      const uint32_t* row = in + first + best * nch;
      if (!started) {
        M.load_strided(b, row, (int)n_in);
        started = true;
      } else {
        uint32_t drop = (uint32_t)cur - (uint32_t)be;
        if (drop > (uint32_t)dmax) drop = (uint32_t)dmax;
#pragma unroll 1
        for (; drop > 0; --drop) {
          L.put(b);
          M.mul(b, L);
        }
        M.mul(b, AStrided{row, (int)n_in});
      }
      cur = be;
    }
  }
  M.reduce_once(b);
  M.store_strided(b, outp + j, (int)n_out);
  if (MN2::G::g() == 0) {
    eo[j] = cur;
    if (co) co[j] = total;
  }
}

}  // namespace xhe
