// Bucket multi-exponentiation (xhe_bucketexp): the kernels around the fused
// histogram's stage A and B.
//
//   out[j] = prod_t bases[t]^(s k[j][t]) mod n^2,   s = -1 where neg[j][t]
//
// Per output column j and window w of c bits every term goes into the bucket
// of its digit with ONE product - that is xhe_hist's accumulation with
// "feature" = (j, w) and "bin" = the digit (k_hist_tile, hist_dev.hpp, on the
// uint16 matrix k_bucket_digits writes) - and the m = 2^c - 1 buckets of a
// (column, window, sign) are then folded as prod_d B_d^d (k_bucket_fold). No
// table and no inverted base: the negative terms have a bucket range of their
// own, and out = Pos * Neg^-1 costs one inversion per output.
//
// Digit -> bin:  digit 0 -> 0xFFFF (dropped by k_hist_tile);
//                positive digit d -> d - 1;  negative digit d -> m + d - 1.
// nbins = m without a sign array, 2 m with one (<= 4094 at c = 11).
//
// k_bucket_fold, one 256-thread block per (column, window, sign), NGRP = 256 /
// TPI lane groups. With bucket 0 padded as the Montgomery one there are 2^c
// buckets, cut into NG = min(NGRP, 2^c) contiguous chunks of L = 2^c / NG:
//   level 1  group g walks its chunk from the top with running products
//            S *= B_d; F *= S, and leaves S_g (the chunk's total) and F_g =
//            prod_i B_{gL+i}^i (its local fold): 2 L - 3 products on the chain.
//   level 2  prod_d B_d^d = prod_g F_g * (prod_g S_g^g)^L, and prod_g S_g^g =
//            prod_{g >= 1} Suf_g with Suf_g = prod_{h >= g} S_h: the running-
//            product fold again, as a suffix scan over the groups (log2 NG
//            steps of one product each, in place in LDS). Every group then
//            raises its Suf_g to L (log2 L squarings), multiplies by its F_g,
//            and a tree over the groups (log2 NG steps) leaves the fold.
// Chain depth 2 L - 3 + 2 log2 NG + log2 L + 1 products: 20 at c = 8 with 64
// groups (L = 4), 42 with 16 groups (L = 16), 79 / 269 at c = 11 - against
// the 2 m = 510 (4094) of one running-product walk.
//
// A product's operand a is always read from memory (bn_dev.hpp), so a group
// keeps ONE residue in registers: S_g lives in the group's LDS row, F_g in
// its row of the block's workspace in global memory (written and read by the
// same block only, as the histogram's parked rows), and the step "S *= B; F
// *= S" is  b = B_d; b *= S (LDS); S = b; b *= F (global); F = b.
// LDS: NGRP rows of S4 words - 38.9 KB at 2048 bits (64 x 608 B), 58.4 KB at
// 3072 (64 x 912 B), 19.5 KB at 4096 (16 x 1216 B), 41.0 KB at 8192 (16 x
// 2560 B): below the 64 KB a launch gets without opting in.
#pragma once
#include "hist_dev.hpp"

namespace xhe {

// One thread per (column, term): the term's kw words are read once, low word
// first, through a 64-bit window; block x walks t (the uint16 stores of a
// wave are 128 contiguous bytes), block y is the column of the launch group.
// k: [ncols][nterms][kw], neg: [ncols][nterms] or null, both already offset
// to the group's first column. bins: [gcols * nwin][stride].
__global__ void __launch_bounds__(256)
    k_bucket_digits(const uint32_t* __restrict__ k, const uint8_t* __restrict__ neg, int kw, int64_t nterms, int c,
                    int nwin, uint16_t* __restrict__ bins, int64_t stride) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nterms) return;
  const int64_t j = blockIdx.y;
  const uint32_t* kt = k + ((size_t)j * nterms + t) * kw;
  const uint32_t m = (1u << c) - 1u;
  const uint32_t off = neg && neg[(size_t)j * nterms + t] ? m : 0u;
  uint16_t* o = bins + (size_t)j * nwin * stride + t;
  uint64_t acc = 0;
  int have = 0, wi = 0;
  for (int w = 0; w < nwin; ++w) {
    if (have < c && wi < kw) {  // (have < 11: the next word fits)
      acc |= (uint64_t)kt[wi++] << have;
      have += 32;
    }
    const uint32_t d = (uint32_t)acc & m;
    acc >>= c;
    have = have > c ? have - c : 0;
    o[(size_t)w * stride] = (uint16_t)(d ? off + d - 1u : 0xFFFFu);
  }
}

template <class MN2>
constexpr int bucket_fold_lds() {
  return (256 / MN2::TPI) * MN2::S4 * 4;
}

// Block x = f * nsign + sg: feature f (column * nwin + window, local to the
// launch group) and sign range sg. cur: the group's Montgomery bucket rows
// [S4][ncur], bucket d of the block at column f * nbins + sg * m + d - 1.
// frows: NGRP rows of S4 words per block. P: [S4][pcols], the block's fold
// goes to column sg * sign_stride + pcol0 + f (k_mexp_horner's layout: column
// j * nwin + w with the Neg columns behind the Pos ones).
// Compiled for one block per CU: at two the level-1 bucket loop reloaded
// spilled values from scratch at the head of every step (one 8-byte value at
// 2048 bits, seven at 8192), and the fold's grid - one block per (column,
// window, sign) - rarely fills the chip twice over anyway.
template <class MN2>
__global__ void __launch_bounds__(256, 1)
    k_bucket_fold(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ cur, int ncur, int nbins,
                  int c, int nsign, uint32_t* frows, uint32_t* __restrict__ P, int pcols, int64_t pcol0,
                  int64_t sign_stride) {
  extern __shared__ uint32_t fold_lds[];
  constexpr int S4 = MN2::S4, NGRP = 256 / MN2::TPI;
  static_assert(bucket_fold_lds<MN2>() <= 60 * 1024, "k_bucket_fold: the S rows must fit the default LDS");
  const int grp = threadIdx.x / MN2::TPI;
  const int nb = 1 << c, m = nb - 1;
  const int L = nb > NGRP ? nb / NGRP : 1, NG = nb / L;
  const int f = blockIdx.x / nsign, sg = blockIdx.x - f * nsign;
  const uint32_t* Bk = cur + (int64_t)f * nbins + (int64_t)sg * m - 1;  // bucket d >= 1 at Bk + d
  uint32_t* srow = fold_lds + grp * S4;
  uint32_t* frow = frows + ((size_t)blockIdx.x * NGRP + grp) * S4;
  const bool act = grp < NG;

  MN2 M;
  M.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  auto one = [&]() {
    M.load_row(b, opaque(n2dev<MN2>(key).R1));
    M.reduce_once(b);
  };

  // level 1: S_g in srow (and b), F_g in frow (L > 1)
  if (act) {
    const int lo = grp * L, hi = lo + L - 1;
    if (hi == 0) one();  // (L == 1, group 0: the padded bucket)
    else M.load_strided(b, Bk + hi, ncur);
    M.store_row(b, srow);
    if (L > 1) {
      M.store_row(b, frow);
      wave_sync_mem_();
#pragma unroll 1
      for (int d = hi - 1; d > lo; --d) {
        M.load_strided(b, Bk + d, ncur);
        M.mul(b, ARowV{srow});
        M.store_row(b, srow);
        wave_sync_mem_();
        M.mul(b, ARowV{frow});
        M.store_row(b, frow);
        wave_sync_mem_();
      }
      if (lo > 0) {  // the chunk's first bucket counts in S_g alone (chunk 0: the padded one)
        M.load_strided(b, Bk + lo, ncur);
        M.mul(b, ARowV{srow});
        M.store_row(b, srow);
      } else {
        M.load_row(b, srow);
      }
    }
  }
  __syncthreads();

  // level 2: suffix products of the chunk totals, in place
  for (int off = 1; off < NG; off <<= 1) {
    const bool on = act && grp + off < NG;
    if (on) M.mul(b, ARowV{fold_lds + (grp + off) * S4});
    __syncthreads();  // (every partner row is read before its owner rewrites it)
    if (on) M.store_row(b, srow);
    __syncthreads();
  }
  // X_g = Suf_g^L * F_g (g >= 1), X_0 = F_0
  if (act) {
    if (grp == 0) {
      if (L > 1) M.load_row(b, frow);
      else one();
    } else {
      for (int l = L; l > 1; l >>= 1) {
        M.mul(b, ARowV{srow});
        M.store_row(b, srow);
        wave_sync_mem_();
      }
      if (L > 1) M.mul(b, ARowV{frow});
    }
    M.store_row(b, srow);
  }
  __syncthreads();
  // tree over the groups: a step reads rows >= off and writes rows < off
  for (int off = NG >> 1; off >= 1; off >>= 1) {
    if (grp < off) {
      M.mul(b, ARowV{fold_lds + (grp + off) * S4});
      M.store_row(b, srow);
    }
    __syncthreads();
  }
  if (grp == 0) {
    M.reduce_once(b);
    M.store_strided(b, P + sg * sign_stride + pcol0 + f, pcols);
  }
}

// out[j] = pos[j] * ninv[j] mod n^2 on plain words (the Horner outputs and
// the batch inverse of the Neg half): to Montgomery form by R^2, then one
// product by the packed inverse.
template <class MN2, int PW>
__global__ void __launch_bounds__(256, 2)
    k_bucket_finish(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ pos,
                    const uint32_t* __restrict__ ninv, int64_t ncols, uint32_t* __restrict__ out) {
  const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  if (j >= ncols) return;
  MN2 M;
  M.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  M.load_words(b, pos + (size_t)j * PW, PW);
  M.mul(b, ARow{n2dev<MN2>(key).R2});
  M.mul(b, ARowPacked<MN2::W, PW>{ninv + (size_t)j * PW});
  M.reduce_once(b);
  M.store_words(b, out + (size_t)j * key.n2w, key.n2w);
}

}  // namespace xhe
