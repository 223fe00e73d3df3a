// k_enc_obf: the online half of an encryption, on an obfuscator X made
// earlier (xhe_obf_fill): ct = (1 + n m) X mod n^2 without a product mod n^2.
//
//   x0 = X mod n,  t = (m x0) mod n,  ct = X + n t - [>= n^2] n^2
//
// ((1 + n m) X = X + n m (x0 + n (X div n)) = X + n (m x0) (mod n^2), and
// n (m x0) = n t (mod n^2); X < n^2 and t < n give X + n t < 2 n^2.)
//
// One lane group per element in the 4-lane (p2L) limb shape M, whose S limbs
// of W bits hold a residue mod n (R = 2^(W S) >= 16 n): key.nL is n as a
// Montgomery modulus in it, key.n2_limL is n^2 in 2 S limbs. Per element:
//   one Montgomery reduction of the 2 S limbs of X       (S^2 mads)   X R^-1
//   two Montgomery products, by R^3 and by m             (4 S^2)      t
//   one wide product n t on top of X                     (S^2)
//   one compare-and-subtract of n^2 over the 2 S limbs
// against 2 (2 S)^2 = 8 S^2 mads for one product mod n^2. A 2 S-limb value is
// held as two halves in the lane layout: lane g has limbs [g L, (g + 1) L) of
// the low half and of the high half. The wide product retires its low limbs
// one per column from lane 0; they reach their lanes through a row of LDS.
#pragma once
#include "bn_dev.hpp"
#include "keydev.hpp"

namespace xhe {

// Operand-a source over packed little-endian words: limb i is bits
// [bit0 + W i, bit0 + W (i + 1)) of the nwords words at w (zero beyond them).
// Uniform inside a lane group.
template <int W>
struct AWords {
  const uint32_t* w;
  int nwords, bit0;
  XHE_DEV uint32_t limb(int i) const {
    const int bit = bit0 + W * i, k = bit >> 5, sh = bit & 31;
    const uint32_t lo = word_or0(w, k, nwords), hi = word_or0(w, k + 1, nwords);
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh) & ((1u << W) - 1u);
  }
  XHE_DEV uint4 load4(int i) const { return make_uint4(limb(i), limb(i + 1), limb(i + 2), limb(i + 3)); }
};

// Mont::load_words for the high half: limbs [S, 2 S) of the packed words (the
// lane index dispatched to compile-time copies, as load_words_from does)
template <class M, int GG>
XHE_DEV void load_high_g(uint32_t (&b)[M::L], const uint32_t* w, int nwords) {
#pragma unroll
  for (int j = 0; j < M::L; ++j) {
    const int bit = M::W * (M::S + GG * M::L + j);
    const int k = bit >> 5, sh = bit & 31;
    const uint32_t lo = word_or0(w, k, nwords);
    const uint32_t hi = sh + M::W > 32 ? word_or0(w, k + 1, nwords) : 0u;
    b[j] = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh) & M::MASK;
  }
}
template <class M, int GG = 0>
XHE_DEV void load_high(uint32_t (&b)[M::L], const uint32_t* w, int nwords, int g) {
  if constexpr (GG == M::TPI - 1) {
    load_high_g<M, GG>(b, w, nwords);
  } else {
    if (g == GG) load_high_g<M, GG>(b, w, nwords);
    else load_high<M, GG + 1>(b, w, nwords, g);
  }
}

// d = b - row - bin over one half (bin: the borrow into limb 0 of lane 0);
// returns the borrow out of the half's top limb, the same in every lane of
// the group. The ripple is reduce_once's: a lane emits at most one borrow, so
// TPI - 1 rounds of passing them up settle it.
template <class M>
XHE_DEV uint32_t sub_half(const uint32_t (&b)[M::L], const uint32_t* row, uint32_t bin, uint32_t (&d)[M::L]) {
  using G = typename M::G;
  const int g = G::g();
  uint32_t br = g == 0 ? bin : 0u;
#pragma unroll
  for (int j = 0; j < M::L; ++j) {
    const int64_t x = (int64_t)b[j] - (int64_t)row[g * M::L + j] - (int64_t)br;
    br = x < 0 ? 1u : 0u;
    d[j] = (uint32_t)(x + ((int64_t)br << M::W));
  }
  if constexpr (M::TPI > 1) {
    uint32_t total = br;
#pragma unroll
    for (int r = 1; r < M::TPI; ++r) {
      uint32_t in = G::from_prev(br);
#pragma unroll
      for (int j = 0; j < M::L; ++j) {
        const int64_t x = (int64_t)d[j] - (int64_t)in;
        in = x < 0 ? 1u : 0u;
        d[j] = (uint32_t)(x + ((int64_t)in << M::W));
      }
      br = in;
      total |= in;
    }
    br = G::bcast_last(total);
  }
  return br;
}

// Mont::store_words for one half of a 2 S-limb value: the half's limb 0 is
// bit `base` of the words at out; n0, n1 are the two limbs that follow this
// lane's (the next lane's first two; past the low half's last lane, the high
// half's first two). A lane writes the words that start in its bits.
template <class M>
XHE_DEV void store_half(const uint32_t (&b)[M::L], uint32_t n0, uint32_t n1, int base, uint32_t* __restrict__ out,
                        int nwords) {
  constexpr int L = M::L, W = M::W, LB = L * W, NWM = (LB + 31) / 32 + 1;
  auto limb = [&](int x) -> uint64_t {
    return x < L ? (uint64_t)b[x] : x == L ? (uint64_t)n0 : x == L + 1 ? (uint64_t)n1 : 0ull;
  };
  uint32_t u[NWM + 1];
#pragma unroll
  for (int i = 0; i <= NWM; ++i) {
    const int bit = 32 * i, jl = bit / W, sh = bit - jl * W;
    const uint64_t v = limb(jl) | (limb(jl + 1) << W) | (limb(jl + 2) << (2 * W));
    u[i] = (uint32_t)(v >> sh);
  }
  const int b0 = base + M::G::g() * LB, ks = (b0 + 31) >> 5;
  const int off = (ks << 5) - b0;  // [0, 32): local bit of the lane's first word
  const int ke = (b0 + LB + 31) >> 5, kend = ke < nwords ? ke : nwords;
  uint32_t* o = out + ks;
#pragma unroll
  for (int i = 0; i < NWM; ++i) {
    const uint32_t w = (uint32_t)((((uint64_t)u[i + 1] << 32) | u[i]) >> off);
    if (ks + i < kend) o[i] = w;
  }
}

// m: [count][nw] words (m < n), obf: [count][n2w] words (X < n^2), out:
// [count][n2w] words, not overlapping obf. wipe: row e of obf is zeroed once
// its last read has completed. Blocks of 256 threads.
template <class M>
__global__ void __launch_bounds__(256) k_enc_obf(KeyDev key, const uint32_t* __restrict__ m_words, uint32_t* obf,
                                                 int64_t count, int wipe, uint32_t* __restrict__ out) {
  using G = typename M::G;
  constexpr int S = M::S, L = M::L, W = M::W, TPI = M::TPI;
  constexpr int RS = M::S4 | 1;  // LDS row stride (odd: the groups' lead lanes write distinct banks)
  __shared__ uint32_t low_all[(256 / TPI) * RS];
  const int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / TPI;
  if (e >= count) return;  // whole groups leave together
  const int g = G::g();
  const bool lead = g == 0;
  uint32_t* low = low_all + (threadIdx.x / TPI) * RS;
  uint32_t* X = obf + (size_t)e * key.n2w;
  M mod;
  mod.init(key.nL.N, key.nL.n0inv);

  // t = m (X mod n) mod n
  uint32_t t[L];
  mod.load_words(t, X, key.n2w);                            // limbs [0, S) of X
  mod.redc_wide(t, AWords<W>{X, key.n2w, W * S});            // X R^-1 mod n (X < n^2 < R n)
  mod.mul(t, ARow{key.nL.R3});                               // X R
  mod.mul(t, AWords<W>{m_words + (size_t)e * key.nw, key.nw, 0});  // X m
  mod.reduce_once(t);                                        // [0, n)

  // X + n t: the columns of n over the limbs of t, on top of X's low half;
  // lane 0 retires one low limb per column into the LDS row
  uint64_t T[L];
  {
    uint32_t x[L];
    mod.load_words(x, X, key.n2w);
#pragma unroll
    for (int j = 0; j < L; ++j) T[j] = x[j];
  }
  for (int i0 = 0; i0 < M::S4; i0 += 4) {
    const uint4 a4 = ARow{key.nL.N}.load4(i0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (i0 + r < S) {
        const uint32_t ai = comp4(a4, r);
        const uint64_t x0 = mad64(ai, t[0], T[0]);
        if (lead) low[i0 + r] = (uint32_t)x0 & M::MASK;
        mad_shift(T, t, ai);
        T[L - 1] = G::from_next64(x0);
        T[0] += lead ? (x0 >> W) : 0ull;
      }
    }
  }
  uint32_t hi[L], lo[L];
  {
    uint32_t x[L];
    load_high<M>(x, X, key.n2w, g);  // X's high half joins the columns [S, 2 S)
#pragma unroll
    for (int j = 0; j < L; ++j) T[j] += x[j];
  }
  mod.normalize(T, hi);  // X + n t < 2 n^2 < 2^(2 W S): no carry leaves the top lane
  wave_sync_mem_();      // the LDS row is complete, and every read of X has returned
  if (wipe) {
    for (int k = g; k < key.n2w; k += TPI) X[k] = 0u;
  }
#pragma unroll
  for (int j = 0; j < L; ++j) lo[j] = low[g * L + j];

  // - n^2 when it fits
  {
    uint32_t dlo[L], dhi[L];
    uint32_t br = sub_half<M>(lo, key.n2_limL, 0u, dlo);
    br = sub_half<M>(hi, key.n2_limL + S, br, dhi);
    if (!br) {
#pragma unroll
      for (int j = 0; j < L; ++j) lo[j] = dlo[j], hi[j] = dhi[j];
    }
  }

  uint32_t* o = out + (size_t)e * key.n2w;
  const uint32_t h0 = G::bcast0(hi[0]), h1 = G::bcast0(hi[1]);
  const uint32_t l0 = G::from_next(lo[0]), l1 = G::from_next(lo[1]);
  const bool last = g == TPI - 1;
  store_half<M>(lo, last ? h0 : l0, last ? h1 : l1, 0, o, key.n2w);
  store_half<M>(hi, G::from_next(hi[0]), G::from_next(hi[1]), W * S, o, key.n2w);
}

}  // namespace xhe
