// Batched base-2 Fermat test for the key-prime search (include/xhe.h
// xhe_fermat2_host): pass = [2^(N-1) == 1 (mod N)] for candidates
// N = start + offset, each with a modulus of its own.
//
// Every other Montgomery kernel of this library takes one modulus per key;
// here the modulus differs from candidate to candidate, so it lives in the
// per-lane registers of the lane-group shapes (Mont::nl, TPI > 1) and the
// constants a key would bring are derived on the device per candidate:
//   N        start + offset, the carry rippling through every word (LDS row)
//   n0inv    -N^-1 mod 2^W by Newton steps on the low word
//   R mod N  2^BITS - N is already reduced (the top bit of N is set), then
//            W*S - BITS modular doublings (shift, conditional subtraction)
// The exponentiation runs left to right over the bits of N - 1 on the
// Montgomery form of 2: one squaring per bit (the operand goes through the
// group's LDS row, SqLds) and a doubling where the bit is set. The doubling is
// a one-bit shift across the group's limbs and stays unreduced: R >= 2^32 N in
// every shape below, so a squaring of an operand below 4N is below 2N again
// ("almost Montgomery", bn_dev.hpp) and the only conditional subtraction is
// the one before the verdict, which compares with R mod N. No table, no
// general product.
//
// One candidate is one lane group (8 lanes up to 1536 bits, a 16-lane DPP row
// above), one wave a block: a search window holds tens to a few hundred
// candidates, far fewer waves than the chip has SIMDs, so the time of a launch
// is one candidate's chain of BITS dependent squarings and the shapes are the
// ones with the fewest limbs per lane that Mont has (L = 5 .. 10).
#pragma once
#include "bn_dev.hpp"
#include "xhe_kernels.hpp"

namespace xhe {

// b <- b << s over the group's W-bit limbs, s = 0 or 1 (group-uniform); the
// value stays below 2^(W S), so the bit leaving the top limb is zero
template <class M>
XHE_DEV void shl_bit(uint32_t (&b)[M::L], uint32_t s) {
  const uint32_t in = M::G::from_prev(b[M::L - 1]);
  const uint32_t rs = M::W - s;  // s = 0: a limb >> W = 0
#pragma unroll
  for (int j = M::L - 1; j > 0; --j) b[j] = ((b[j] << s) | (b[j - 1] >> rs)) & M::MASK;
  b[0] = ((b[0] << s) | (in >> rs)) & M::MASK;
}

// starts: rows of BITS/32 words; candidate e is starts[which[e]] + offs[e]
// (checked by the caller: odd, top bit set, no carry out of BITS bits).
template <class M, int BITS>
__global__ void __launch_bounds__(64) k_fermat2(const uint32_t* __restrict__ starts,
                                                const int32_t* __restrict__ which,
                                                const uint32_t* __restrict__ offs, int64_t count,
                                                uint8_t* __restrict__ pass) {
  constexpr int TPI = M::TPI, L = M::L, NW = BITS / 32, GPW = 64 / TPI;
  static_assert(TPI == 8 || TPI == 16, "lane groups inside one DPP row");
  static_assert(M::W * M::S >= BITS + 32, "R >= 2^32 N: doublings stay unreduced between squarings");
  static_assert(M::S4 >= NW && M::S4 == M::S, "the squaring row also stages 2^BITS - N");
  __shared__ __attribute__((aligned(16))) uint32_t n_img[GPW][NW];
  __shared__ __attribute__((aligned(16))) uint32_t sq_img[SqLds<M>::WORDS_PER_WAVE];
  const int g = M::G::g();
  const int grp = (int)(threadIdx.x & 63) / TPI;
  const int64_t e_raw = (int64_t)blockIdx.x * GPW + grp;
  const bool real = e_raw < count;
  const int64_t e = real ? e_raw : count - 1;  // idle groups repeat the last candidate: the wave stays whole
  uint32_t* nw = n_img[grp];
  const SqLds<M> sq(sq_img);

  // N = start + offset
  const uint32_t* st = starts + (size_t)which[e] * NW;
  for (int k = g; k < NW; k += TPI) nw[k] = st[k];
  wave_sync_mem_();
  if (g == 0) {
    const uint32_t lo = nw[0] + offs[e];
    uint32_t c = lo < nw[0] ? 1u : 0u;
    nw[0] = lo;
    for (int k = 1; k < NW && c; ++k) {
      const uint32_t v = nw[k] + 1u;
      nw[k] = v;
      c = v == 0u ? 1u : 0u;
    }
  }
  wave_sync_mem_();

  M mo;
  mo.N = nullptr;  // lane groups read the modulus from nl only
  {
    // -N^-1 mod 2^W: x = N is an inverse to 3 bits, each step doubles them
    const uint32_t n0 = nw[0];
    uint32_t x = n0;
#pragma unroll
    for (int it = 0; it < 4; ++it) x *= 2u - n0 * x;
    mo.n0inv = (0u - x) & M::MASK;
    uint32_t nl[L];
    mo.load_words(nl, nw, NW);
#pragma unroll
    for (int j = 0; j < L; ++j) mo.nl[j] = nl[j];
  }

  // R mod N from 2^BITS - N = ~N + 1 (N odd: the +1 never leaves word 0)
  for (int k = g; k < NW; k += TPI) sq.slot[k] = k == 0 ? 0u - nw[0] : ~nw[k];
  wave_sync_mem_();
  uint32_t r1[L];
  mo.load_words(r1, sq.slot, NW);
  wave_sync_mem_();
#pragma unroll 1
  for (int d = 0; d < M::W * M::S - BITS; ++d) {
    shl_bit<M>(r1, 1u);
    mo.reduce_once(r1);
  }

  // x = 2 R (the top bit of N - 1), then one squaring per remaining bit
  uint32_t x[L];
#pragma unroll
  for (int j = 0; j < L; ++j) x[j] = r1[j];
  shl_bit<M>(x, 1u);
#pragma unroll 1
  for (int i = BITS - 2; i >= 0; --i) {
    sq.put(x);
    mo.mul(x, sq);
    const uint32_t bit = i > 0 ? (nw[i >> 5] >> (i & 31)) & 1u : 0u;  // N - 1: bit 0 cleared
    shl_bit<M>(x, bit);
  }
  mo.reduce_once(x);
  uint32_t ne = 0;
#pragma unroll
  for (int j = 0; j < L; ++j) ne |= x[j] ^ r1[j];
  const uint64_t differ = __builtin_amdgcn_ballot_w64(ne != 0);
  const uint64_t mine = ((1ull << TPI) - 1ull) << (grp * TPI);
  if (real && g == 0) pass[e] = (differ & mine) == 0 ? 1 : 0;
}

}  // namespace xhe
