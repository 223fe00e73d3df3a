// k_modinv: modular inverse mod n^2 on the device, one wavefront per value
// (the root of the batch-inversion product tree, xhe_invert_dev).
//
// Bernstein-Yang divsteps ("safegcd") on (delta, f, g), f = n^2 (odd), g = x:
//   delta > 0 and g odd:  (delta, f, g) <- (1 - delta, g, (g - f) / 2)
//   otherwise:            (delta, f, g) <- (1 + delta, f, (g + (g mod 2) f) / 2)
// in batches of kModinvBatch = 30 steps. A batch reads only the low word of f
// and g, which every lane holds after a readfirstlane, so the 30 dependent
// steps are wave-uniform scalar work; they yield a matrix (u, v; q, r) with
// |u| + |v| <= 2^30 and |q| + |r| <= 2^30 (int32), and
//   (f, g) <- (u f + v g, q f + r g) / 2^30                        exactly,
//   (d, e) <- (u d + v e + md n^2, q d + r e + me n^2) / 2^30      exactly,
// md, me chosen from the low words and (n^2)^-1 mod 2^30 (Newton steps from
// the modulus's low word). d x = f and e x = g (mod n^2) hold throughout and
// d, e stay in (-2 n^2, n^2), so when g = 0, f = +-gcd(x, n^2) and, for a
// unit, sign(f) d is the inverse.
//
// Layout: f, g, d, e and n^2 are two's-complement numbers of T = 64 LPL words,
// LPL = ceil((n2w + 1) / 64), lane l holding words [l LPL, (l + 1) LPL) in
// registers. n2w is a multiple of 64, so T >= n2w + 64: the words past n2w are
// sign extension, and no intermediate (below 2^32 n^2 in magnitude) comes
// near 2^(32 T - 1). A linear combination sum_i a_i X_i mod 2^(32 T) with
// signed wave-uniform a_i is |a_i| (X_i or ~X_i) per word plus sum |a_i| over
// the negated terms entering at word 0 (-X = ~X + 1): every product and every
// carry is non-negative. Per lane: multiply-adds into a 64-bit accumulator
// with a local carry chain; the lane's carry-out (below 2^32) goes to the
// next lane, whose add of it can carry once more, and that last binary carry
// is resolved exactly across the wave from two ballot masks (generate: the
// add overflowed; propagate: the lane's words are all ones) by one 64-bit
// addition, carries = (G | P) + G xor (G | P) xor G. Then the shift by 30
// bits, one word from the lane above.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xhe {

constexpr int kModinvBatch = 30;

// Batches that cover the Bernstein-Yang bound floor((49 b + 57) / 17) on the
// divsteps of b-bit operands (b = 32 n2w >= 46); units finish long before.
inline int modinv_max_batches(int n2w) {
  const int64_t b = 32 * (int64_t)n2w;
  return (int)(((49 * b + 57) / 17 + kModinvBatch - 1) / kModinvBatch);
}
constexpr int modinv_lpl(int n2w) { return (n2w + 1 + 63) / 64; }

__device__ __forceinline__ uint32_t mi_lane0(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
// sign mask (0 or -1) of a number: its top word sits in lane 63
__device__ __forceinline__ int32_t mi_sign(uint32_t top) { return (int32_t)__builtin_amdgcn_readlane(top, 63) >> 31; }

// out = (a A + b B [+ c C]) mod 2^(32 T), shifted right by 30 bits when SHIFT
// (the caller guarantees the 30 low bits are zero). |a| + |b| <= 2^30 and
// |c| < 2^31: a word's sum stays below 3 2^62 + 2^32. out must not alias an
// operand the caller still needs; it may alias A, B or C.
template <int LPL, bool SHIFT, bool T3>
__device__ __forceinline__ void mi_lin(uint32_t (&out)[LPL], const uint32_t (&A)[LPL], int32_t a,
                                       const uint32_t (&B)[LPL], int32_t b, const uint32_t (&C)[LPL], int32_t c,
                                       int lane) {
  const uint32_t ma = a < 0 ? ~0u : 0u, mb = b < 0 ? ~0u : 0u, mc = c < 0 ? ~0u : 0u;
  const uint32_t ua = a < 0 ? 0u - (uint32_t)a : (uint32_t)a, ub = b < 0 ? 0u - (uint32_t)b : (uint32_t)b,
                 uc = c < 0 ? 0u - (uint32_t)c : (uint32_t)c;
  uint32_t x[LPL];
  uint64_t t = 0;
#pragma unroll
  for (int j = 0; j < LPL; ++j) {
    t += (uint64_t)ua * (A[j] ^ ma) + (uint64_t)ub * (B[j] ^ mb);
    if constexpr (T3) t += (uint64_t)uc * (C[j] ^ mc);
    x[j] = (uint32_t)t;
    t >>= 32;
  }
  // the lane below's carry-out (< 2^32); lane 0 takes the +1s of the negated terms
  uint32_t cin = __shfl_up((uint32_t)t, 1, 64);
  if (lane == 0) cin = (ua & ma) + (ub & mb) + (T3 ? (uc & mc) : 0u);
  t = cin;
  uint32_t ones = ~0u;
#pragma unroll
  for (int j = 0; j < LPL; ++j) {
    t += x[j];
    x[j] = (uint32_t)t;
    t >>= 32;
    ones &= x[j];
  }
  const uint64_t G = __ballot(t != 0);
  const uint64_t P = __ballot(ones == ~0u) & ~G;
  const uint64_t carries = ((G | P) + G) ^ (G | P) ^ G;  // bit l: the carry into lane l
  t = (carries >> lane) & 1;
#pragma unroll
  for (int j = 0; j < LPL; ++j) {
    t += x[j];
    x[j] = (uint32_t)t;
    t >>= 32;
  }
  if constexpr (SHIFT) {
    uint32_t up = __shfl_down(x[0], 1, 64);
    if (lane == 63) up = (uint32_t)((int32_t)x[LPL - 1] >> 31);
#pragma unroll
    for (int j = 0; j < LPL; ++j) {
      const uint32_t hi = j + 1 < LPL ? x[j + 1] : up;
      out[j] = (x[j] >> kModinvBatch) | (hi << (32 - kModinvBatch));
    }
  } else {
#pragma unroll
    for (int j = 0; j < LPL; ++j) out[j] = x[j];
  }
}

// status[0] = 0 ahead of a call's k_modinv, which only ever raises it
__global__ void k_modinv_clear(int32_t* __restrict__ status) {
  if (blockIdx.x == 0 && threadIdx.x == 0) status[0] = 0;
}

// out[i] = in[i]^-1 mod n^2, rows of n2w words, in[i] < 2^(32 n2w); one
// 64-lane block per row. A row without an inverse is written as zeros and
// status[0] becomes 1. n2: the n2w words of n^2 in device memory.
template <int LPL>
__global__ void __launch_bounds__(64) k_modinv(const uint32_t* __restrict__ n2, int n2w,
                                               const uint32_t* __restrict__ in, int64_t count,
                                               uint32_t* __restrict__ out, int32_t* __restrict__ status,
                                               int max_batches) {
  const int64_t row = blockIdx.x;
  if (row >= count) return;
  const int lane = threadIdx.x;
  uint32_t M[LPL], F[LPL], G[LPL], D[LPL], E[LPL];
#pragma unroll
  for (int j = 0; j < LPL; ++j) {
    const int w = lane * LPL + j;
    M[j] = w < n2w ? n2[w] : 0u;
    G[j] = w < n2w ? in[(size_t)row * n2w + w] : 0u;
    F[j] = M[j];
    D[j] = 0u;
    E[j] = w == 0 ? 1u : 0u;
  }
  constexpr uint32_t kMask = (1u << kModinvBatch) - 1;
  const uint32_t m0 = mi_lane0(M[0]);
  uint32_t minv = m0;  // m0 m0 = 1 mod 8; each Newton step doubles the bits: 3, 6, 12, 24, 48
  for (int i = 0; i < 4; ++i) minv *= 2u - m0 * minv;
  int32_t delta = 1;
  for (int batch = 0; batch < max_batches; ++batch) {
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < LPL; ++j) any |= G[j];
    if (__ballot(any != 0) == 0) break;
    // 30 divsteps on the low words: wave-uniform
    uint32_t f = mi_lane0(F[0]), g = mi_lane0(G[0]);
    int32_t u = 1, v = 0, q = 0, r = 1;
    for (int i = 0; i < kModinvBatch; ++i) {
      if (g & 1) {
        if (delta > 0) {
          delta = 1 - delta;
          const uint32_t f1 = g;
          g = (g - f) >> 1;
          f = f1;
          const int32_t u1 = q + q, v1 = r + r;
          q -= u;
          r -= v;
          u = u1;
          v = v1;
        } else {
          ++delta;
          g = (g + f) >> 1;
          q += u;
          r += v;
          u += u;
          v += v;
        }
      } else {
        ++delta;
        g >>= 1;
        u += u;
        v += v;
      }
    }
    // d, e in (-2 n^2, n^2): a negative one counts as itself + n^2 (sd, se),
    // then the multiple of n^2 in [0, 2^30) that clears the 30 low bits
    const int32_t sd = mi_sign(D[LPL - 1]), se = mi_sign(E[LPL - 1]);
    const uint32_t d0 = mi_lane0(D[0]), e0 = mi_lane0(E[0]);
    int32_t md = (u & sd) + (v & se), me = (q & sd) + (r & se);
    const uint32_t cd = (uint32_t)u * d0 + (uint32_t)v * e0, ce = (uint32_t)q * d0 + (uint32_t)r * e0;
    md -= (int32_t)((minv * cd + (uint32_t)md) & kMask);
    me -= (int32_t)((minv * ce + (uint32_t)me) & kMask);
    uint32_t nf[LPL], nd[LPL];
    mi_lin<LPL, true, false>(nf, F, u, G, v, M, 0, lane);
    mi_lin<LPL, true, false>(G, F, q, G, r, M, 0, lane);
    mi_lin<LPL, true, true>(nd, D, u, E, v, M, md, lane);
    mi_lin<LPL, true, true>(E, D, q, E, r, M, me, lane);
#pragma unroll
    for (int j = 0; j < LPL; ++j) {
      F[j] = nf[j];
      D[j] = nd[j];
    }
  }
  // g = 0 and f = 1 or -1, else no inverse
  uint32_t gany = 0, fone = lane == 0 ? F[0] ^ 1u : F[0], fneg = ~F[0];
#pragma unroll
  for (int j = 0; j < LPL; ++j) gany |= G[j];
#pragma unroll
  for (int j = 1; j < LPL; ++j) {
    fone |= F[j];
    fneg |= ~F[j];
  }
  const bool is_one = __ballot(fone != 0) == 0, is_neg = __ballot(fneg != 0) == 0;
  const bool ok = __ballot(gany != 0) == 0 && (is_one || is_neg);
  uint32_t R[LPL], S[LPL];
  if (ok) {
    mi_lin<LPL, false, false>(R, D, is_neg ? -1 : 1, M, 0, M, 0, lane);  // in (-2 n^2, 2 n^2)
    for (int i = 0; i < 2; ++i) mi_lin<LPL, false, false>(R, R, 1, M, mi_sign(R[LPL - 1]) & 1, M, 0, lane);
    mi_lin<LPL, false, false>(S, R, 1, M, -1, M, 0, lane);  // R in [0, 2 n^2): R - n^2 where that is >= 0
    const bool sub = mi_sign(S[LPL - 1]) == 0;
#pragma unroll
    for (int j = 0; j < LPL; ++j) R[j] = sub ? S[j] : R[j];
  } else {
#pragma unroll
    for (int j = 0; j < LPL; ++j) R[j] = 0u;
    if (lane == 0) status[0] = 1;
  }
#pragma unroll
  for (int j = 0; j < LPL; ++j) {
    const int w = lane * LPL + j;
    if (w < n2w) out[(size_t)row * n2w + w] = R[j];
  }
}

}  // namespace xhe
