// Device self-test of the block-form Montgomery reductions at both ends of
// k_djn_pmd (xfl_amd/csrc/bn_dev.hpp Mont::red_rows): run on the GPU box by
// tests/test_gpu_redc_block.py, which passes the primes of its keys as hex
// arguments (P Q [P Q ...]).
//
// Per prime, one launch of 64 lanes each:
// 1. "redc_wide": Mont<74, 28, 1>::redc_wide(b, AZero{}) mod N = P^2, the exit
//    of k_djn_pmd, on 74-limb inputs X (top limb unmasked): v and v R mod N for
//    v = 0, 1, N - 1, N, 2N - 1; 2^15 N - 1, the bound of what to_mont2 hands
//    over; the low 37 limbs all MASK; every limb MASK below a 17-bit top limb;
//    seeded random values below 2^15 N.
// 2. "redc_p": pmd_redc_words<37>, the REDC by P of the prologue, on 65-word
//    inputs m: 0, 1, P - 1, P, R P - 1, 2^2048 - 1, the low 37 limbs all MASK,
//    seeded random values below 2^2048 and below R P.
// Each result t is checked exactly against host big integers (hostbn.hpp):
// t R - X = q M with 0 <= q < R (so t = (X + q M) / R, the Montgomery
// reduction's own value, not only its residue) and t < 2 M.
// Prints one JSON line per check and prime; exits 1 on any mismatch.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../xfl_amd/csrc/bn_dev.hpp"
#include "../../xfl_amd/csrc/hostbn.hpp"
#include "../../xfl_amd/csrc/pdigit_dev.hpp"

using namespace xhe;
constexpr int K = 37, S = 74, LANES = 64, MW = 65;
using MP = Mont<S, 28, 1>;
using MK = Mont<K, 28, 1>;
constexpr int NQ = PMD<K>::NQ;

__global__ void __launch_bounds__(64) k_redc_wide(const uint32_t* __restrict__ N, uint32_t n0inv, const uint32_t* x,
                                                  uint32_t* out) {
  const int e = threadIdx.x;
  MP M;
  M.init(N, n0inv);
  uint32_t b[S];
#pragma unroll
  for (int j = 0; j < S; ++j) b[j] = x[(size_t)e * S + j];
  M.redc_wide(b, AZero{});
#pragma unroll
  for (int j = 0; j < S; ++j) out[(size_t)e * S + j] = b[j];
}

__global__ void __launch_bounds__(64) k_redc_p(const uint32_t* __restrict__ P, uint32_t n0inv, const uint32_t* m,
                                               uint32_t* out) {
  __shared__ __attribute__((aligned(16))) uint32_t img[NQ * 256];
  const int e = threadIdx.x;
  MK M;
  M.init(P, n0inv);
  uint32_t t[K];
  pmd_redc_words<K>(M, img + e * 4, m + (size_t)e * MW, MW, t);
#pragma unroll
  for (int j = 0; j < K; ++j) out[(size_t)e * K + j] = t[j];
}

static BigU from_hex(const char* s) {
  BigU r;
  for (; *s; ++s) {
    const int d = *s >= '0' && *s <= '9' ? *s - '0' : *s >= 'a' && *s <= 'f' ? *s - 'a' + 10 : *s - 'A' + 10;
    r = add(shl(r, 4), BigU((uint64_t)d));
  }
  return r;
}
static BigU rand_big(std::mt19937_64& rng, int bits) {
  std::vector<uint32_t> w((bits + 31) / 32);
  for (auto& v : w) v = (uint32_t)rng();
  if (bits % 32) w.back() &= (1u << (bits % 32)) - 1;
  return BigU::from_words(w.data(), w.size());
}
// n limbs with the top one unmasked
static std::vector<uint32_t> limbs_loose(const BigU& a, int n) {
  std::vector<uint32_t> l(n);
  for (int j = 0; j < n; ++j) {
    const size_t bit = (size_t)28 * j, k = bit >> 5, sh = bit & 31;
    const uint64_t x = (uint64_t)a.word(k) | ((uint64_t)a.word(k + 1) << 32);
    l[j] = j + 1 < n ? (uint32_t)((x >> sh) & 0xFFFFFFFu) : (uint32_t)(x >> sh);
  }
  return l;
}
static BigU from_limbs(const uint32_t* l, int n) {
  BigU r;
  for (int j = n - 1; j >= 0; --j) r = add(shl(r, 28), BigU((uint64_t)l[j]));
  return r;
}
// t = (X + q M) / R with 0 <= q < R, and t < 2 M
static bool exact_redc(const BigU& t, const BigU& X, const BigU& M, const BigU& R) {
  const BigU tR = mul(t, R);
  if (cmp(tR, X) < 0) return false;
  BigU q, r;
  divmod(sub(tR, X), M, &q, &r);
  return r.is_zero() && cmp(q, R) < 0 && cmp(t, shl(M, 1)) < 0;
}

template <class T>
static T* to_dev(const std::vector<T>& v) {
  T* d = nullptr;
  hipMalloc(&d, v.size() * sizeof(T));
  hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return d;
}

static int check_prime(const BigU& P, int index, std::mt19937_64& rng) {
  int rc = 0;
  const BigU one(1);
  // 1. the exit REDC mod N = P^2
  {
    const BigU N = mul(P, P), R = pow2(28 * S), top = sub(shl(N, 15), one);
    std::vector<BigU> X;
    const BigU vs[5] = {BigU(), one, sub(N, one), N, sub(shl(N, 1), one)};
    for (const BigU& v : vs) X.push_back(v);
    for (const BigU& v : vs) X.push_back(mulmod(v, R, N));
    X.push_back(top);
    X.push_back(sub(pow2(28 * K), one));                   // the low half all MASK
    X.push_back(sub(pow2(28 * (S - 1) + 17), one));        // every limb MASK below a 17-bit top limb
    while ((int)X.size() < LANES) X.push_back(mod(rand_big(rng, 28 * S), shl(N, 15)));
    std::vector<uint32_t> hx, hN = N.to_limbs(28, S);
    hN.resize(MP::S4, 0);
    for (const BigU& v : X) {
      auto l = limbs_loose(v, S);
      hx.insert(hx.end(), l.begin(), l.end());
    }
    uint32_t *dN = to_dev(hN), *dx = to_dev(hx), *dout = nullptr;
    hipMalloc(&dout, hx.size() * 4);
    hipLaunchKernelGGL(k_redc_wide, dim3(1), dim3(LANES), 0, 0, dN, mont_ninv(N.word(0), 28), dx, dout);
    std::vector<uint32_t> ho(hx.size());
    if (hipMemcpy(ho.data(), dout, ho.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) {
      printf("{\"error\": \"hip\"}\n");
      return 1;
    }
    int bad = 0;
    for (int i = 0; i < LANES; ++i) {
      bool ok = true;
      for (int j = 0; j < S; ++j) ok = ok && ho[(size_t)i * S + j] <= 0xFFFFFFFu;  // normalised limbs
      ok = ok && exact_redc(from_limbs(&ho[(size_t)i * S], S), X[i], N, R);
      if (!ok && ++bad < 4) printf("  redc_wide prime %d lane %d wrong\n", index, i);
    }
    printf("{\"check\": \"redc_wide\", \"prime\": %d, \"bad\": %d, \"of\": %d}\n", index, bad, LANES);
    rc |= bad != 0;
    hipFree(dN), hipFree(dx), hipFree(dout);
  }
  // 2. the prologue's REDC by P
  {
    const BigU R = pow2(28 * K), RP = mul(R, P);
    std::vector<BigU> X = {BigU(), one, sub(P, one), P, sub(RP, one), sub(pow2(2048), one), sub(R, one)};
    while ((int)X.size() < LANES) X.push_back((X.size() & 1) ? rand_big(rng, 2048) : mod(rand_big(rng, 2080), RP));
    std::vector<uint32_t> hm((size_t)LANES * MW), hP = P.to_limbs(28, K);
    hP.resize(MK::S4, 0);
    for (int i = 0; i < LANES; ++i) X[i].to_words(&hm[(size_t)i * MW], MW);
    uint32_t *dP = to_dev(hP), *dm = to_dev(hm), *dout = nullptr;
    hipMalloc(&dout, (size_t)LANES * K * 4);
    hipLaunchKernelGGL(k_redc_p, dim3(1), dim3(LANES), 0, 0, dP, mont_ninv(P.word(0), 28), dm, dout);
    std::vector<uint32_t> ho((size_t)LANES * K);
    if (hipMemcpy(ho.data(), dout, ho.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) {
      printf("{\"error\": \"hip\"}\n");
      return 1;
    }
    int bad = 0;
    for (int i = 0; i < LANES; ++i) {
      bool ok = true;
      for (int j = 0; j < K; ++j) ok = ok && ho[(size_t)i * K + j] <= 0xFFFFFFFu;
      ok = ok && exact_redc(from_limbs(&ho[(size_t)i * K], K), X[i], P, R);
      if (!ok && ++bad < 4) printf("  redc_p prime %d lane %d wrong\n", index, i);
    }
    printf("{\"check\": \"redc_p\", \"prime\": %d, \"bad\": %d, \"of\": %d}\n", index, bad, LANES);
    rc |= bad != 0;
    hipFree(dP), hipFree(dm), hipFree(dout);
  }
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: redc_block_selftest PRIME_HEX [PRIME_HEX ...]\n");
    return 2;
  }
  std::mt19937_64 rng(1537);
  int rc = 0;
  for (int i = 1; i < argc; ++i) rc |= check_prime(from_hex(argv[i]), i - 1, rng);
  return rc;
}
