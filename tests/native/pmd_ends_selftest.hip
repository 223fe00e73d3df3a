// Device self-test of k_djn_pmd's exit through the digits
// (xfl_amd/csrc/pdigit_dev.hpp pmd_exit): run on the GPU box by
// tests/test_gpu_pmd_ends.py, which passes the primes of its key as hex
// arguments (P Q).
//
// Per prime, launches of one wave (64 lanes) each run pmd_exit on states (a,
// c, Lhat) written by the host - a, c as 37 limbs with the top one unmasked,
// Lhat as the 33 words of a lane's log sum:
// 1. "forced": a = 0; a = P (u = P: an encryption cannot be steered there); a,
//    c and Lhat at the tops of their ranges (a = P + floor(2 P^2 / R), c = R +
//    4P - 1, Lhat = R - 1) alone and together; a = P with c = -R mod P (and that
//    plus P), where z lands on P - 1 before the u = P correction wraps it to 0;
//    the zero state.
// 2. "random": 256 seeded random states with a, c, Lhat anywhere in their ranges.
// Each result x (74 limbs, each below 2^28) is checked exactly against host big
// integers (hostbn.hpp): x = (R a + P c)(1 + P L) R^-2 mod P^2 with L = Lhat
// R^-2 mod P, the canonical residue below P^2.
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
constexpr int K = 37, S = 74, LANES = 64;
using D = PMD<K>;
constexpr int NQ = D::NQ, LW = D::LW, LQ = (LW + 3) / 4, TCW = (K + 3) & ~3;

// state of lane e: a at st[e][0..K), c at st[e][K..2K), Lhat at st[e][2K..2K + 4 LQ)
constexpr int SW = 2 * K + 4 * LQ;

__global__ void __launch_bounds__(64) k_exit(const uint32_t* __restrict__ P, uint32_t n0inv,
                                             const uint32_t* __restrict__ tc, const uint32_t* __restrict__ st,
                                             uint32_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t img[NQ * 256];
  __shared__ __attribute__((aligned(16))) uint32_t topc[TCW];
  const int e = threadIdx.x;
  if (e < K) topc[e] = tc[e];
  __syncthreads();
  uint32_t* slot = img + e * 4;
  D M;
  M.init(P, n0inv);
  const uint32_t* s = st + (size_t)e * SW;
  uint32_t a[K], c[K];
#pragma unroll
  for (int j = 0; j < K; ++j) a[j] = s[j], c[j] = s[K + j];
#pragma unroll
  for (int q = 0; q < LQ; ++q)
    *reinterpret_cast<uint4*>(slot + (D::EQ + q) * 256) =
        make_uint4(s[2 * K + 4 * q], s[2 * K + 4 * q + 1], s[2 * K + 4 * q + 2], s[2 * K + 4 * q + 3]);
  __builtin_amdgcn_sched_barrier(0);
  uint32_t x[S];
  pmd_exit<K>(M, a, c, slot, topc, P, x);
#pragma unroll
  for (int j = 0; j < S; ++j) out[(size_t)e * S + j] = x[j];
}

static BigU from_hex(const char* s) {
  BigU r;
  for (; *s; ++s) {
    const int d = *s >= '0' && *s <= '9' ? *s - '0' : *s >= 'a' && *s <= 'f' ? *s - 'a' + 10 : *s - 'A' + 10;
    r = add(shl(r, 4), BigU((uint64_t)d));
  }
  return r;
}
static BigU rand_below(std::mt19937_64& rng, const BigU& bound) {
  std::vector<uint32_t> w((bound.bits() + 64 + 31) / 32);
  for (auto& v : w) v = (uint32_t)rng();
  return mod(BigU::from_words(w.data(), w.size()), bound);
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

template <class T>
static T* to_dev(const std::vector<T>& v) {
  T* d = nullptr;
  hipMalloc(&d, v.size() * sizeof(T));
  hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return d;
}

struct State {
  BigU a, c, l;
};

struct PrimeCtx {
  BigU P, P2, R, Rinv2P, Rinv2P2;
  uint32_t *dP, *dtc;
  uint32_t n0inv;
};

// one wave over up to 64 states; returns the number of wrong lanes, -1 on a HIP error
static int run_wave(const PrimeCtx& cx, const std::vector<State>& sts, const char* what, int index) {
  std::vector<uint32_t> hs((size_t)LANES * SW, 0u);
  for (size_t i = 0; i < sts.size(); ++i) {
    const auto al = limbs_loose(sts[i].a, K), cl = limbs_loose(sts[i].c, K);
    memcpy(&hs[i * SW], al.data(), K * 4);
    memcpy(&hs[i * SW + K], cl.data(), K * 4);
    sts[i].l.to_words(&hs[i * SW + 2 * K], LW);
  }
  uint32_t *ds = to_dev(hs), *dout = nullptr;
  hipMalloc(&dout, (size_t)LANES * S * 4);
  hipLaunchKernelGGL(k_exit, dim3(1), dim3(LANES), 0, 0, cx.dP, cx.n0inv, cx.dtc, ds, dout);
  std::vector<uint32_t> ho((size_t)LANES * S);
  const bool ok = hipMemcpy(ho.data(), dout, ho.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
  hipFree(ds), hipFree(dout);
  if (!ok) return -1;
  int bad = 0;
  for (size_t i = 0; i < sts.size(); ++i) {
    bool good = true;
    for (int j = 0; j < S; ++j) good = good && ho[i * S + j] <= 0xFFFFFFFu;  // normalised limbs
    const BigU L = mulmod(mod(sts[i].l, cx.P), cx.Rinv2P, cx.P);
    const BigU X = add(mul(cx.R, sts[i].a), mul(cx.P, sts[i].c));
    const BigU want = mulmod(mulmod(mod(X, cx.P2), add(BigU(1), mul(cx.P, L)), cx.P2), cx.Rinv2P2, cx.P2);
    good = good && cmp(from_limbs(&ho[i * S], S), want) == 0;
    if (!good && ++bad < 4) printf("  %s prime %d lane %zu wrong\n", what, index, i);
  }
  return bad;
}

static int check_prime(const BigU& P, int index, std::mt19937_64& rng) {
  const BigU one(1);
  PrimeCtx cx;
  cx.P = P, cx.P2 = mul(P, P), cx.R = pow2(28 * K);
  const BigU RP = mod(cx.R, P), RP2 = mod(cx.R, cx.P2);
  cx.Rinv2P = modinv(mulmod(RP, RP, P), P);
  cx.Rinv2P2 = modinv(mulmod(RP2, RP2, cx.P2), cx.P2);
  std::vector<uint32_t> hP = P.to_limbs(28, K), htc = submod(one, RP, P).to_limbs(28, K);  // E = (1 - R) mod P
  hP.resize((K + 3) & ~3, 0);
  for (auto& v : htc) v += (1u << 28) - 1u;
  htc.resize(TCW, 0);
  cx.dP = to_dev(hP), cx.dtc = to_dev(htc);
  cx.n0inv = mont_ninv(P.word(0), 28);
  BigU q2;
  divmod(shl(cx.P2, 1), cx.R, &q2, nullptr);
  const BigU a_top = add(P, q2), c_top = sub(add(cx.R, shl(P, 2)), one), l_top = sub(cx.R, one);
  const BigU a_bound = add(a_top, one), c_bound = add(c_top, one);
  const BigU negR = submod(BigU(), RP, P);  // -R mod P
  int rc = 0;
  {
    std::vector<State> sts = {
        {BigU(), rand_below(rng, c_bound), rand_below(rng, cx.R)},
        {P, rand_below(rng, c_bound), rand_below(rng, cx.R)},
        {a_top, c_top, l_top},
        {a_top, BigU(), BigU()},
        {BigU(), BigU(), BigU()},
        {BigU(), c_top, l_top},
        {P, c_top, l_top},
        {P, negR, rand_below(rng, cx.R)},
        {P, add(negR, P), l_top},
        {P, BigU(), BigU()},
        {rand_below(rng, a_bound), c_top, rand_below(rng, cx.R)},
        {rand_below(rng, a_bound), rand_below(rng, c_bound), l_top},
    };
    const int bad = run_wave(cx, sts, "forced", index);
    if (bad < 0) {
      printf("{\"error\": \"hip\"}\n");
      return 2;
    }
    printf("{\"check\": \"forced\", \"prime\": %d, \"bad\": %d, \"of\": %zu}\n", index, bad, sts.size());
    rc |= bad != 0;
  }
  {
    int bad = 0, of = 0;
    for (int w = 0; w < 4; ++w) {
      std::vector<State> sts;
      for (int i = 0; i < LANES; ++i)
        sts.push_back({rand_below(rng, a_bound), rand_below(rng, c_bound), rand_below(rng, cx.R)});
      const int b = run_wave(cx, sts, "random", index);
      if (b < 0) {
        printf("{\"error\": \"hip\"}\n");
        return 2;
      }
      bad += b, of += LANES;
    }
    printf("{\"check\": \"random\", \"prime\": %d, \"bad\": %d, \"of\": %d}\n", index, bad, of);
    rc |= bad != 0;
  }
  hipFree(cx.dP), hipFree(cx.dtc);
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: pmd_ends_selftest PRIME_HEX [PRIME_HEX ...]\n");
    return 2;
  }
  std::mt19937_64 rng(1937);
  int rc = 0;
  for (int i = 1; i < argc; ++i) {
    const int r = check_prime(from_hex(argv[i]), i - 1, rng);
    if (r == 2) return 2;  // a HIP error: nothing more is started on the device
    rc |= r;
  }
  return rc;
}
