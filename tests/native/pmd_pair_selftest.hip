// Device self-test of k_djn_pmd's rows in pairs (xfl_amd/csrc/pdigit_dev.hpp
// PMD::mul_pair followed by PMD::mul): run on the GPU box by
// tests/test_gpu_pmd_pair.py, which passes the primes of its key as hex
// arguments (P Q).
//
// Per prime, launches of one wave (64 lanes) each take two row digits e1, e2 (37
// limbs each, below P) and a state (a, c) written by the host: e2 goes into the
// lane's slot as the streamed row, e1 into registers, mul_pair leaves the
// operand (a12, c12) in the slot - copied out - and mul multiplies the state by
// it. Checked exactly against host big integers (hostbn.hpp):
//     e1 e2 + m P = R a12 with m_i = topc_i - c12_i a W-bit digit, a12 in
//     normalised limbs and below P (1 + P/R);
//     R a' + P c' = (R a + P c)(R a12 + P c12) R^-2 (mod P^2), a' < P (1 + 2P/R),
//     c' < R + 4P, limbs normalised below the top one.
// 1. "pair_forced": e in {1, P - 1, R mod P, 2^1023} paired with each other, and
//    (2^1023, 2^13), whose product is R: m = 0.
// 2. "state_forced": a = 0; a, c at the tops of their ranges (a = P + floor(2 P^2
//    / R), c = R + 4P - 1) alone and together; the zero state - on random and on
//    forced pairs.
// 3. "quotient_forced": e1 e2 = 0 (mod 2^(28 k)), the low k digits of m zero, and
//    e1 e2 = P (mod 2^(28 k)), the low k digits of m all ones (MASK), for k = 1,
//    2, 18, 35, 36 (m = R - 1 whole needs e1 e2 = P mod R with both below P: not
//    constructible by this means).
// 4. "random": 256 seeded random pairs and states.
// Prints one JSON line per check and prime; exits 1 on any mismatch.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../xfl_amd/csrc/bn_dev.hpp"
#include "../../xfl_amd/csrc/hostbn.hpp"
#include "../../xfl_amd/csrc/pdigit_dev.hpp"

using namespace xhe;
constexpr int K = 37, LANES = 64;
using D = PMD<K>;
constexpr int NQ = D::NQ, TCW = (K + 3) & ~3;
constexpr uint32_t MASK = D::MASK;

// lane e: e1 at in[e][0..K), e2 at [K..2K), a at [2K..3K), c at [3K..4K)
constexpr int IW = 4 * K;
// lane e: the operand's NQ quads at out[e][0..4 NQ), a' at [4 NQ..4 NQ + K), c' after it
constexpr int OW = 4 * NQ + 2 * K;

__global__ void __launch_bounds__(64) k_pair(const uint32_t* __restrict__ P, uint32_t n0inv,
                                             const uint32_t* __restrict__ tc, const uint32_t* __restrict__ in,
                                             uint32_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t img[NQ * 256];
  __shared__ __attribute__((aligned(16))) uint32_t topc[TCW];
  const int e = threadIdx.x;
  if (e < K) topc[e] = tc[e];
  __syncthreads();
  uint32_t* slot = img + e * 4;
  D M;
  M.init(P, n0inv);
  const uint32_t* s = in + (size_t)e * IW;
  uint32_t* o = out + (size_t)e * OW;
  uint32_t r[K];
#pragma unroll
  for (int j = 0; j < K; ++j) r[j] = s[j];
#pragma unroll
  for (int q = 0; q < D::EQ; ++q)
    *reinterpret_cast<uint4*>(slot + (D::PQ + q) * 256) =
        make_uint4(4 * q < K ? s[K + 4 * q] : 0u, 4 * q + 1 < K ? s[K + 4 * q + 1] : 0u,
                   4 * q + 2 < K ? s[K + 4 * q + 2] : 0u, 4 * q + 3 < K ? s[K + 4 * q + 3] : 0u);
  __builtin_amdgcn_sched_barrier(0);
  M.mul_pair(r, slot, topc);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const uint4 v = *reinterpret_cast<const uint4*>(slot + q * 256);
    o[4 * q] = v.x, o[4 * q + 1] = v.y, o[4 * q + 2] = v.z, o[4 * q + 3] = v.w;
  }
  uint32_t a[K], c[K];
#pragma unroll
  for (int j = 0; j < K; ++j) a[j] = s[2 * K + j], c[j] = s[3 * K + j];
  __builtin_amdgcn_sched_barrier(0);
  M.mul(a, c, slot, topc);
#pragma unroll
  for (int j = 0; j < K; ++j) o[4 * NQ + j] = a[j], o[4 * NQ + K + j] = c[j];
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
// the value of n lazy limbs (any 32-bit words at weights 2^(28 j))
static BigU from_limbs(const uint32_t* l, int n) {
  BigU r;
  for (int j = n - 1; j >= 0; --j) r = add(shl(r, 28), BigU((uint64_t)l[j]));
  return r;
}
// x^-1 mod 2^bits for odd x (Newton: the correct bits double each round)
static BigU inv_pow2(const BigU& x, size_t bits) {
  const BigU m = pow2(bits);
  BigU inv(1);
  for (size_t have = 1; have < bits; have *= 2) {
    const BigU t = mod(mul(x, inv), m);                      // x inv mod 2^bits
    inv = mod(mul(inv, mod(sub(add(m, BigU(2)), t), m)), m);  // inv (2 - x inv)
  }
  return inv;
}

template <class T>
static T* to_dev(const std::vector<T>& v) {
  T* d = nullptr;
  hipMalloc(&d, v.size() * sizeof(T));
  hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return d;
}

struct Case {
  BigU e1, e2, a, c;
};

struct PrimeCtx {
  BigU P, P2, R, Rinv2P2, a12_bound, a_bound, c_bound;  // the bounds exclusive, a's scaled by R
  std::vector<uint32_t> tc;
  uint32_t *dP, *dtc;
  uint32_t n0inv;
};

// one wave over up to 64 cases; returns the number of wrong lanes, -1 on a HIP error
static int run_wave(const PrimeCtx& cx, const std::vector<Case>& cs, const char* what, int index) {
  std::vector<uint32_t> hs((size_t)LANES * IW, 0u);
  for (size_t i = 0; i < cs.size(); ++i) {
    const auto e1 = cs[i].e1.to_limbs(28, K), e2 = cs[i].e2.to_limbs(28, K);
    const auto al = limbs_loose(cs[i].a, K), cl = limbs_loose(cs[i].c, K);
    memcpy(&hs[i * IW], e1.data(), K * 4);
    memcpy(&hs[i * IW + K], e2.data(), K * 4);
    memcpy(&hs[i * IW + 2 * K], al.data(), K * 4);
    memcpy(&hs[i * IW + 3 * K], cl.data(), K * 4);
  }
  uint32_t *ds = to_dev(hs), *dout = nullptr;
  hipMalloc(&dout, (size_t)LANES * OW * 4);
  hipLaunchKernelGGL(k_pair, dim3(1), dim3(LANES), 0, 0, cx.dP, cx.n0inv, cx.dtc, ds, dout);
  std::vector<uint32_t> ho((size_t)LANES * OW);
  const bool ok = hipMemcpy(ho.data(), dout, ho.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
  hipFree(ds), hipFree(dout);
  if (!ok) return -1;
  int bad = 0;
  for (size_t i = 0; i < cs.size(); ++i) {
    const uint32_t* o = &ho[i * OW];
    bool good = true;
    uint32_t a12[K], c12[K], m[K];
    for (int j = 0; j < K; ++j) {
      a12[j] = o[4 * (j >> 1) + 2 * (j & 1)];
      c12[j] = o[4 * (j >> 1) + 2 * (j & 1) + 1];
      m[j] = cx.tc[j] - c12[j];
      good = good && a12[j] <= MASK && m[j] <= MASK && c12[j] < (1u << 29);
    }
    const BigU A12 = from_limbs(a12, K), C12 = from_limbs(c12, K), Mq = from_limbs(m, K);
    good = good && cmp(add(mul(cs[i].e1, cs[i].e2), mul(Mq, cx.P)), mul(cx.R, A12)) == 0;
    good = good && cmp(mul(A12, cx.R), cx.a12_bound) < 0;
    const uint32_t *an = o + 4 * NQ, *cn = o + 4 * NQ + K;
    for (int j = 0; j + 1 < K; ++j) good = good && an[j] <= MASK && cn[j] <= MASK;
    const BigU A = from_limbs(an, K), C = from_limbs(cn, K);
    const BigU X = mod(add(mul(cx.R, cs[i].a), mul(cx.P, cs[i].c)), cx.P2);
    const BigU Y = mod(add(mul(cx.R, A12), mul(cx.P, C12)), cx.P2);
    const BigU want = mulmod(mulmod(X, Y, cx.P2), cx.Rinv2P2, cx.P2);
    good = good && cmp(mod(add(mul(cx.R, A), mul(cx.P, C)), cx.P2), want) == 0;
    good = good && cmp(mul(A, cx.R), cx.a_bound) < 0 && cmp(C, cx.c_bound) < 0;
    if (!good && ++bad < 4) printf("  %s prime %d lane %zu wrong\n", what, index, i);
  }
  return bad;
}

static int report(const PrimeCtx& cx, const std::vector<Case>& cs, const char* what, int index, int& rc) {
  int bad = 0;
  for (size_t off = 0; off < cs.size(); off += LANES) {
    const std::vector<Case> part(cs.begin() + off, cs.begin() + std::min(cs.size(), off + LANES));
    const int b = run_wave(cx, part, what, index);
    if (b < 0) {
      printf("{\"error\": \"hip\"}\n");
      return 2;
    }
    bad += b;
  }
  printf("{\"check\": \"%s\", \"prime\": %d, \"bad\": %d, \"of\": %zu}\n", what, index, bad, cs.size());
  rc |= bad != 0;
  return 0;
}

static int check_prime(const BigU& P, int index, std::mt19937_64& rng) {
  const BigU one(1);
  PrimeCtx cx;
  cx.P = P, cx.P2 = mul(P, P), cx.R = pow2(28 * K);
  const BigU RP = mod(cx.R, P), RP2 = mod(cx.R, cx.P2);
  cx.Rinv2P2 = modinv(mulmod(RP2, RP2, cx.P2), cx.P2);
  cx.a12_bound = add(mul(P, cx.R), cx.P2);           // a12 R < P R + P^2
  cx.a_bound = add(mul(P, cx.R), shl(cx.P2, 1));     // a' R < P R + 2 P^2
  cx.c_bound = add(cx.R, shl(P, 2));                 // c' < R + 4P
  std::vector<uint32_t> hP = P.to_limbs(28, K);
  cx.tc = submod(one, RP, P).to_limbs(28, K);  // E = (1 - R) mod P
  hP.resize((K + 3) & ~3, 0);
  for (auto& v : cx.tc) v += MASK;
  cx.tc.resize(TCW, 0);
  cx.dP = to_dev(hP), cx.dtc = to_dev(cx.tc);
  cx.n0inv = mont_ninv(P.word(0), 28);
  BigU q2;
  divmod(shl(cx.P2, 1), cx.R, &q2, nullptr);
  const BigU a_top = add(P, q2), c_top = sub(cx.c_bound, one);
  const BigU a_rb = add(a_top, one);
  auto rnd_e = [&]() { return rand_below(rng, P); };
  auto rnd_a = [&]() { return rand_below(rng, a_rb); };
  auto rnd_c = [&]() { return rand_below(rng, cx.c_bound); };
  const std::vector<BigU> forced = {one, sub(P, one), RP, pow2(1023)};
  int rc = 0;
  {
    std::vector<Case> cs;
    for (const auto& x : forced)
      for (const auto& y : forced) cs.push_back({x, y, rnd_a(), rnd_c()});
    cs.push_back({pow2(1023), pow2(13), rnd_a(), rnd_c()});  // e1 e2 = R: m = 0
    cs.push_back({pow2(13), pow2(1023), rnd_a(), rnd_c()});
    if (report(cx, cs, "pair_forced", index, rc)) return 2;
  }
  {
    const std::vector<std::pair<BigU, BigU>> states = {
        {BigU(), rnd_c()}, {a_top, c_top}, {a_top, BigU()}, {BigU(), BigU()}, {BigU(), c_top}, {rnd_a(), c_top},
        {a_top, rnd_c()}};
    std::vector<Case> cs;
    for (const auto& st : states) {
      cs.push_back({rnd_e(), rnd_e(), st.first, st.second});
      cs.push_back({forced[1], forced[1], st.first, st.second});
      cs.push_back({forced[0], forced[3], st.first, st.second});
      cs.push_back({forced[2], forced[1], st.first, st.second});
    }
    if (report(cx, cs, "state_forced", index, rc)) return 2;
  }
  {
    std::vector<Case> cs;
    for (int k : {1, 2, 18, 35, 36}) {
      const size_t bits = (size_t)28 * k;
      const BigU m2 = pow2(bits), hi_bound = pow2(1020 - bits);  // every e below 2^1020 < P
      // the low k digits of m zero: e1 e2 = 0 (mod 2^bits)
      const size_t h1 = bits / 2, h2 = bits - h1;
      const BigU r1 = rand_below(rng, pow2(1020 - h1)), r2 = rand_below(rng, pow2(1020 - h2));
      cs.push_back({shl(r1, h1), shl(r2, h2), rnd_a(), rnd_c()});
      // the low k digits of m all ones: e1 e2 = P (mod 2^bits), e2 odd
      BigU e2 = rnd_e();
      if (!(e2.word(0) & 1u)) e2 = add(e2, one);
      if (cmp(e2, P) >= 0) e2 = sub(e2, BigU(2));
      const BigU lo = mod(mul(mod(P, m2), inv_pow2(mod(e2, m2), bits)), m2);
      const BigU e1 = add(lo, shl(rand_below(rng, hi_bound), bits));
      cs.push_back({e1, e2, rnd_a(), rnd_c()});
      cs.push_back({e2, e1, a_top, c_top});
    }
    if (report(cx, cs, "quotient_forced", index, rc)) return 2;
  }
  {
    std::vector<Case> cs;
    for (int i = 0; i < 4 * LANES; ++i) cs.push_back({rnd_e(), rnd_e(), rnd_a(), rnd_c()});
    if (report(cx, cs, "random", index, rc)) return 2;
  }
  hipFree(cx.dP), hipFree(cx.dtc);
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: pmd_pair_selftest PRIME_HEX [PRIME_HEX ...]\n");
    return 2;
  }
  std::mt19937_64 rng(2401);
  int rc = 0;
  for (int i = 1; i < argc; ++i) {
    const int r = check_prime(from_hex(argv[i]), i - 1, rng);
    if (r == 2) return 2;  // a HIP error: nothing more is started on the device
    rc |= r;
  }
  return rc;
}
