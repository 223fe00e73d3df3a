// Host-only derivation of a key's constants: the words of the constant blob
// and the KeyDev that points into it (keydev.hpp). Pure integer arithmetic on
// hostbn.hpp: no HIP runtime call, no environment, so it runs (and is tested,
// tests/test_keyconst.py) on any machine. xhe.hip uploads the words and binds
// the KeyDev to the device address.
//
// Every constant is stored together with the KeyDev field that will point at
// it (KeyImage::put*), so a constant cannot be stored without being bound and
// a field never stored stays null. The order of the put calls is the blob's
// layout (alignment, which constants share cache lines): append only, inside
// a family - the blob ends with a constant tests/native/keyconst_check.cpp
// names (tests/test_keyconst.py test_presence), so a new family goes before
// the last put of n2_constants, as k_enc_obf's did.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "hostbn.hpp"
#include "keydev.hpp"
#include "rns_layout.hpp"

namespace xhe {

struct ModSpec {
  int S, W;  // S limbs of W bits
  int S4() const { return (S + 3) & ~3; }
  BigU R() const { return pow2((size_t)W * S); }  // the shape's Montgomery factor 2^(W S)
};

// Everything the derivation needs besides the key's integers: the limb shapes
// of the kernels that will read the constants (xhe.hip fills them from the
// kernels' template types). The 2048-bit-only and 3072+-only shapes are zero
// where they do not apply.
struct KeySpec {
  int K;  // key bits: 2048, 3072, 4096 or 8192
  bool priv, djn;
  ModSpec mp2, mp2L, mp2X;  // residues mod p^2, q^2: batch, 4-lane and 16-lane shapes
  ModSpec mp;               // mod p, q
  ModSpec mn2, mn2X;        // mod n^2: batch and 16-lane shapes
  ModSpec nd;    // 2048: Montgomery digits mod n^2 (limbs of n)
  ModSpec pmd;   // 2048: one-lane Montgomery digits mod P^2 (limbs of P; the mod-p shape)
  ModSpec wave;  // 2048: the one-block n^2 products (WaveMont)
  ModSpec bar;   // 2048: Barrett reduction mod n^2 (limbs of n^2)
  ModSpec pd;    // 3072+: Montgomery digits mod P^2 (limbs of P)
  int win;       // fixed-base window bits (DJN keys)
  bool split;    // private DJN keys: the split window layout (win_layout)
  int nw() const { return K / 32; }
  int n2w() const { return K / 16; }
};

// Window layout of a fixed-base table over rand_bits exponent bits: uniform
// ceil(rand_bits/win) windows, or (split) floor(rand_bits/win) windows of
// which the first rand_bits mod win are win+1 bits wide (KeyDev::nhi).
inline void win_layout(int rand_bits, int win, bool split, int* nwin, int* nhi) {
  *nwin = (rand_bits + win - 1) / win;
  *nhi = 0;
  if (split && rand_bits % win != 0 && rand_bits % win <= rand_bits / win) {
    *nwin = rand_bits / win;
    *nhi = rand_bits % win;
  }
}

// ---- RNS small-batch decrypt constants (rns_dev.hpp k_dec_rns; checked
// against tools/rns_model.py, which builds the same bases)
namespace rnsh {
inline bool prime32(uint32_t n) {  // deterministic Miller-Rabin for n < 2^32
  if (n < 2) return false;
  for (uint32_t p : {2u, 3u, 5u, 7u})
    if (n % p == 0) return n == p;
  uint32_t d = n - 1;
  int r = 0;
  while (!(d & 1)) d >>= 1, ++r;
  for (uint64_t a : {2ull, 3ull, 5ull, 7ull}) {
    uint64_t x = 1, b = a, e = d;
    while (e) {
      if (e & 1) x = x * b % n;
      b = b * b % n;
      e >>= 1;
    }
    if (x == 1 || x == n - 1) continue;
    bool ok = false;
    for (int i = 1; i < r && !ok; ++i) {
      x = x * x % n;
      ok = x == n - 1;
    }
    if (!ok) return false;
  }
  return true;
}
inline uint32_t inv_mod(uint32_t a, uint32_t m) {  // a^-1 mod m (gcd = 1)
  int64_t t0 = 0, t1 = 1, r0 = m, r1 = a % m;
  while (r1) {
    const int64_t q = r0 / r1;
    std::swap(r0, r1);
    r1 -= q * r0;
    std::swap(t0, t1);
    t1 -= q * t0;
  }
  return (uint32_t)((t0 % (int64_t)m + m) % m);
}
inline uint32_t inv_2_32(uint32_t a) {  // odd a
  uint32_t x = a;
  for (int i = 0; i < 5; ++i) x *= 2u - a * x;
  return x;
}
inline uint32_t shoup_const(uint32_t w, uint32_t m) {  // floor(w 2^32 / m), w < m
  return (uint32_t)(((uint64_t)w << 32) / m);
}
inline uint32_t mod_small(const BigU& x, uint32_t m) {  // m = 0: mod 2^32
  if (m == 0) return x.word(0);
  uint64_t r = 0;
  for (size_t k = x.w.size(); k-- > 0;) r = ((r << 32) | x.w[k]) % m;
  return (uint32_t)r;
}
struct Bases {
  std::vector<uint32_t> b, b2;  // B and B' (the 2 RK largest primes below 2^28, interleaved)
  BigU M, M2;
  std::vector<BigU> Mi, M2j;
  std::vector<uint32_t> shared;  // the S_* block
};
inline const Bases& bases() {
  static const Bases B = [] {
    using namespace rns;
    Bases r;
    std::vector<uint32_t> pr;
    for (uint32_t c = (1u << 28) - 1; (int)pr.size() < 2 * RK; c -= 2)
      if (prime32(c)) pr.push_back(c);
    for (int i = 0; i < 2 * RK; ++i) (i % 2 ? r.b2 : r.b).push_back(pr[i]);
    r.M = BigU(1);
    r.M2 = BigU(1);
    for (int i = 0; i < RK; ++i) {
      r.M = mul(r.M, BigU(r.b[i]));
      r.M2 = mul(r.M2, BigU(r.b2[i]));
    }
    for (int i = 0; i < RK; ++i) {
      BigU q;
      divmod(r.M, BigU(r.b[i]), &q, nullptr);
      r.Mi.push_back(q);
      divmod(r.M2, BigU(r.b2[i]), &q, nullptr);
      r.M2j.push_back(q);
    }
    std::vector<uint32_t>& s = r.shared;
    s.assign(S_WORDS, 0u);
    for (int slot = 0; slot < NSLOT; ++slot) {  // slot = 80 base + channel; B' channel RCH is r
      const bool gB = slot < 80;
      const int ch = gB ? slot : slot - 80;
      const bool isr = !gB && ch == RCH;
      if (!(ch < RK || isr)) continue;
      const uint32_t m = isr ? 0u : (gB ? r.b[ch] : r.b2[ch]);
      if (m) {
        s[S_M + slot] = m;
        s[S_MU + slot] = (uint32_t)((1ull << 59) / m);
        s[S_T32 + slot] = (uint32_t)((1ull << 32) % m);
      }
      for (int i = 0; i < RK; ++i)  // B: |M'_j|_(m_i); B': |M_i|_(m'_j); 2^32: |M_i|_(2^32)
        s[S_ROWS + i * NSLOT + slot] = gB ? mod_small(r.M2j[i], m) : mod_small(r.Mi[i], m);
      if (gB) {
        s[S_B + slot] = mod_small(r.M2, m);                       // |M'|_(m_i)
        s[S_C + slot] = inv_mod(mod_small(r.Mi[ch], m), m);        // |M_i^-1|_(m_i)
      } else if (!isr) {
        const uint64_t minv = inv_mod(mod_small(r.M, m), m);
        s[S_B + slot] = (uint32_t)minv;                                               // |M^-1|_(m'_j)
        s[S_C + slot] = (uint32_t)(minv * inv_mod(mod_small(r.M2j[ch], m), m) % m);  // |M^-1 M'_j^-1|_(m'_j)
        s[S_D + slot] = r.M2j[ch].word(0);                                            // |M'_j|_(2^32)
      } else {
        s[S_B + slot] = inv_2_32(r.M.word(0));  // M^-1 mod 2^32
      }
      if (m) {
        s[S_BS + slot] = shoup_const(s[S_B + slot], m);
        s[S_CS + slot] = shoup_const(s[S_C + slot], m);
      }
    }
    for (int i = 0; i < RK; ++i) {
      const std::vector<uint32_t> l = r.Mi[i].to_limbs(28, RKP);
      for (int c = 0; c < RKP; ++c) s[S_MPOS + i * RKP + c] = l[c];
    }
    const std::vector<uint32_t> lm = r.M.to_limbs(28, RKP);
    for (int c = 0; c < RKP; ++c) s[S_MFULL + c] = lm[c];
    s[S_M2RINV] = inv_2_32(r.M2.word(0));
    return r;
  }();
  return B;
}
// the per-prime block for N = P^2: |-N^-1 M_i^-1| (B), |N M^-1| and |N M^-1
// M'_j^-1| (B'), N mod 2^32; M^3 mod N in every channel; and the exponent P - 1
// as the kernel's sliding-window schedule (5-bit windows, the rule of
// pow_uniform_exp: each window ends in a set bit)
inline std::vector<uint32_t> prime_block(const BigU& P) {
  using namespace rns;
  const Bases& b = bases();
  const BigU N = mul(P, P);
  std::vector<uint32_t> v(P_WORDS, 0u);
  const BigU MN = mod(b.M, N);
  const BigU M3 = mulmod(mulmod(MN, MN, N), MN, N);
  for (int slot = 0; slot < NSLOT; ++slot) {
    const bool gB = slot < 80;
    const int ch = gB ? slot : slot - 80;
    const bool isr = !gB && ch == RCH;
    if (!(ch < RK || isr)) continue;
    const uint32_t m = isr ? 0u : (gB ? b.b[ch] : b.b2[ch]);
    if (gB) {
      const uint64_t ni = inv_mod(mod_small(N, m), m), mi = inv_mod(mod_small(b.Mi[ch], m), m);
      v[P_A + slot] = (uint32_t)((m - ni * mi % m) % m);
    } else if (!isr) {
      const uint64_t nm = (uint64_t)mod_small(N, m) * inv_mod(mod_small(b.M, m), m) % m;
      v[P_A + slot] = (uint32_t)nm;
      v[P_A2 + slot] = (uint32_t)(nm * inv_mod(mod_small(b.M2j[ch], m), m) % m);
      v[P_A2S + slot] = shoup_const(v[P_A2 + slot], m);
    } else {
      v[P_A + slot] = N.word(0);
    }
    if (m) v[P_AS + slot] = shoup_const(v[P_A + slot], m);
    v[P_M3 + slot] = mod_small(M3, m);
  }
  // schedule over e = P - 1 (bits high to low)
  const BigU e = sub(P, BigU(1));
  const int nb = (int)e.bits();
  auto bit = [&](int i) { return (e.word((size_t)i / 32) >> (i % 32)) & 1u; };  // i: from the bottom
  auto window = [&](int hi, int* lo_out) {  // the window from bit hi down (at most 5 bits, ends in a set bit)
    int lo = std::max(hi - 4, 0);
    while (!bit(lo)) ++lo;
    uint32_t val = 0;
    for (int i = hi; i >= lo; --i) val = val << 1 | bit(i);
    *lo_out = lo;
    return val;
  };
  int ns = 0, lo;
  const uint32_t first = window(nb - 1, &lo);
  v[P_SCHED + ns++] = (first - 1) / 2;
  int i = lo - 1;
  uint32_t sq = 0;
  while (i >= 0) {
    if (!bit(i)) {
      ++sq;
      --i;
      continue;
    }
    const uint32_t w = window(i, &lo);
    sq += (uint32_t)(i - lo + 1);
    if (ns >= P_SCHED_MAX) throw std::runtime_error("rns schedule overflow");
    v[P_SCHED + ns++] = sq << 8 | ((w - 1) / 2 + 1);
    sq = 0;
    i = lo - 1;
  }
  if (sq) {
    if (ns >= P_SCHED_MAX) throw std::runtime_error("rns schedule overflow");
    v[P_SCHED + ns++] = sq << 8;
  }
  v[P_NS] = (uint32_t)ns;
  return v;
}
}  // namespace rnsh

// ------------------------------------------------------------------ image
using RowF = const uint32_t* KeyDev::*;  // a row of words or limbs
using PairF = const uint2* KeyDev::*;    // a row of digit pairs
using ModF = ModDev KeyDev::*;
using IntF = int KeyDev::*;

// Where a stored constant's address goes: a KeyDev pointer field, a pointer
// of one of its ModDevs, or (the table bases, which no kernel reads after key
// creation) a word offset kept by the host.
struct Dst {
  RowF w = nullptr;
  PairF d = nullptr;
  ModF m = nullptr;
  const uint32_t* ModDev::*mw = nullptr;
  size_t* off = nullptr;
  Dst(RowF f) : w(f) {}
  Dst(PairF f) : d(f) {}
  Dst(ModF mod, const uint32_t* ModDev::*f) : m(mod), mw(f) {}
  Dst(size_t* o) : off(o) {}
};

// A derived key: the blob's words, the (field, word offset) bindings and the
// scalar fields. bind() resolves the bindings against the blob's address.
struct KeyImage {
  std::vector<uint32_t> words;
  KeyDev kd{};  // scalars as derived, every pointer null (see bind)
  int rand_bits = 0, rand_words = 0;
  size_t hM_n2 = 0, hM_p2[2] = {0, 0};  // fixed-base table bases h R mod n^2 (public DJN), mod p^2 / q^2 (private)
  // 2048-bit private DJN keys: h^-1 R mod p / q in the digit limbs (a row of
  // S4 words each), the base of the chains k_tab_to_pmd takes the rows'
  // inverses from. Needed only while the tables are built: not in the blob.
  std::vector<uint32_t> hinvM_p[2];

  // rows start 16-byte aligned: every constant is padded to a multiple of 4 words
  void put(const std::vector<uint32_t>& v, Dst dst, size_t min_words = 0) {
    const size_t off = words.size();
    const size_t len = (std::max(v.size(), min_words) + 3) & ~(size_t)3;
    words.resize(off + len, 0u);
    std::copy(v.begin(), v.end(), words.begin() + off);
    if (dst.off) *dst.off = off;
    else binds.push_back({dst, off});
  }
  void put_limbs(const BigU& x, const ModSpec& s, Dst dst) { put(x.to_limbs(s.W, s.S), dst, s.S4()); }
  void put_words(const BigU& x, int nw, Dst dst) {
    std::vector<uint32_t> v(nw);
    x.to_words(v.data(), nw);
    put(v, dst);
  }
  // A whole modulus. npow > 0 also stores R^j mod M for j < npow (consecutive
  // rows of S4 limbs): the fix-up factors of chains over plain residues
  // (k_chunk_prod, raw inputs)
  void put_mod(const BigU& M, const ModSpec& s, ModF m, int npow = 0) {
    const BigU R1 = mod(s.R(), M), R2 = mulmod(R1, R1, M), R3 = mulmod(R2, R1, M);
    put_limbs(M, s, {m, &ModDev::N});
    put_limbs(R1, s, {m, &ModDev::R1});
    put_limbs(R2, s, {m, &ModDev::R2});
    put_limbs(R3, s, {m, &ModDev::R3});
    (kd.*m).n0inv = mont_ninv(M.word(0), s.W);
    if (npow <= 0) return;
    std::vector<uint32_t> rows((size_t)npow * s.S4(), 0u);
    BigU x = mod(BigU(1), M);
    for (int j = 0; j < npow; ++j) {
      const std::vector<uint32_t> l = x.to_limbs(s.W, s.S);
      std::copy(l.begin(), l.end(), rows.begin() + (size_t)j * s.S4());
      x = mulmod(x, R1, M);
    }
    put(rows, {m, &ModDev::Rpow});
  }

  KeyDev bind(const uint32_t* base) const {
    KeyDev r = kd;
    for (const Binding& b : binds) {
      const uint32_t* p = base + b.off;
      if (b.dst.w) r.*b.dst.w = p;
      else if (b.dst.d) r.*b.dst.d = reinterpret_cast<const uint2*>(p);
      else (r.*b.dst.m).*b.dst.mw = p;
    }
    return r;
  }

 private:
  struct Binding {
    Dst dst;
    size_t off;
  };
  std::vector<Binding> binds;
};

// The KeyDev fields that exist once per prime: [0] for P, [1] for Q.
namespace pq {
constexpr ModF m2[2] = {&KeyDev::p2, &KeyDev::q2}, m2L[2] = {&KeyDev::p2L, &KeyDev::q2L},
               m2X[2] = {&KeyDev::p2X, &KeyDev::q2X}, m1[2] = {&KeyDev::p, &KeyDev::q},
               dm[2] = {&KeyDev::dp, &KeyDev::dq};
constexpr RowF nprime[2] = {&KeyDev::p2_nprime, &KeyDev::q2_nprime}, rns[2] = {&KeyDev::rns_p, &KeyDev::rns_q},
               nR2[2] = {&KeyDev::nR2_p2, &KeyDev::nR2_q2}, nR2L[2] = {&KeyDev::nR2_p2L, &KeyDev::nR2_q2L},
               nR[2] = {&KeyDev::nR_p2, &KeyDev::nR_q2}, R1C[2] = {&KeyDev::R1C_p2X, &KeyDev::R1C_q2X},
               nR2C[2] = {&KeyDev::nR2C_p2X, &KeyDev::nR2C_q2X}, m1_words[2] = {&KeyDev::pm1_words, &KeyDev::qm1_words},
               inv_lim[2] = {&KeyDev::pinv_lim, &KeyDev::qinv_lim}, hR[2] = {&KeyDev::hpR, &KeyDev::hqR},
               topc[2] = {&KeyDev::topc_p, &KeyDev::topc_q}, mu[2] = {&KeyDev::mu_p, &KeyDev::mu_q},
               ms[2] = {&KeyDev::ms_p, &KeyDev::ms_q},
               e_words[2] = {&KeyDev::ep_words, &KeyDev::eq_words},
               x_kn2[2] = {&KeyDev::x_kn2_p, &KeyDev::x_kn2_q}, x_rmn[2] = {&KeyDev::x_rmn_p, &KeyDev::x_rmn_q},
               x_topc[2] = {&KeyDev::x_topc_p, &KeyDev::x_topc_q}, x_fold[2] = {&KeyDev::x_fold_p, &KeyDev::x_fold_q},
               x_hpR[2] = {&KeyDev::x_hpR_p, &KeyDev::x_hpR_q};
constexpr PairF x_dwt[2] = {&KeyDev::x_dwt_p, &KeyDev::x_dwt_q}, x_dw[2] = {&KeyDev::x_dw_p, &KeyDev::x_dw_q};
constexpr IntF m1_bits[2] = {&KeyDev::pm1_bits, &KeyDev::qm1_bits}, e_bits[2] = {&KeyDev::ep_bits, &KeyDev::eq_bits};
}  // namespace pq

// One prime X of a private key: the other prime Y, X^2, n mod X^2, and (from
// decrypt_constants on) hx = L_x((1 + n)^(x-1) mod x^2)^-1 mod x
struct Prime {
  BigU X, Y, X2, n, h;
};

// ------------------------------------------------------ Montgomery digits
// A value mod M^2 as two digits to the base M (pdigit_dev.hpp), M in the limbs
// of `s`, R = 2^(W S) > M.
struct DigitMod {
  const BigU& M;
  ModSpec s;
  BigU R, RM, Rinv;  // R, R mod M, R^-1 mod M
  DigitMod(const BigU& M_, const ModSpec& s_) : M(M_), s(s_), R(s_.R()), RM(mod(R, M_)), Rinv(modinv(RM, M_)) {}
};

// The digits (e, f) of w, given Xw = w R^2 mod M^2: R e + M f = Xw (mod M^2),
// e, f < M, as S interleaved pairs of limbs
inline std::vector<uint32_t> digit_pairs(const DigitMod& d, const BigU& Xw) {
  const BigU e = mulmod(mod(Xw, d.M), d.Rinv, d.M);
  BigU Q;
  divmod(add(Xw, mul(d.R, sub(d.M, e))), d.M, &Q, nullptr);  // (Xw - R e) / M + R
  const BigU f = submod(mod(Q, d.M), d.RM, d.M);
  const std::vector<uint32_t> el = e.to_limbs(d.s.W, d.s.S), fl = f.to_limbs(d.s.W, d.s.S);
  std::vector<uint32_t> v(2 * (size_t)d.s.S);
  for (int i = 0; i < d.s.S; ++i) {
    v[2 * i] = el[i];
    v[2 * i + 1] = fl[i];
  }
  return v;
}

// MASK + E_i, E = (1 - R) mod M, given RM = R mod M (the digit products' top correction)
inline std::vector<uint32_t> mask_plus_e(const BigU& M, const BigU& RM, const ModSpec& s) {
  std::vector<uint32_t> v = submod(BigU(1), RM, M).to_limbs(s.W, s.S);
  for (auto& x : v) x += (1u << s.W) - 1u;
  return v;
}

// What every digit modulus starts with: M itself as a modulus, ceil(R/M) M^2
// (the input conversion's offset, 2 S limbs) and R - M
inline void digit_modulus(KeyImage& im, const DigitMod& d, const BigU& M2, ModF m, RowF kn2, RowF rmn) {
  im.put_mod(d.M, d.s, m);
  BigU c;
  divmod(sub(add(d.R, d.M), BigU(1)), d.M, &c, nullptr);  // ceil(R / M)
  im.put_limbs(mul(c, M2), ModSpec{2 * d.s.S, d.s.W}, kn2);
  im.put_limbs(sub(d.R, d.M), d.s, rmn);
}

// ------------------------------------------------------------ the families
// n, n^2 and the encoding bounds as words; n^2 in its Montgomery shapes
inline void n2_constants(KeyImage& im, const KeySpec& s, const BigU& n, const BigU& n2, const BigU* h_pub) {
  im.put_words(n, s.nw(), &KeyDev::n_words);
  im.put_words(n2, s.n2w(), &KeyDev::n2_words);
  BigU maxpos;
  divmod(n, BigU(3), &maxpos, nullptr);
  im.put_words(maxpos, s.nw(), &KeyDev::maxpos);
  im.put_words(sub(n, maxpos), s.nw(), &KeyDev::minneg);
  im.put_limbs(n, s.mp2, &KeyDev::n_lim);
  im.put_mod(n2, s.mn2, &KeyDev::n2, kRpowRows);
  im.put_mod(n2, s.mn2X, &KeyDev::n2X, kRpowRows);
  if (s.K == 2048) {  // k_add_barrett: mu = floor(beta^(2S) / n^2), beta = 2^W, S + 1 limbs
    BigU mu;
    divmod(pow2((size_t)s.bar.W * 2 * s.bar.S), n2, &mu, nullptr);
    im.put_limbs(mu, ModSpec{s.bar.S + 1, s.bar.W}, &KeyDev::n2_mu);
  }
  if (s.K == 2048) {  // k_mexp_horner_wave: n^2, -n^-2 mod R_w, C = R_w^2 R_X^-1, R_w^2 mod n^2
    const ModSpec& sw = s.wave;
    const BigU Rw = sw.R();
    im.put_limbs(n2, sw, &KeyDev::n2w_N);
    im.put_limbs(sub(Rw, modinv(n2, Rw)), sw, &KeyDev::n2w_np);
    const BigU Rwn = mod(Rw, n2), Rw2 = mulmod(Rwn, Rwn, n2);
    im.put_limbs(mulmod(Rw2, modinv(mod(s.mn2X.R(), n2), n2), n2), sw, &KeyDev::n2w_C);
    im.put_limbs(Rw2, sw, &KeyDev::n2w_R2);
  }
  // k_enc_obf: x0 = X mod n and t = m x0 mod n are Montgomery products mod n
  // in the 4-lane shape (R >= 16 n as for p^2, both below 2^K); n^2 in 2 S of
  // its limbs for the last compare-and-subtract
  im.put_mod(n, s.mp2L, &KeyDev::nL);
  im.put_limbs(n2, ModSpec{2 * s.mp2L.S, s.mp2L.W}, &KeyDev::n2_limL);
  const BigU Rn2 = mod(s.mn2.R(), n2);
  im.put_limbs(mulmod(n, mulmod(Rn2, Rn2, n2), n2), s.mn2, &KeyDev::nR2_n2);
  if (h_pub) im.put_limbs(mulmod(mod(*h_pub, n2), Rn2, n2), s.mn2, &im.hM_n2);  // public DJN table base
}

// Montgomery digits mod n^2 (2048-bit keys; PMDX over the limbs of n,
// pdigit_dev.hpp): the digit modulus n, the digits of 1, of R^2 and of
// R^2 R_MN2^-1, MASK + E_i
inline void ndigit_constants(KeyImage& im, const KeySpec& s, const BigU& n, const BigU& n2) {
  const DigitMod d(n, s.nd);
  digit_modulus(im, d, n2, &KeyDev::nd, &KeyDev::nd_kn2, &KeyDev::nd_rmn);
  const BigU Rn2 = mod(d.R, n2), R2 = mulmod(Rn2, Rn2, n2), R4 = mulmod(R2, R2, n2);
  im.put(digit_pairs(d, R2), &KeyDev::nd_d1);  // w = 1
  im.put(digit_pairs(d, R4), &KeyDev::nd_dw);  // w = R^2
  // w = R^2 R_MN2^-1 (R_MN2: the public DJN tables' Montgomery factor):
  // converts their rows to canonical digits (k_tab_to_pmdx, n)
  im.put(digit_pairs(d, mulmod(R4, modinv(mod(s.mn2.R(), n2), n2), n2)), &KeyDev::nd_dwt);
  im.put(mask_plus_e(n, d.RM, d.s), &KeyDev::nd_topc);
}

// mod p^2 / q^2: the moduli in their three shapes, the one-wave and RNS
// decrypts' constants (2048), n R^k, the CRT constants (context.py:46) and,
// for DJN keys, the table bases and the 16-lane shape's start values
inline void prime2_constants(KeyImage& im, const KeySpec& s, const Prime (&pr)[2], const BigU* h, int nwin) {
  const ModSpec &s2 = s.mp2, &sL = s.mp2L, &sx = s.mp2X;
  const BigU &p2 = pr[0].X2, &q2 = pr[1].X2;
  im.put_mod(p2, s2, &KeyDev::p2);
  for (int i = 0; i < 2; ++i) im.put_mod(pr[i].X2, sL, pq::m2L[i]);
  for (int i = 0; i < 2; ++i) im.put_mod(pr[i].X2, sx, pq::m2X[i]);
  im.put_mod(q2, s2, &KeyDev::q2);
  const BigU R = s2.R();
  if (s.K == 2048) {
    // -P^-2 mod R for k_dec_wave's parallel REDC
    for (int i = 0; i < 2; ++i) im.put_limbs(sub(R, modinv(pr[i].X2, R)), s2, pq::nprime[i]);
    // the RNS decrypt's bases (shared by every key) and per-prime constants
    im.put(rnsh::bases().shared, &KeyDev::rns);
    for (int i = 0; i < 2; ++i) im.put(rnsh::prime_block(pr[i].X), pq::rns[i]);
  }
  const BigU Rm[2] = {mod(R, p2), mod(R, q2)};
  for (int i = 0; i < 2; ++i)  // n R^2 mod P^2
    im.put_limbs(mulmod(pr[i].n, mulmod(Rm[i], Rm[i], pr[i].X2), pr[i].X2), s2, pq::nR2[i]);
  const BigU RL = sL.R();
  for (int i = 0; i < 2; ++i) {  // n R_L^2 mod P^2 for the 4-lane shape (k_nodjn_crt<MP2L, 1>)
    const BigU RLm = mod(RL, pr[i].X2);
    im.put_limbs(mulmod(pr[i].n, mulmod(RLm, RLm, pr[i].X2), pr[i].X2), sL, pq::nR2L[i]);
  }
  for (int i = 0; i < 2; ++i) im.put_limbs(mulmod(pr[i].n, Rm[i], pr[i].X2), s2, pq::nR[i]);  // n R mod P^2
  im.put_limbs(mulmod(modinv(q2, p2), Rm[0], p2), s2, &KeyDev::q2invR_p2);
  im.put_limbs(q2, s2, &KeyDev::q2_lim);
  im.put_limbs(shl(p2, 2), s2, &KeyDev::p2x4_lim);
  if (!s.djn) return;
  for (int i = 0; i < 2; ++i)  // h_pow_n mod p^2 (context.py:63)
    im.put_limbs(mulmod(mod(*h, pr[i].X2), Rm[i], pr[i].X2), s2, &im.hM_p2[i]);
  // 16-lane small-batch shape on the same tables (k_djn_pow_x): C = (R'/R)^nwin
  const BigU Rx = sx.R(), Cexp = pow2((size_t)(sx.S - s2.S) * s2.W * nwin);
  for (int i = 0; i < 2; ++i) {
    const BigU& X2 = pr[i].X2;
    const BigU RxP = mod(Rx, X2), CR = mulmod(mod(Cexp, X2), RxP, X2);
    im.put_limbs(CR, sx, pq::R1C[i]);
    im.put_limbs(mulmod(pr[i].n, mulmod(CR, RxP, X2), X2), sx, pq::nR2C[i]);
  }
}

// mod p / q (decrypt): the moduli, the exponents P - 1, P^-1 mod R, hp R,
// the CRT's q^-1 R (context.py:43), and the one-lane digit kernels' MASK + E_i
// (2048; k_djn_pmd, k_dec_pmd) and k_djn_pmd's plaintext factors mu and ms
// (2048-bit DJN keys). Leaves hp, hq in pr[].h.
inline void decrypt_constants(KeyImage& im, const KeySpec& s, const BigU& n, Prime (&pr)[2]) {
  const ModSpec& s1 = s.mp;
  const BigU T = s1.R();
  for (int i = 0; i < 2; ++i) im.put_mod(pr[i].X, s1, pq::m1[i]);
  for (int i = 0; i < 2; ++i) {
    const BigU m1 = sub(pr[i].X, BigU(1));
    im.kd.*pq::m1_bits[i] = (int)m1.bits();
    im.put_words(m1, s.nw() / 2 + 1, pq::m1_words[i]);
  }
  for (int i = 0; i < 2; ++i) im.put_limbs(modinv(pr[i].X, T), s1, pq::inv_lim[i]);
  // hp = L_p((n+1)^(p-1) mod p^2)^-1 mod p (context.py:47,193-194). By the
  // binomial theorem (n+1)^(p-1) = 1 + (p-1) n (mod n^2, hence mod p^2).
  BigU Tm[2];
  for (int i = 0; i < 2; ++i) {
    const BigU& X = pr[i].X;
    const BigU x = mod(add(BigU(1), mul(sub(X, BigU(1)), n)), pr[i].X2);
    BigU L;
    divmod(sub(x, BigU(1)), X, &L, nullptr);
    pr[i].h = modinv(L, X);
    Tm[i] = mod(T, X);
  }
  for (int i = 0; i < 2; ++i) im.put_limbs(mulmod(pr[i].h, Tm[i], pr[i].X), s1, pq::hR[i]);
  im.put_limbs(mulmod(modinv(pr[1].X, pr[0].X), Tm[0], pr[0].X), s1, &KeyDev::qinvpR);
  im.put_limbs(pr[1].X, s1, &KeyDev::q_lim);
  if (s.K == 2048)  // the digits' R is the mod-p shape's R, so R mod P is kd.p.R1
    for (int i = 0; i < 2; ++i) im.put(mask_plus_e(pr[i].X, mod(s.pmd.R(), pr[i].X), s.pmd), pq::topc[i]);
  // k_djn_pmd's plaintext factor Q R^4 mod P: REDC(m) = m R^-1, and its
  // Montgomery product with Q R^4 is Q m R^2 mod P, the log digit of 1 + n m
  if (s.K == 2048 && s.djn)
    for (int i = 0; i < 2; ++i) {
      const BigU &X = pr[i].X, RX = mod(s.pmd.R(), X), R2 = mulmod(RX, RX, X);
      im.put_limbs(mulmod(mod(pr[i].Y, X), mulmod(R2, R2, X), X), s.pmd, pq::mu[i]);
    }
  // and its short-plaintext factor Q R^2 B mod P, B = 2^(28 * 4): s ms / B (four
  // Montgomery steps by P) is s Q R^2 mod P, the log digit of 1 + n s
  if (s.K == 2048 && s.djn)
    for (int i = 0; i < 2; ++i) {
      const BigU &X = pr[i].X, RX = mod(s.pmd.R(), X), R2 = mulmod(RX, RX, X);
      im.put_limbs(mulmod(mulmod(mod(pr[i].Y, X), R2, X), mod(pow2((size_t)s.pmd.W * 4), X), X), s.pmd, pq::ms[i]);
    }
}

// Montgomery digits mod P^2 (3072+-bit keys; k_djn_pmdx, k_dec_pmdx_*), one
// prime: the digit modulus P, MASK + E_i, the fold constant Q R^3 mod P, the
// digits of R^2 R_MP2^-1 (R_MP2: the MP2 shape's R, the tables' factor) and of
// R^2 (plain conversion), and hp R mod P (decrypt)
inline void pdigit_constants(KeyImage& im, const KeySpec& s, const Prime& pr, int i) {
  const BigU &X = pr.X, &X2 = pr.X2;
  const DigitMod d(X, s.pd);
  digit_modulus(im, d, X2, pq::dm[i], pq::x_kn2[i], pq::x_rmn[i]);
  im.put(mask_plus_e(X, d.RM, d.s), pq::x_topc[i]);
  im.put_limbs(mulmod(mod(pr.Y, X), mulmod(mulmod(d.RM, d.RM, X), d.RM, X), X), d.s, pq::x_fold[i]);
  const BigU Rx2 = mod(d.R, X2), R2 = mulmod(Rx2, Rx2, X2), R4 = mulmod(R2, R2, X2);
  im.put(digit_pairs(d, mulmod(R4, modinv(mod(s.mp2.R(), X2), X2), X2)), pq::x_dwt[i]);  // w = R^2 R_MP2^-1
  im.put(digit_pairs(d, R4), pq::x_dw[i]);                                               // w = R^2
  im.put_limbs(mulmod(pr.h, d.RM, X), d.s, pq::x_hpR[i]);
}

// 2p and p as mod-p limbs; the non-DJN private obfuscation exponents
// ep = n mod phi(p^2) (context.py:51-52)
inline void exponent_constants(KeyImage& im, const KeySpec& s, const BigU& n, const Prime (&pr)[2]) {
  im.put_limbs(shl(pr[0].X, 1), s.mp, &KeyDev::p2x_lim);
  im.put_limbs(pr[0].X, s.mp, &KeyDev::p_lim);
  for (int i = 0; i < 2; ++i) {
    const BigU e = mod(n, mul(pr[i].X, sub(pr[i].X, BigU(1))));
    im.kd.*pq::e_bits[i] = (int)e.bits();
    im.put_words(e, s.nw(), pq::e_words[i]);
  }
}

// The inverse table base h^-1 R mod P as a padded limb row: the one modular
// inversion per prime behind the tables' log digits (pdigit_dev.hpp)
inline std::vector<uint32_t> inverse_base_limbs(const ModSpec& s, const BigU& h, const BigU& P) {
  std::vector<uint32_t> v = mulmod(modinv(mod(h, P), P), mod(s.R(), P), P).to_limbs(s.W, s.S);
  v.resize((size_t)s.S4(), 0u);
  return v;
}

// p, q: null for a public key; h (= h_pow_n, context.py:63): null for a non-DJN key.
inline KeyImage derive_key_constants(const KeySpec& s, const BigU& n, const BigU* p, const BigU* q, const BigU* h) {
  KeyImage im;
  KeyDev& kd = im.kd;
  kd.K = s.K;
  kd.nw = s.nw();
  kd.n2w = s.n2w();
  kd.priv = s.priv;
  kd.djn = s.djn;
  kd.n_bits = (int)n.bits();
  // randomness bound (paillier.py:195 djn_exp_bound = 2^(bitlen(n)//2); :215 r < n)
  im.rand_bits = s.djn ? (int)(n.bits() / 2) : (int)n.bits();
  im.rand_words = (im.rand_bits + 31) / 32;
  if (s.djn) {  // the fixed-base tables' windows; public tables stay uniform
    kd.win = s.win;
    win_layout(im.rand_bits, s.win, s.priv && s.split, &kd.nwin, &kd.nhi);
  }
  const BigU n2 = mul(n, n);
  n2_constants(im, s, n, n2, s.djn && !s.priv ? h : nullptr);
  if (s.K == 2048) {
    kd.ndig = 1;
    ndigit_constants(im, s, n, n2);
  }
  if (!s.priv) return im;
  Prime pr[2] = {{*p, *q, mul(*p, *p), {}, {}}, {*q, *p, mul(*q, *q), {}, {}}};
  for (Prime& x : pr) x.n = mod(n, x.X2);
  prime2_constants(im, s, pr, h, kd.nwin);
  decrypt_constants(im, s, n, pr);
  if (s.K != 2048) {
    kd.pmdx_dec = 1;
    for (int i = 0; i < 2; ++i) pdigit_constants(im, s, pr[i], i);
  }
  exponent_constants(im, s, n, pr);
  if (s.K == 2048 && s.djn)
    for (int i = 0; i < 2; ++i) im.hinvM_p[i] = inverse_base_limbs(s.pmd, *h, pr[i].X);
  return im;
}

}  // namespace xhe
