// Host-only check of keyconst.hpp (tests/test_keyconst.py): derives a key's
// constants, binds the KeyDev to the host vector's own address and prints
// every field with the limbs it points at, read through the bound KeyDev.
//
//   stdin, one line of hex words:  K flags win n p q h     ("-": absent)
//     flags: 1 private, 2 DJN;  win: window bits, | 0x100 for the split layout
//   stdout:
//     words <count>
//     S <name> <decimal>                    scalar fields
//     F <name> <word offset | -1> <W> <len> <len hex limbs>   (W = 32: words)
//     B <count hex words>                   the whole blob (argv[1] == "--blob")
//
// The limb shapes below are a second, independent statement of DESIGN.md §3
// and of the Shape* comments in xhe.hip: the library fills its KeySpec from
// the kernels' template types, this program from literals.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../xfl_amd/csrc/keyconst.hpp"

using namespace xhe;

static KeySpec spec_for(int K) {
  KeySpec s{};
  s.K = K;
  switch (K) {
    case 2048:  // 28-bit limbs mod p^2 (1, 4, 16 lanes) and mod p; 27-bit mod n^2
      s.mp2 = {74, 28}, s.mp2L = {76, 28}, s.mp2X = {80, 28}, s.mp = {37, 28}, s.mn2 = {152, 27}, s.mn2X = {160, 27};
      s.nd = {80, 27};     // n in 80 limbs of 27 bits, R = 2^2160
      s.pmd = {37, 28};    // P in 37 limbs of 28 bits, R = 2^1036
      s.wave = {154, 27};  // n^2 in 154 limbs of 27 bits, R_w = 2^4158
      s.bar = {152, 27};   // mu = floor(2^(27*304) / n^2) in 153 limbs
      break;
    case 3072:
      s.mp2 = {110, 28}, s.mp2L = {112, 28}, s.mp2X = {112, 28}, s.mp = {56, 28}, s.mn2 = {228, 27}, s.mn2X = {240, 27};
      s.pd = {60, 27};  // P in 60 limbs of 27 bits
      break;
    case 4096:  // 27-bit limbs everywhere
      s.mp2 = {152, 27}, s.mp2L = {152, 27}, s.mp2X = {160, 27}, s.mp = {76, 27}, s.mn2 = {304, 27}, s.mn2X = {304, 27};
      s.pd = {80, 27};
      break;
    case 8192:  // n^2 in 26-bit limbs
      s.mp2 = {304, 27}, s.mp2L = {304, 27}, s.mp2X = {304, 27}, s.mp = {152, 27}, s.mn2 = {640, 26}, s.mn2X = {640, 26};
      s.pd = {160, 27};  // R = 2^4320
      break;
    default:
      fprintf(stderr, "keyconst_check: unsupported key size %d\n", K);
      exit(2);
  }
  return s;
}

static BigU from_hex(const std::string& h) {
  BigU r;
  for (size_t end = h.size(); end > 0;) {
    const size_t beg = end >= 8 ? end - 8 : 0;
    r.w.push_back((uint32_t)strtoul(h.substr(beg, end - beg).c_str(), nullptr, 16));
    end = beg;
  }
  r.trim();
  return r;
}

struct Emit {
  const uint32_t* base;
  size_t nwords;
  void scalar(const char* name, long long v) const { printf("S %s %lld\n", name, v); }
  void row(const std::string& name, const void* ptr, int W, int len) const {
    const uint32_t* p = static_cast<const uint32_t*>(ptr);
    if (!p) {
      printf("F %s -1 0 0\n", name.c_str());
      return;
    }
    const long long off = p - base;
    printf("F %s %lld %d %d", name.c_str(), off, W, len);
    if (off < 0 || (size_t)off + (size_t)len > nwords) {
      printf(" OUT-OF-BLOB\n");
      return;
    }
    for (int i = 0; i < len; ++i) printf(" %x", p[i]);
    printf("\n");
  }
  void limbs(const char* name, const void* p, const ModSpec& s) const { row(name, p, s.W, s.S); }
  void mod(const std::string& name, const ModDev& m, const ModSpec& s, int npow = 0) const {
    row(name + ".N", m.N, s.W, s.S);
    row(name + ".R1", m.R1, s.W, s.S);
    row(name + ".R2", m.R2, s.W, s.S);
    row(name + ".R3", m.R3, s.W, s.S);
    row(name + ".Rpow", m.Rpow, s.W, npow * s.S4());
    scalar((name + ".n0inv").c_str(), m.n0inv);
  }
};

// Every KeyDev field that points into the blob, by name (the table pointers
// tab_n2 / tab_p2 / tab_q2 and tab_rs, pmd, pmdx, pub_nd belong to the table
// phase on the device), then the scalars.
static void emit_key(const Emit& e, const KeyDev& kd, const KeySpec& s) {
  const ModSpec w32n{s.nw(), 32}, w32n2{s.n2w(), 32}, w32h{s.nw() / 2 + 1, 32};
  const ModSpec nd2{2 * s.nd.S, s.nd.W}, pd2{2 * s.pd.S, s.pd.W}, mu{s.bar.S ? s.bar.S + 1 : 0, s.bar.W};
  e.limbs("n_words", kd.n_words, w32n);
  e.limbs("n2_words", kd.n2_words, w32n2);
  e.limbs("maxpos", kd.maxpos, w32n);
  e.limbs("minneg", kd.minneg, w32n);
  e.limbs("n_lim", kd.n_lim, s.mp2);
  e.mod("n2", kd.n2, s.mn2, kRpowRows);
  e.limbs("nR2_n2", kd.nR2_n2, s.mn2);
  e.limbs("ep_words", kd.ep_words, w32n);
  e.limbs("eq_words", kd.eq_words, w32n);
  e.mod("p2", kd.p2, s.mp2);
  e.mod("q2", kd.q2, s.mp2);
  e.mod("p2L", kd.p2L, s.mp2L);
  e.mod("q2L", kd.q2L, s.mp2L);
  e.mod("p2X", kd.p2X, s.mp2X);
  e.mod("q2X", kd.q2X, s.mp2X);
  e.mod("n2X", kd.n2X, s.mn2X, kRpowRows);
  e.limbs("nR2_p2", kd.nR2_p2, s.mp2);
  e.limbs("nR_p2", kd.nR_p2, s.mp2);
  e.limbs("nR_q2", kd.nR_q2, s.mp2);
  e.limbs("nR2C_p2X", kd.nR2C_p2X, s.mp2X);
  e.limbs("nR2C_q2X", kd.nR2C_q2X, s.mp2X);
  e.limbs("R1C_p2X", kd.R1C_p2X, s.mp2X);
  e.limbs("R1C_q2X", kd.R1C_q2X, s.mp2X);
  e.limbs("nR2_q2", kd.nR2_q2, s.mp2);
  e.limbs("nR2_p2L", kd.nR2_p2L, s.mp2L);
  e.limbs("nR2_q2L", kd.nR2_q2L, s.mp2L);
  e.limbs("q2invR_p2", kd.q2invR_p2, s.mp2);
  e.limbs("q2_lim", kd.q2_lim, s.mp2);
  e.limbs("p2x4_lim", kd.p2x4_lim, s.mp2);
  e.mod("p", kd.p, s.mp);
  e.mod("q", kd.q, s.mp);
  e.limbs("pm1_words", kd.pm1_words, w32h);
  e.limbs("qm1_words", kd.qm1_words, w32h);
  e.limbs("pinv_lim", kd.pinv_lim, s.mp);
  e.limbs("qinv_lim", kd.qinv_lim, s.mp);
  e.limbs("hpR", kd.hpR, s.mp);
  e.limbs("hqR", kd.hqR, s.mp);
  e.limbs("qinvpR", kd.qinvpR, s.mp);
  e.limbs("q_lim", kd.q_lim, s.mp);
  e.limbs("p2x_lim", kd.p2x_lim, s.mp);
  e.limbs("p_lim", kd.p_lim, s.mp);
  e.limbs("topc_p", kd.topc_p, s.pmd);
  e.limbs("topc_q", kd.topc_q, s.pmd);
  e.mod("nd", kd.nd, s.nd);
  e.limbs("nd_kn2", kd.nd_kn2, nd2);
  e.limbs("nd_rmn", kd.nd_rmn, s.nd);
  e.limbs("nd_topc", kd.nd_topc, s.nd);
  e.limbs("nd_dw", kd.nd_dw, nd2);
  e.limbs("nd_d1", kd.nd_d1, nd2);
  e.limbs("nd_dwt", kd.nd_dwt, nd2);
  e.mod("dp", kd.dp, s.pd);
  e.mod("dq", kd.dq, s.pd);
  e.limbs("x_kn2_p", kd.x_kn2_p, pd2);
  e.limbs("x_kn2_q", kd.x_kn2_q, pd2);
  e.limbs("x_rmn_p", kd.x_rmn_p, s.pd);
  e.limbs("x_rmn_q", kd.x_rmn_q, s.pd);
  e.limbs("x_topc_p", kd.x_topc_p, s.pd);
  e.limbs("x_topc_q", kd.x_topc_q, s.pd);
  e.limbs("x_fold_p", kd.x_fold_p, s.pd);
  e.limbs("x_fold_q", kd.x_fold_q, s.pd);
  e.limbs("x_dwt_p", kd.x_dwt_p, pd2);
  e.limbs("x_dwt_q", kd.x_dwt_q, pd2);
  e.limbs("x_dw_p", kd.x_dw_p, pd2);
  e.limbs("x_dw_q", kd.x_dw_q, pd2);
  e.limbs("x_hpR_p", kd.x_hpR_p, s.pd);
  e.limbs("x_hpR_q", kd.x_hpR_q, s.pd);
  e.limbs("p2_nprime", kd.p2_nprime, s.mp2);
  e.limbs("q2_nprime", kd.q2_nprime, s.mp2);
  e.row("rns", kd.rns, 32, rns::S_WORDS);
  e.row("rns_p", kd.rns_p, 32, rns::P_WORDS);
  e.row("rns_q", kd.rns_q, 32, rns::P_WORDS);
  e.limbs("n2w_N", kd.n2w_N, s.wave);
  e.limbs("n2w_np", kd.n2w_np, s.wave);
  e.limbs("n2w_C", kd.n2w_C, s.wave);
  e.limbs("n2w_R2", kd.n2w_R2, s.wave);
  e.limbs("n2_mu", kd.n2_mu, mu);
  e.scalar("K", kd.K);
  e.scalar("nw", kd.nw);
  e.scalar("n2w", kd.n2w);
  e.scalar("priv", kd.priv);
  e.scalar("djn", kd.djn);
  e.scalar("n_bits", kd.n_bits);
  e.scalar("ep_bits", kd.ep_bits);
  e.scalar("eq_bits", kd.eq_bits);
  e.scalar("pm1_bits", kd.pm1_bits);
  e.scalar("qm1_bits", kd.qm1_bits);
  e.scalar("win", kd.win);
  e.scalar("nwin", kd.nwin);
  e.scalar("nhi", kd.nhi);
  e.scalar("ndig", kd.ndig);
  e.scalar("pmdx_dec", kd.pmdx_dec);
}

int main(int argc, char** argv) {
  const bool blob = argc > 1 && std::string(argv[1]) == "--blob";
  std::string line;
  if (!std::getline(std::cin, line)) return 2;
  std::istringstream in(line);
  std::string sK, sflags, swin, sn, sp, sq, sh;
  if (!(in >> sK >> sflags >> swin >> sn >> sp >> sq >> sh)) return 2;
  const int flags = (int)strtol(sflags.c_str(), nullptr, 16), win = (int)strtol(swin.c_str(), nullptr, 16);
  KeySpec s = spec_for((int)strtol(sK.c_str(), nullptr, 16));
  s.priv = (flags & 1) != 0;
  s.djn = (flags & 2) != 0;
  s.win = win & 0xff;
  s.split = (win & 0x100) != 0;
  const BigU n = from_hex(sn), p = from_hex(sp), q = from_hex(sq), h = from_hex(sh);
  if (s.priv != (sp != "-") || s.priv != (sq != "-") || s.djn != (sh != "-")) return 2;
  const KeyImage im = derive_key_constants(s, n, s.priv ? &p : nullptr, s.priv ? &q : nullptr, s.djn ? &h : nullptr);
  const KeyDev kd = im.bind(im.words.data());
  const Emit e{im.words.data(), im.words.size()};
  printf("words %zu\n", im.words.size());
  emit_key(e, kd, s);
  e.scalar("rand_bits", im.rand_bits);
  e.scalar("rand_words", im.rand_words);
  // the fixed-base tables' bases (host-side offsets, read at key creation only)
  e.limbs("hM_n2", s.djn && !s.priv ? e.base + im.hM_n2 : nullptr, s.mn2);
  e.limbs("hM_p2", s.djn && s.priv ? e.base + im.hM_p2[0] : nullptr, s.mp2);
  e.limbs("hM_q2", s.djn && s.priv ? e.base + im.hM_p2[1] : nullptr, s.mp2);
  if (blob) {
    printf("B");
    for (uint32_t w : im.words) printf(" %x", w);
    printf("\n");
  }
  return 0;
}
