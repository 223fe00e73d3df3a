// Host-only check of k_djn_pmd's short-plaintext factors (tests/test_ms_const.py):
// derives a key's constants as keyconst_check.cpp does and prints the two
// fields KeyDev::ms_p / ms_q (Q R^2 B mod P and P R^2 B mod Q, R = 2^(28 * 37),
// B = 2^(28 * 4), as 37 limbs of 28 bits in a row of 40 words) with their place
// in the blob.
//
//   stdin, one line of hex words:  K flags win n p q h     ("-": absent)
//     flags: 1 private, 2 DJN;  win: window bits, | 0x100 for the split layout
//   stdout:
//     words <count>
//     F <name> <word offset | -1> <W> <len> <len hex limbs>
//       ms_p, ms_q; mu_q (the constant before them) and eq_words (the
//       blob's last constant) for the placement
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../xfl_amd/csrc/keyconst.hpp"

using namespace xhe;

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

static void row(const char* name, const uint32_t* p, const uint32_t* base, size_t nwords, int W, int len) {
  if (!p) {
    printf("F %s -1 0 0\n", name);
    return;
  }
  const long long off = p - base;
  printf("F %s %lld %d %d", name, off, W, len);
  if (off < 0 || (size_t)off + (size_t)len > nwords) {
    printf(" OUT-OF-BLOB\n");
    return;
  }
  for (int i = 0; i < len; ++i) printf(" %x", p[i]);
  printf("\n");
}

int main() {
  std::string line;
  if (!std::getline(std::cin, line)) return 2;
  std::istringstream in(line);
  std::string sK, sflags, swin, sn, sp, sq, sh;
  if (!(in >> sK >> sflags >> swin >> sn >> sp >> sq >> sh)) return 2;
  const int K = (int)strtol(sK.c_str(), nullptr, 16);
  const int flags = (int)strtol(sflags.c_str(), nullptr, 16), win = (int)strtol(swin.c_str(), nullptr, 16);
  KeySpec s{};
  s.K = K;
  if (K == 2048) {  // the 2048-bit shapes, as keyconst_check.cpp states them
    s.mp2 = {74, 28}, s.mp2L = {76, 28}, s.mp2X = {80, 28}, s.mp = {37, 28}, s.mn2 = {152, 27}, s.mn2X = {160, 27};
    s.nd = {80, 27}, s.pmd = {37, 28}, s.wave = {154, 27}, s.bar = {152, 27};
  } else if (K == 3072) {
    s.mp2 = {110, 28}, s.mp2L = {112, 28}, s.mp2X = {112, 28}, s.mp = {56, 28}, s.mn2 = {228, 27}, s.mn2X = {240, 27};
    s.pd = {60, 27};
  } else {
    fprintf(stderr, "ms_const_check: unsupported key size %d\n", K);
    return 2;
  }
  s.priv = (flags & 1) != 0;
  s.djn = (flags & 2) != 0;
  s.win = win & 0xff;
  s.split = (win & 0x100) != 0;
  const BigU n = from_hex(sn), p = from_hex(sp), q = from_hex(sq), h = from_hex(sh);
  if (s.priv != (sp != "-") || s.priv != (sq != "-") || s.djn != (sh != "-")) return 2;
  const KeyImage im = derive_key_constants(s, n, s.priv ? &p : nullptr, s.priv ? &q : nullptr, s.djn ? &h : nullptr);
  const KeyDev kd = im.bind(im.words.data());
  const uint32_t* base = im.words.data();
  printf("words %zu\n", im.words.size());
  row("ms_p", kd.ms_p, base, im.words.size(), 28, 37);
  row("ms_q", kd.ms_q, base, im.words.size(), 28, 37);
  row("mu_q", kd.mu_q, base, im.words.size(), 28, 37);
  row("eq_words", kd.eq_words, base, im.words.size(), 32, kd.nw);
  return 0;
}
