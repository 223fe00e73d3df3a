// Prints the kernel path xfl_amd/csrc/paths.hpp chooses, one answer per line
// of stdin (tests/test_paths.py holds the expected answers). Host-only: plain
// g++ -std=c++17, no ROCm include.
//
//   <op> name=value ... [XHE_NAME=value ...]
//
// The name=value tokens are the arguments of the op's planner function; every
// token that starts with XHE_ is a kernel switch, looked up by parse_pins in
// place of the environment ("XHE_NDIG=" sets the empty string; a switch not
// named is unset). Ops: const, pins, enc_djn, enc_pub_djn, enc_nodjn, n2, add,
// powmod, invert, segprod, horner, decrypt.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../../xfl_amd/csrc/paths.hpp"

using namespace xhe::paths;

namespace {

const char* name(EncDjn p) {
  switch (p) {
    case EncDjn::PMD: return "PMD";
    case EncDjn::PMDX: return "PMDX";
    case EncDjn::POW_X: return "POW_X";
    case EncDjn::POW_LDS: return "POW_LDS";
    case EncDjn::POW: return "POW";
  }
  return "?";
}
const char* name(EncPubDjn p) { return p == EncPubDjn::PUB_ND ? "PUB_ND" : p == EncPubDjn::PUB ? "PUB" : "?"; }
const char* name(EncNoDjn p) {
  switch (p) {
    case EncNoDjn::PMD: return "PMD";
    case EncNoDjn::PUB_WAVE: return "PUB_WAVE";
    case EncNoDjn::CRT: return "CRT";
    case EncNoDjn::NDIG: return "NDIG";
    case EncNoDjn::PUB: return "PUB";
  }
  return "?";
}
const char* name(N2Shape p) { return p == N2Shape::ROW16 ? "ROW16" : p == N2Shape::LANES4 ? "LANES4" : "?"; }
const char* name(Add p) { return p == Add::WAVE ? "WAVE" : p == Add::BARRETT ? "BARRETT" : p == Add::MONT ? "MONT" : "?"; }
const char* name(Pow p) { return p == Pow::NDIG ? "NDIG" : p == Pow::MONT ? "MONT" : "?"; }
const char* name(Invert p) { return p == Invert::WTREE ? "WTREE" : p == Invert::TREE ? "TREE" : "?"; }
const char* name(SegFirst p) { return p == SegFirst::WORDS ? "WORDS" : p == SegFirst::ALIGN ? "ALIGN" : "?"; }
const char* name(Horner p) { return p == Horner::WAVE ? "WAVE" : p == Horner::LANES ? "LANES" : "?"; }
const char* name(Dec p) {
  switch (p) {
    case Dec::PMDX: return "PMDX";
    case Dec::RNS: return "RNS";
    case Dec::WAVE: return "WAVE";
    case Dec::ROW16: return "ROW16";
    case Dec::QUAD4: return "QUAD4";
    case Dec::PMD1: return "PMD1";
    case Dec::POW1: return "POW1";
  }
  return "?";
}

struct Line {
  std::map<std::string, std::string> args, env;
  int64_t num(const char* key) const {
    auto it = args.find(key);
    if (it == args.end()) {
      fprintf(stderr, "paths_check: missing argument %s\n", key);
      exit(2);
    }
    return atoll(it->second.c_str());
  }
};

}  // namespace

int main() {
  std::string text;
  while (std::getline(std::cin, text)) {
    std::istringstream in(text);
    std::string op, tok;
    if (!(in >> op) || op[0] == '#') continue;
    Line l;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) {
        fprintf(stderr, "paths_check: token without '=': %s\n", tok.c_str());
        return 2;
      }
      (tok.rfind("XHE_", 0) == 0 ? l.env : l.args)[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    const Pins pins = parse_pins([&](const char* n) -> const char* {
      auto it = l.env.find(n);
      return it == l.env.end() ? nullptr : it->second.c_str();
    });
    auto N = [&](const char* key) { return l.num(key); };
    if (op == "const") {
      printf("kEncRowMax=%lld kPmdSplit16Max=%lld kPmdSplit4Max=%lld kPubWaveMax=%lld kN2RowMax=%lld kWaveAddMax=%lld "
             "kWtreeMax=%lld kMexpWaveMax=%lld kDecWaveMax=%lld kDecRowMax=%lld kDecQuadMax=%lld\n",
             (long long)kEncRowMax, (long long)kPmdSplit16Max, (long long)kPmdSplit4Max, (long long)kPubWaveMax,
             (long long)kN2RowMax, (long long)kWaveAddMax, (long long)kWtreeMax, (long long)kMexpWaveMax,
             (long long)kDecWaveMax, (long long)kDecRowMax, (long long)kDecQuadMax);
    } else if (op == "pins") {
      printf("enc_tpi=%d pmd_split=%d pub_tpi=%d n2_tpi=%d dec_tpi=%d ndig_pub=%d ndig=%d nodjn_pmd=%d add_wave=%d "
             "add_bar=%d sum_words=%d mexp_wave=%d dec_pmdx=%d dec_rns=%d\n",
             pins.enc_tpi, pins.pmd_split, pins.pub_tpi, pins.n2_tpi, pins.dec_tpi, pins.ndig_pub, pins.ndig,
             pins.nodjn_pmd, pins.add_wave, pins.add_bar, pins.sum_words, pins.mexp_wave, pins.dec_pmdx, pins.dec_rns);
    } else if (op == "enc_djn") {
      const EncDjn p = enc_djn((int)N("K"), (int)N("lanes"), N("pmd") != 0, N("pmdx") != 0, N("n"), pins);
      if (p == EncDjn::PMD) printf("PMD/%d\n", pmd_split(N("n"), pins));
      else puts(name(p));
    } else if (op == "enc_pub_djn") {
      puts(name(enc_pub_djn((int)N("K"), N("pub_nd") != 0)));
    } else if (op == "enc_nodjn") {
      puts(name(enc_nodjn((int)N("K"), N("priv") != 0, N("ndig") != 0, N("count"), pins)));
    } else if (op == "n2") {
      puts(name(n2_shape(N("count"), pins)));
    } else if (op == "add") {
      puts(name(add((int)N("K"), (int)N("lanes"), N("count"), (int)N("dmax"), pins)));
    } else if (op == "powmod") {
      puts(name(powmod((int)N("K"), (int)N("lanes"), N("ndig") != 0, pins)));
    } else if (op == "invert") {
      puts(name(invert((int)N("K"), (int)N("lanes"), N("count"))));
    } else if (op == "segprod") {
      puts(name(segprod_first(N("count"), (int)N("dmax"), N("has_d") != 0, pins)));
    } else if (op == "horner") {
      puts(name(mexp_horner((int)N("K"), (int)N("lanes"), N("ncols"), pins)));
    } else if (op == "decrypt") {
      puts(name(decrypt((int)N("K"), (int)N("lanes"), N("pmdx_dec") != 0, N("rns") != 0, N("count"), pins)));
    } else {
      fprintf(stderr, "paths_check: unknown op %s\n", op.c_str());
      return 2;
    }
  }
  return 0;
}
