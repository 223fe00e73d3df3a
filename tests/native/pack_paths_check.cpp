// Prints what xfl_amd/csrc/paths.hpp's pack() chooses for xhe_pack, one answer
// per line of stdin (tests/test_pack_host.py holds the expected answers), in
// the input format of paths_check.cpp. Host-only: plain g++ -std=c++17.
//
//   pack K=.. lanes=.. ndig=.. ngroups=.. [XHE_NAME=value ...]  ->  SHAPE/ARITH
//   const                                                       ->  kPackRowMax=.. kN2RowMax=..
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../../xfl_amd/csrc/paths.hpp"

using namespace xhe::paths;

int main() {
  std::string text;
  while (std::getline(std::cin, text)) {
    std::istringstream in(text);
    std::string op, tok;
    if (!(in >> op) || op[0] == '#') continue;
    std::map<std::string, std::string> args, env;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) {
        fprintf(stderr, "pack_paths_check: token without '=': %s\n", tok.c_str());
        return 2;
      }
      (tok.rfind("XHE_", 0) == 0 ? env : args)[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    const Pins pins = parse_pins([&](const char* n) -> const char* {
      auto it = env.find(n);
      return it == env.end() ? nullptr : it->second.c_str();
    });
    auto N = [&](const char* key) -> int64_t {
      auto it = args.find(key);
      if (it == args.end()) {
        fprintf(stderr, "pack_paths_check: missing argument %s\n", key);
        exit(2);
      }
      return atoll(it->second.c_str());
    };
    if (op == "const") {
      printf("kPackRowMax=%lld kN2RowMax=%lld\n", (long long)kPackRowMax, (long long)kN2RowMax);
    } else if (op == "pack") {
      const Pack p = pack((int)N("K"), (int)N("lanes"), N("ndig") != 0, N("ngroups"), pins);
      printf("%s/%s\n", p.shape == N2Shape::ROW16 ? "ROW16" : "LANES4", p.arith == Pow::NDIG ? "NDIG" : "MONT");
    } else {
      fprintf(stderr, "pack_paths_check: unknown op %s\n", op.c_str());
      return 2;
    }
  }
  return 0;
}
