// Prints what xfl_amd/csrc/scan_plan.hpp plans, for tests/test_scan_plan.py.
// Plain g++, no HIP. One answer line per input line:
//   chunk_len count=N     -> the chunk length of a call over N elements
//   plan LEN,LEN,...      -> the plan of segments of these lengths at that
//                            call's chunk length: per level "rows=R:" and its
//                            chunks "first/len/total/carry", levels joined
//                            by " | " ("empty" when there is no level)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../xfl_amd/csrc/scan_plan.hpp"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, arg;
    in >> op >> arg;
    if (op == "chunk_len" && arg.rfind("count=", 0) == 0) {
      std::printf("%lld\n", (long long)xhe::scan::chunk_len(atoll(arg.c_str() + 6)));
    } else if (op == "plan") {
      std::vector<int64_t> seg{0};
      std::istringstream lens(arg);
      std::string tok;
      while (std::getline(lens, tok, ',')) seg.push_back(seg.back() + atoll(tok.c_str()));
      const xhe::scan::Plan p =
          xhe::scan::make_plan(seg.data(), (int64_t)seg.size() - 1, xhe::scan::chunk_len(seg.back()));
      std::string out;
      for (size_t l = 0; l < p.levels.size(); ++l) {
        const xhe::scan::Level& L = p.levels[l];
        if (l) out += " | ";
        out += "rows=" + std::to_string(L.rows) + ":";
        for (int64_t j = L.chunk0; j < L.chunk0 + L.nchunks; ++j) {
          const int64_t* c = &p.chunks[(size_t)j * xhe::scan::kFields];
          out += " " + std::to_string(c[0]) + "/" + std::to_string(c[1]) + "/" + std::to_string(c[2]) + "/" +
                 std::to_string(c[3]);
        }
      }
      std::printf("%s\n", out.empty() ? "empty" : out.c_str());
    } else {
      std::fprintf(stderr, "scan_plan_check: bad line: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
