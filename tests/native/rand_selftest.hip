// The obfuscation draw kernels (xfl_amd/csrc/xhe_kernels.hpp: k_rand_djn,
// k_rand_below) launched directly with tiny `bits` and `bound`, where the
// paths the C ABI cannot reach with real keys run all the time: the zero-draw
// redraw of k_rand_djn (group ballot, then rand_elem from attempt 1) and the
// ST_VALUE exit after 64 rejections. Run on the GPU box by
// tests/test_gpu_native_selftests.py.
//
// This program checks nothing. Per case it fills the output (count rows and
// one guard row) and the statuses with 0xA5A5A5A5, launches the kernel once
// and prints one JSON line with the case's parameters, the key and nonce, and
// the output words, statuses and guard row as hex; the pytest compares them
// with tests/chacha_ref.py. Exit status 1 only on a HIP error.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../xfl_amd/csrc/xhe_kernels.hpp"

using namespace xhe;

#define CK(x)                                                                              \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));   \
      return 1;                                                                            \
    }                                                                                      \
  } while (0)

constexpr uint32_t FILL = 0xA5A5A5A5u;
constexpr int COUNT = 300;
constexpr int64_t BASE = 0;
constexpr uint64_t NONCE = 0x0123456789ABCDEFull;

struct Case {
  const char* kernel;  // "djn" or "below"
  int words, bits, tpe;
  uint64_t bound;  // k_rand_below only (words <= 2)
};

static const Case CASES[] = {
    {"djn", 4, 1, 1, 0},
    {"djn", 4, 3, 1, 0},
    {"djn", 32, 2, 2, 0},
    {"djn", 32, 33, 2, 0},
    {"djn", 48, 2, 4, 0},
    {"djn", 128, 1, 8, 0},
    {"djn", 3, 70, 1, 0},
    {"djn", 4, 64, 1, 0},  // bits - 32 k = 32: a whole top word, the edge of the mask
    {"djn", 40, 1270, 4, 0},  // lanes 1 and 2 hold live words (all other groups mask them to zero); a half last block
    {"below", 2, 40, 0, (1ull << 39) + 12345},
    {"below", 2, 33, 0, (1ull << 32) + (1ull << 31)},
    {"below", 1, 1, 0, 2},
    {"below", 2, 40, 0, 1},
    {"below", 2, 64, 0, (1ull << 63) + (1ull << 62) + 5},  // a whole top word
};

static void hex_words(std::string& s, const uint32_t* w, size_t n) {
  char b[9];
  for (size_t i = 0; i < n; ++i) {
    snprintf(b, sizeof b, "%08x", w[i]);
    s += b;
  }
}

static int run(const Case& c, const ChaChaKey& ck, const std::string& key_hex) {
  const size_t nout = (size_t)(COUNT + 1) * c.words;  // the last row is the guard
  std::vector<uint32_t> out(nout, FILL), st(COUNT + 1, FILL);
  uint32_t *d_out = nullptr, *d_st = nullptr, *d_bound = nullptr;
  CK(hipMalloc(&d_out, nout * 4));
  CK(hipMalloc(&d_st, st.size() * 4));
  CK(hipMemcpy(d_out, out.data(), nout * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_st, st.data(), st.size() * 4, hipMemcpyHostToDevice));
  const bool djn = c.kernel[0] == 'd';
  if (djn) {
    const unsigned blocks = (unsigned)(((int64_t)COUNT * c.tpe + 255) / 256);
    hipLaunchKernelGGL(k_rand_djn, dim3(blocks), dim3(256), 0, 0, ck, BASE, (int64_t)COUNT, c.words, c.bits, c.tpe,
                       d_out, reinterpret_cast<int32_t*>(d_st));
  } else {
    uint32_t bw[2] = {(uint32_t)c.bound, (uint32_t)(c.bound >> 32)};
    CK(hipMalloc(&d_bound, sizeof bw));
    CK(hipMemcpy(d_bound, bw, sizeof bw, hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)((COUNT + 255) / 256);
    hipLaunchKernelGGL(k_rand_below, dim3(blocks), dim3(256), 0, 0, ck, BASE, (int64_t)COUNT, c.words, c.bits,
                       d_bound, d_out, reinterpret_cast<int32_t*>(d_st));
  }
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(out.data(), d_out, nout * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(st.data(), d_st, st.size() * 4, hipMemcpyDeviceToHost));
  CK(hipFree(d_out));
  CK(hipFree(d_st));
  if (d_bound) CK(hipFree(d_bound));
  std::string s;
  char head[512];
  snprintf(head, sizeof head,
           "{\"kernel\": \"%s\", \"words\": %d, \"bits\": %d, \"tpe\": %d, \"bound\": \"%llx\", \"count\": %d, "
           "\"base\": %lld, \"key\": \"%s\", \"nonce\": \"%llx\", \"out\": \"",
           c.kernel, c.words, c.bits, c.tpe, (unsigned long long)c.bound, COUNT, (long long)BASE, key_hex.c_str(),
           (unsigned long long)NONCE);
  s += head;
  hex_words(s, out.data(), (size_t)COUNT * c.words);
  s += "\", \"status\": \"";
  hex_words(s, st.data(), COUNT);
  s += "\", \"guard\": \"";
  hex_words(s, out.data() + (size_t)COUNT * c.words, c.words);
  s += "\", \"status_guard\": \"";
  hex_words(s, st.data() + COUNT, 1);
  s += "\"}\n";
  fputs(s.c_str(), stdout);
  fflush(stdout);
  return 0;
}

int main() {
  uint8_t seed[32];
  for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(i + 1);
  ChaChaKey ck;
  memcpy(ck.k, seed, 32);
  ck.nonce0 = (uint32_t)NONCE;
  ck.nonce1 = (uint32_t)(NONCE >> 32);
  std::string key_hex;
  char b[3];
  for (int i = 0; i < 32; ++i) {
    snprintf(b, sizeof b, "%02x", seed[i]);
    key_hex += b;
  }
  for (const Case& c : CASES)
    if (run(c, ck, key_hex)) return 1;
  return 0;
}
