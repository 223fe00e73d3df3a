// Sanitizer harness for the receiving side's index scan and the per-quad
// unpack (built by tests/test_wire_scan.py with g++ -fsanitize=address,undefined
// -fno-sanitize-recover=all, together with wire_abi.cpp):
//
//   wire_scan_fuzz scan N2W SEED...  xhe_wire_scan (the index of a payload a
//                            remote party sent, Paillier.ciphertext_from,
//                            paillier.py:260-271) on each seed file, whole and
//                            range by range through 4 KiB windows; then on
//                            every truncation, on seeded byte flips (half of
//                            them in the bytes between two values) and with
//                            value length fields inflated. Every accepted scan
//                            must keep all its ranges inside the input and
//                            give xhe_wire_decode's rows, exponents and shape
//                            on the same bytes; a scan through windows must
//                            agree with the whole one. Seeds in a foreign
//                            layout must be refused.
//   wire_scan_fuzz unpack    wireu::unpack_quad - the code k_wire_unpack runs
//                            per 16 B of a row - against memcpy + zero fill:
//                            all 16 source residues, the edge lengths, values
//                            that end exactly at the buffer's end (allocated
//                            at its exact size: an over-read aborts), and
//                            hostile offsets / lengths, which must read as
//                            zero bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
#include <string>
#include <vector>

#include "../../include/xhe.h"
#include "../../xfl_amd/csrc/wire_unpack.hpp"

using Bytes = std::vector<uint8_t>;

#define REQUIRE(c)                                                      \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      std::abort();                                                     \
    }                                                                   \
  } while (0)

static const int64_t kCap = 4096;  // the seeds hold at most 2001 elements
static long g_accepted = 0, g_refused = 0;

struct Index {
  std::vector<uint32_t> off;
  std::vector<uint16_t> len;
  std::vector<int32_t> exps;
  int64_t count = 0;
  int64_t shape[8] = {0};
  int ndim = 0;
};

// the whole payload in one call -> its return code
static int scan_whole(const Bytes& b, int n2w, Index& ix) {
  ix.off.assign(kCap, 0);
  ix.len.assign(kCap, 0);
  ix.exps.assign(kCap, 0);
  int64_t found = 0, next = 0;
  const int rc = xhe_wire_scan(b.data(), (int64_t)b.size(), 0, 1, n2w, ix.off.data(), ix.len.data(), ix.exps.data(),
                               kCap, &found, &next, ix.shape, &ix.ndim);
  if (rc == XHE_OK) {
    REQUIRE(next == (int64_t)b.size());
    for (int64_t k = 0; k < found; ++k) {
      REQUIRE((int64_t)ix.off[k] + ix.len[k] <= (int64_t)b.size());
      REQUIRE(ix.len[k] <= 4 * n2w);
    }
  }
  ix.count = found;
  return rc;
}

// range by range through windows of `win` bytes, as the pipeline calls it
// (each window copied to a buffer of its exact size) -> true when accepted
static bool scan_windows(const Bytes& b, int n2w, int64_t win, Index& ix) {
  ix.off.assign(kCap, 0);
  ix.len.assign(kCap, 0);
  ix.exps.assign(kCap, 0);
  int64_t pos = 0, e0 = 0;
  while (true) {
    const int64_t n = std::min<int64_t>(win, (int64_t)b.size() - pos);
    const bool last = pos + n == (int64_t)b.size();
    const Bytes w(b.begin() + pos, b.begin() + pos + n);
    int64_t found = 0, next = 0;
    const int rc = xhe_wire_scan(w.data(), n, e0, last, n2w, ix.off.data() + e0, ix.len.data() + e0,
                                 ix.exps.data() + e0, kCap - e0, &found, &next, ix.shape, &ix.ndim);
    if (rc != XHE_OK) return false;
    REQUIRE(next >= 0 && next <= n);
    for (int64_t k = e0; k < e0 + found; ++k) {
      REQUIRE((int64_t)ix.off[k] + ix.len[k] <= n);
      ix.off[k] += (uint32_t)pos;  // -> offsets in the payload
    }
    e0 += found;
    if (last) break;
    if (next == 0) return false;  // no whole element in a window: the pipeline gives up
    pos += next;
  }
  ix.count = e0;
  return true;
}

static void same_index(const Index& a, const Index& b) {
  REQUIRE(a.count == b.count && a.ndim == b.ndim);
  for (int d = 0; d < a.ndim; ++d) REQUIRE(a.shape[d] == b.shape[d]);
  for (int64_t k = 0; k < a.count; ++k)
    REQUIRE(a.off[k] == b.off[k] && a.len[k] == b.len[k] && a.exps[k] == b.exps[k]);
}

// an accepted scan against xhe_wire_decode on the same bytes
static void against_decode(const Bytes& b, int n2w, const Index& ix) {
  static std::vector<uint32_t> ct;
  static std::vector<int32_t> ex(kCap);
  ct.assign((size_t)kCap * n2w, 0xdeadbeefu);
  int64_t count = -1, shape[8];
  int ndim = -1;
  REQUIRE(xhe_wire_decode(b.data(), (int64_t)b.size(), n2w, ct.data(), ex.data(), kCap, &count, shape, &ndim) ==
          XHE_OK);
  REQUIRE(count == ix.count && ndim == ix.ndim);
  for (int d = 0; d < ndim; ++d) REQUIRE(shape[d] == ix.shape[d]);
  std::vector<uint8_t> row((size_t)4 * n2w);
  for (int64_t k = 0; k < count; ++k) {
    REQUIRE(ex[k] == ix.exps[k]);
    std::memset(row.data(), 0, row.size());
    std::memcpy(row.data(), b.data() + ix.off[k], ix.len[k]);
    REQUIRE(std::memcmp(row.data(), &ct[(size_t)k * n2w], row.size()) == 0);
  }
}

// whole scan, windowed scan and decode on the same bytes -> accepted
static bool check(const Bytes& b, int n2w) {
  if (b.empty()) return false;  // the C ABI rejects len <= 0
  Index whole, win;
  const int rc = scan_whole(b, n2w, whole);
  REQUIRE(rc == XHE_OK || rc == XHE_ENOTSUP);
  const bool w = scan_windows(b, n2w, 4096, win);
  if (rc != XHE_OK) {
    REQUIRE(!w);  // no partial acceptance through windows either
    ++g_refused;
    return false;
  }
  against_decode(b, n2w, whole);
  REQUIRE(w);
  same_index(whole, win);
  ++g_accepted;
  return true;
}

// Every truncation of a payload. A cut at k leaves the elements before the
// one it falls in untouched, so the scan of the cut payload is the clean
// scan up to that element's boundary (checked once, by check(seed)) followed
// by the last range from there - which is run here for every k; cuts inside
// the header and the first element are run from byte 0. No cut payload may be
// accepted (the footer must end it).
static void truncations(const Bytes& seed, int n2w, const Index& clean) {
  std::vector<int64_t> start((size_t)clean.count + 1);  // element boundaries, from a windowed scan's `next`s
  {
    int64_t found = 0, next = 0, shape[8];
    int ndim;
    std::vector<uint32_t> off(1);
    std::vector<uint16_t> len(1);
    std::vector<int32_t> ex(1);
    int64_t pos = 0;
    for (int64_t e = 0; e <= clean.count; ++e) {
      start[(size_t)e] = pos;
      if (e == clean.count) break;
      // one element per call: a window that ends two bytes behind it
      int64_t hi = (int64_t)clean.off[e] + clean.len[e];
      int rc = XHE_ENOTSUP;
      for (int64_t n = hi - pos; pos + n <= (int64_t)seed.size() && n < hi - pos + 24; ++n) {
        rc = xhe_wire_scan(seed.data() + pos, n, e, 0, n2w, off.data(), len.data(), ex.data(), 1, &found, &next,
                           shape, &ndim);
        REQUIRE(rc == XHE_OK);
        if (found == 1) break;
      }
      REQUIRE(found == 1);
      pos += next;
    }
  }
  Index ix;
  for (int64_t e = 0; e <= clean.count; ++e) {
    // (from the element before the cut's: a cut at a boundary is not empty)
    const int64_t from = e <= 1 ? 0 : start[(size_t)e - 1];
    const int64_t e0 = e <= 1 ? 0 : e - 1;
    const int64_t to = e < clean.count ? start[(size_t)e + 1] : (int64_t)seed.size();
    for (int64_t k = std::max<int64_t>(start[(size_t)e], 1); k < to; ++k) {
      const Bytes cut(seed.begin() + from, seed.begin() + k);
      int64_t found = 0, next = 0;
      ix.off.assign(8, 0);
      ix.len.assign(8, 0);
      ix.exps.assign(8, 0);
      int rc = xhe_wire_scan(cut.data(), (int64_t)cut.size(), e0, 1, n2w, ix.off.data(), ix.len.data(),
                             ix.exps.data(), 8, &found, &next, ix.shape, &ix.ndim);
      REQUIRE(rc == XHE_ENOTSUP);
      // the same bytes as a range that is not the last: whole elements only, inside the range
      rc = xhe_wire_scan(cut.data(), (int64_t)cut.size(), e0, 0, n2w, ix.off.data(), ix.len.data(), ix.exps.data(),
                         8, &found, &next, ix.shape, &ix.ndim);
      REQUIRE(rc == XHE_OK || rc == XHE_ENOTSUP);
      if (rc == XHE_OK) {
        REQUIRE(next <= (int64_t)cut.size() && found <= 2);
        for (int64_t j = 0; j < found; ++j) REQUIRE((int64_t)ix.off[j] + ix.len[j] <= next);
      }
      ++g_refused;
    }
  }
}

static void fuzz_seed(const Bytes& seed, int n2w, std::mt19937_64& rng) {
  Index clean;
  REQUIRE(scan_whole(seed, n2w, clean) == XHE_OK);
  REQUIRE(check(seed, n2w));
  truncations(seed, n2w, clean);
  // byte flips: anywhere, and in the bytes around a value's start and end
  // (opcodes, memo indices, the length field, the exponent)
  const int flips = clean.count > 100 ? 300 : 2000;
  for (int t = 0; t < flips; ++t) {
    Bytes m = seed;
    const int nf = 1 + (int)(rng() % 3);
    for (int f = 0; f < nf; ++f) {
      size_t at = rng() % m.size();
      if (t % 2 && clean.count) {
        const int64_t e = (int64_t)(rng() % (uint64_t)clean.count);
        const int64_t edge = (rng() & 1) ? (int64_t)clean.off[e] - 14 : (int64_t)clean.off[e] + clean.len[e] - 2;
        at = (size_t)std::min<int64_t>((int64_t)m.size() - 1, std::max<int64_t>(0, edge + (int64_t)(rng() % 16)));
      }
      m[at] = (uint8_t)rng();
    }
    check(m, n2w);
  }
  // inflated value length fields (LONG1: one byte, LONG4: four), first,
  // last and block-boundary elements
  static const uint64_t big[] = {~0ull, 0x7fffffffull, 0xffffffffull, 0x80000000ull, 0xffull, 0x7full, 0x10000ull};
  for (int64_t e = 0; e < clean.count; ++e) {
    if (!(e < 3 || e + 2 >= clean.count || (e % 1000 >= 998 || e % 1000 <= 1))) continue;
    // the length field lies right below the value, or below its sign byte's position
    for (int lb : {1, 4}) {
      const int64_t at = (int64_t)clean.off[e] - lb;
      if (at < 1 || seed[(size_t)at - 1] != (lb == 1 ? 0x8a : 0x8b)) continue;
      for (uint64_t v : big) {
        Bytes m = seed;
        for (int i = 0; i < lb; ++i) m[(size_t)at + i] = (uint8_t)(v >> (8 * i));
        check(m, n2w);
      }
    }
  }
}

static Bytes read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return Bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static int scan_mode(int argc, char** argv) {
  std::mt19937_64 rng(17);
  const int n2w = std::atoi(argv[2]);
  int own = 0, foreign = 0;
  for (int a = 3; a < argc; ++a) {
    const Bytes seed = read_file(argv[a]);
    REQUIRE(!seed.empty());
    if (std::string(argv[a]).find("foreign") != std::string::npos) {  // another pickle form: refused, whole and in windows
      REQUIRE(!check(seed, n2w));
      ++foreign;
    } else {
      fuzz_seed(seed, n2w, rng);
      ++own;
    }
  }
  std::printf("own %d foreign %d accepted %ld refused %ld\n", own, foreign, g_accepted, g_refused);
  return 0;
}

// ---------------------------------------------------------------- unpack
// row of n2w words from (bytes, off, len) the plain way: bytes outside the
// buffer are zero, len is cut to the row
static void unpack_ref(const Bytes& b, uint32_t off, uint32_t len, int n2w, std::vector<uint8_t>& row) {
  row.assign((size_t)4 * n2w, 0);
  const int64_t used = std::min<int64_t>(len, 4 * (int64_t)n2w);
  for (int64_t j = 0; j < used; ++j)
    if ((int64_t)off + j < (int64_t)b.size()) row[(size_t)j] = b[(size_t)((int64_t)off + j)];
}

static long unpack_case(const Bytes& b, uint32_t off, uint32_t len, int n2w) {
  std::vector<uint8_t> want;
  unpack_ref(b, off, len, n2w, want);
  for (int q = 0; q < n2w / 4; ++q) {
    uint32_t w[4];
    xhe::wireu::unpack_quad(b.data(), (int64_t)b.size(), off, len, n2w, q, w);
    REQUIRE(std::memcmp(w, want.data() + 16 * q, 16) == 0);
  }
  return 1;
}

static int unpack_mode() {
  std::mt19937_64 rng(29);
  long cases = 0;
  for (int n2w : {128, 192, 256, 512}) {
    const uint32_t lens[] = {0, 1, 3, 4, 5, 15, 16, 17, (uint32_t)(4 * n2w - 1), (uint32_t)(4 * n2w)};
    for (int res = 0; res < 16; ++res) {
      for (uint32_t len : lens) {
        // the value in the middle of a buffer, and ending exactly at its end
        // (for every size of the buffer's last, partial dword)
        for (int tail : {64, 0}) {
          const uint32_t off = 48 + (uint32_t)res;
          Bytes b((size_t)off + len + tail);
          for (auto& x : b) x = (uint8_t)(rng() | 1);  // no zero bytes: a wrong mask or shift shows
          cases += unpack_case(b, off, len, n2w);
        }
      }
    }
    // hostile indices: whatever they hold, no read leaves the buffer
    for (size_t nbytes : {(size_t)1, (size_t)5, (size_t)64, (size_t)4 * n2w + 7, (size_t)8 * n2w + 2}) {
      Bytes b(nbytes);
      for (auto& x : b) x = (uint8_t)(rng() | 1);
      const uint32_t nb = (uint32_t)nbytes;
      const uint32_t offs[] = {0, 1, nb - 1, nb, nb + 1, nb + 3, nb + 4, nb + 17, 0x7fffffffu, 0x80000000u, 0xfffffff0u,
                               0xfffffffdu, 0xffffffffu};
      const uint32_t hl[] = {0, 1, 17, (uint32_t)(4 * n2w), (uint32_t)(4 * n2w + 1), 0xffffu, 0x10000u, 0x7fffffffu,
                             0xffffffffu};
      for (uint32_t off : offs)
        for (uint32_t len : hl) cases += unpack_case(b, off, len, n2w);
    }
  }
  std::printf("unpack cases %ld\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && std::string(argv[1]) == "scan") return scan_mode(argc, argv);
  if (argc == 2 && std::string(argv[1]) == "unpack") return unpack_mode();
  std::fprintf(stderr, "usage: wire_scan_fuzz scan N2W SEED... | unpack\n");
  return 2;
}
