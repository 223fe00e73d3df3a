// xhe: C-ABI over the gfx950 Paillier kernels (see include/xhe.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <memory>
#include <mutex>
#include <atomic>
#include <stdexcept>
#include <unordered_map>
#include <utility>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/xhe.h"
#include "abi_common.hpp"
#include "hostbn.hpp"
#include "keyconst.hpp"
#include "paths.hpp"
#include "scan_plan.hpp"
#include "xhe_kernels.hpp"
#include "fermat_dev.hpp"
#include "dec_wave.hpp"
#include "barrett_dev.hpp"
#include "rns_dev.hpp"
#include "enc_obf_dev.hpp"
#include "wire_unpack.hpp"

using namespace xhe;

namespace {

int fail(int code, const std::string& msg) { return xhe_fail(code, msg); }

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t _e = (x);                                                                   \
    if (_e != hipSuccess) throw HipError(std::string(#x) + ": " + hipGetErrorString(_e)); \
  } while (0)

// Every kernel launch of this file: no dynamic LDS, launch errors thrown.
// The arguments convert to the kernel's parameters implicitly, as in a direct
// hipLaunchKernelGGL (nullptr and int literals included).
template <class... KArgs, class... Args>
void launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, hipStream_t s, Args&&... args) {
  hipLaunchKernelGGL(kernel, grid, block, 0, s, std::forward<Args>(args)...);
  HIPCHK(hipGetLastError());
}

// The kernel switches ($XHE_*; INTEGRATION.md "Other kernel switches"), read
// together once per process; paths.hpp turns them into kernel paths.
const paths::Pins& pins() {
  static const paths::Pins p = paths::parse_pins(getenv);
  return p;
}
// A path the planner chose that this key size has no kernels for (guarded:
// XHE_EINVAL).
[[noreturn]] void no_path(const char* what) {
  throw std::logic_error(std::string(what) + ": no such kernel path for this key size");
}

// The host-side settings (chunking, tracing, test hooks, window bits). The
// callers keep the value in a function-local static: read once per process.
const char* env_str(const char* name) { return getenv(name); }
int64_t env_int(const char* name, int64_t dflt) {
  const char* e = env_str(name);
  return e ? atoll(e) : dflt;
}

// ------------------------------------------------------------------ shapes
// Limb shapes per key size: MP2 for residues mod p^2/q^2, MP for mod p/q.
struct Shape2048 {
  static constexpr int K = 2048, RW = K / 32, RW2 = K / 16;  // packed table row words mod p^2 / n^2
  using MP2 = Mont<74, 28, 1>;
  using MP2L = Mont<76, 28, 4>;   // low-latency (small-batch) decrypt shape
  using MP2X = Mont<80, 28, 16>;  // lowest latency: one 16-lane DPP row per residue (tiny batches)
  using MP = Mont<37, 28, 1>;
  using MN2 = Mont<152, 27, 4>;
  using MN2X = Mont<160, 27, 16>;  // n^2 ops on small batches: one 16-lane DPP row per residue
};
struct Shape3072 {
  static constexpr int K = 3072, RW = K / 32, RW2 = K / 16;  // packed table row words mod p^2 / n^2
  using MP2 = Mont<110, 28, 2>;
  using MP2L = Mont<112, 28, 4>;
  using MP2X = Mont<112, 28, 16>;
  using MP = Mont<56, 28, 2>;
  using MN2 = Mont<228, 27, 4>;
  using MN2X = Mont<240, 27, 16>;
  using PDX = PMDX<60, 2>;   // Montgomery digits mod p^2, q^2: k_djn_pmdx's products (2 lanes of 30 limbs)
  using PDXO = PMDX<60, 4>;  // its conversions (k_pmdx_enc_out, k_tab_to_pmdx; 2 lanes would spill there)
  using PDXP = PMDX<60, 4>;  // the decrypt exponentiation (2 lanes spill 70 VGPRs in pmdx_pow_uniform)
};
// 4096-bit keys (the LR/LinReg/Pearson/WoE operators' OneOf(2048, 4096, 8192)):
// 28-bit limbs would overflow the lazy 64-bit accumulator at S = 147
// ((2S+2) 2^56 >= 2^64), so every modulus uses 27-bit limbs. p^2 residues
// take 4 lanes (38 limbs each), n^2 residues one 16-lane DPP row (19 each)
// in both the batch and the small-batch shapes; the mod-p limbs share W with
// p^2 so k_dec_fin reads k_dec_pow's rows unchanged.
struct Shape4096 {
  static constexpr int K = 4096, RW = K / 32, RW2 = K / 16;  // packed table row words mod p^2 / n^2
  using MP2 = Mont<152, 27, 4>;
  using MP2L = Mont<152, 27, 4>;
  using MP2X = Mont<160, 27, 16>;
  using MP = Mont<76, 27, 4>;
  using MN2 = Mont<304, 27, 16>;
  using MN2X = Mont<304, 27, 16>;
  using PDX = PMDX<80, 4>;
  using PDXO = PMDX<80, 4>;
  using PDXP = PMDX<80, 4>;
};

// 8192-bit keys: p^2 (8192 bits) in one 16-lane row of 27-bit limbs, p in 4
// lanes; n^2 (16384 bits) needs 26-bit limbs for the lazy accumulator
// ((2S+2) 2^52 < 2^64 at S = 640), 40 per lane of a 16-lane row.
struct Shape8192 {
  static constexpr int K = 8192, RW = K / 32, RW2 = K / 16;  // packed table row words mod p^2 / n^2
  using MP2 = Mont<304, 27, 16>;
  using MP2L = Mont<304, 27, 16>;
  using MP2X = Mont<304, 27, 16>;
  using MP = Mont<152, 27, 4>;
  using MN2 = Mont<640, 26, 16>;
  using MN2X = Mont<640, 26, 16>;
  // Montgomery digits mod p^2, q^2 (4096-bit primes: 160 limbs of 27 bits,
  // R = 2^4320): the products (encrypt and decrypt exponentiations) on half
  // rows, 8 lanes of 20 limbs (no spills: 170 / 230 VGPRs); the conversions
  // on whole 16-lane rows (8 lanes spill 44 VGPRs in k_pmdx_enc_out)
  using PDX = PMDX<160, 8>;
  using PDXO = PMDX<160, 16>;
  using PDXP = PMDX<160, 8>;
};

// XHE_ONLY_BITS=K (XHE_ONLY_2048 = 2048): a development build with one key
// size's shapes only (a fraction of the compile time, for kernel A/B runs
// through $XHE_LIB); the shipped library has every key size.
#if defined(XHE_ONLY_2048) && !defined(XHE_ONLY_BITS)
#define XHE_ONLY_BITS 2048
#endif
#ifdef XHE_ONLY_BITS
constexpr bool key_bits_supported(int K) { return K == XHE_ONLY_BITS; }
template <class F>
decltype(auto) with_shape(int, F&& f) {
  if constexpr (XHE_ONLY_BITS == 2048) return f(Shape2048{});
  else if constexpr (XHE_ONLY_BITS == 3072) return f(Shape3072{});
  else if constexpr (XHE_ONLY_BITS == 4096) return f(Shape4096{});
  else return f(Shape8192{});
}
#else
constexpr bool key_bits_supported(int K) { return K == 2048 || K == 3072 || K == 4096 || K == 8192; }

// Calls f(ShapeK{}) for the key size K (checked at xhe_key_create).
template <class F>
decltype(auto) with_shape(int K, F&& f) {
  if (K == 2048) return f(Shape2048{});
  if (K == 3072) return f(Shape3072{});
  if (K == 4096) return f(Shape4096{});
  return f(Shape8192{});
}
#endif

// Shapes that only 2048-bit keys have:
using ND2048 = PMDX<80, 4>;           // Montgomery digits mod n^2 (k_ndig_*, k_djn_pub_nd)
using WaveN2 = WaveMont<154, 16, 27>;  // one-block products mod n^2 (k_*_wave<WaveN2::K_, 16>)

// Prime search (k_fermat2, fermat_dev.hpp): a candidate prime of K/2 bits per
// lane group, the shapes with the fewest limbs per lane (L = 5, 7, 5, 10):
// the launch is as long as one candidate's chain of squarings.
constexpr bool fermat_bits_supported(int bits) { return key_bits_supported(2 * bits); }
template <int B>
using FermatBits = std::integral_constant<int, B>;
template <class F>
void with_fermat_shape(int bits, F&& f) {
#ifdef XHE_ONLY_BITS
  (void)bits;
  if constexpr (XHE_ONLY_BITS == 2048) f(Mont<40, 28, 8>{}, FermatBits<1024>{});
  else if constexpr (XHE_ONLY_BITS == 3072) f(Mont<56, 28, 8>{}, FermatBits<1536>{});
  else if constexpr (XHE_ONLY_BITS == 4096) f(Mont<80, 28, 16>{}, FermatBits<2048>{});
  else f(Mont<160, 27, 16>{}, FermatBits<4096>{});
#else
  if (bits == 1024) f(Mont<40, 28, 8>{}, FermatBits<1024>{});
  else if (bits == 1536) f(Mont<56, 28, 8>{}, FermatBits<1536>{});
  else if (bits == 2048) f(Mont<80, 28, 16>{}, FermatBits<2048>{});
  else f(Mont<160, 27, 16>{}, FermatBits<4096>{});
#endif
}

}  // namespace

struct xhe_key {
  int device = 0;
  int K = 0, nw = 0, n2w = 0;
  bool priv = false, djn = false;
  int rand_bits = 0, rand_words = 0;
  uint32_t* d_blob = nullptr;
  uint32_t* d_tab = nullptr;
  KeyDev kd{};
  std::vector<uint32_t> n_host;   // n words (for host-side checks)
  std::vector<uint32_t> n2_host;  // n^2 words (host inverse at the batch-inversion root)
  int n_bits = 0;
  int dneg = 0;  // smallest d with 1 << d >= min_value_for_negative (= n - n // 3): alignment gaps from
                 // here on take _raw_mul's negative branch (paillier.py:79-86, 173-187)
};

namespace {

struct DevGuard {
  int prev = -1;
  explicit DevGuard(int dev) {
    HIPCHK(hipGetDevice(&prev));
    if (prev != dev) HIPCHK(hipSetDevice(dev));
  }
  ~DevGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

template <class MP2, int RW>
void build_tables_m(xhe_key* k, const ModDev& md, const uint32_t* d_hM, uint32_t* d_tab, uint32_t* d_chain,
                    uint32_t* d_ws, hipStream_t s);

int64_t chain_rows_h(int win) { return ((int64_t)1 << (win / 2)) + ((int64_t)1 << (win - win / 2)); }

// Tables of one modulus, or of p^2 and q^2 concurrently on two streams.
template <class MP2, int RW>
void build_tables_sync(xhe_key* k, const ModDev* md, const uint32_t* const* d_hM, uint32_t* const* d_tab, int count) {
  hipStream_t st[2] = {nullptr, nullptr};
  uint32_t* ws[2] = {nullptr, nullptr};
  uint32_t* chain[2] = {nullptr, nullptr};
  const int win = k->kd.win, nwin = k->kd.nwin, nhi = k->kd.nhi;
  const size_t chain_words =
      (size_t)std::max<int64_t>(nhi ? (nhi + 1) * chain_rows_h(win + 1) : 0, (nwin - nhi) * chain_rows_h(win)) *
      MP2::S4;
  for (int i = 0; i < count; ++i) {
    HIPCHK(hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking));
    HIPCHK(hipMalloc(&ws[i], MP2::S4 * sizeof(uint32_t) * 4));
    HIPCHK(hipMalloc(&chain[i], chain_words * sizeof(uint32_t)));
    build_tables_m<MP2, RW>(k, md[i], d_hM[i], d_tab[i], chain[i], ws[i], st[i]);
  }
  for (int i = 0; i < count; ++i) {
    HIPCHK(hipStreamSynchronize(st[i]));
    HIPCHK(hipFree(ws[i]));
    HIPCHK(hipFree(chain[i]));
    HIPCHK(hipStreamDestroy(st[i]));
  }
}

// One uniform table segment (nwin windows of win bits starting at base
// d_base), enqueued on `s` (no synchronisation; d_ws and d_chain must stay
// alive until s has drained): window bases (low entry 1 of every window) =
// base^(2^(win w)) by one squaring chain over nbases >= nwin windows, every
// window's low and high chains by doubling levels (k_tab_level: log2 depth
// instead of 2^(win/2)) - build_chains_seg - then every packed row as one
// product of a high and a low entry.
template <class MP2>
void build_chains_seg(const ModDev& md, const uint32_t* d_base, int win, int nwin, int nbases, uint32_t* d_chain,
                      uint32_t* d_ws, hipStream_t s) {
  const int half = win / 2;
  launch(k_tab_bases<MP2>, dim3(1), dim3(64), s, md, d_base, win, nbases, d_chain, d_ws);
  auto blocks = [&](int64_t groups) { return dim3((unsigned)std::max<int64_t>(1, (groups * MP2::TPI + 255) / 256)); };
  launch(k_tab_one<MP2>, blocks(nwin), dim3(256), s, md, win, nwin, d_chain);
  const int lim_lo = (1 << half) + 1, lim_hi = 1 << (win - half);
  for (int t = 0; (1 << t) < lim_lo - 1; ++t) {
    launch(k_tab_level<MP2>, blocks((int64_t)nwin << t), dim3(256), s, md, md.N, win, nwin, t, 0, lim_lo, d_chain);
  }
  for (int t = 0; (1 << t) < lim_hi - 1; ++t) {
    launch(k_tab_level<MP2>, blocks((int64_t)nwin << t), dim3(256), s, md, md.N, win, nwin, t, half, lim_hi, d_chain);
  }
}

template <class MP2, int RW>
void build_tables_seg(const ModDev& md, const uint32_t* d_base, int win, int nwin, int nbases, uint32_t* d_tab,
                      int64_t rs, uint32_t* d_chain, uint32_t* d_ws, hipStream_t s) {
  build_chains_seg<MP2>(md, d_base, win, nwin, nbases, d_chain, d_ws, s);
  auto blocks = [&](int64_t groups) { return dim3((unsigned)std::max<int64_t>(1, (groups * MP2::TPI + 255) / 256)); };
  int64_t rows = (int64_t)nwin << win;
  launch((k_tab_combine<MP2, RW>), blocks(rows), dim3(256), s, md, md.N, win, nwin, d_chain, d_tab, rs);
}

// A key's tables (layout win_layout / win_digit): uniform, or the nhi wide
// windows first, whose base chain runs one window further to
// h^(2^(nhi (win+1))), the base of the narrow windows that follow.
template <class MP2, int RW>
void build_tables_m(xhe_key* k, const ModDev& md, const uint32_t* d_hM, uint32_t* d_tab, uint32_t* d_chain,
                    uint32_t* d_ws, hipStream_t s) {
  const int win = k->kd.win, nwin = k->kd.nwin, nhi = k->kd.nhi;
  const int64_t rs = RW == k->K / 32 ? k->kd.tab_rs : RW;  // p^2/q^2 rows (maybe interleaved) or n^2 rows
  if (nhi == 0) {
    build_tables_seg<MP2, RW>(md, d_hM, win, nwin, nwin, d_tab, rs, d_chain, d_ws, s);
    return;
  }
  uint32_t* base2 = d_ws + 2 * MP2::S4;  // d_ws rows: 0 = squaring scratch, 2 = the narrow windows' base
  build_tables_seg<MP2, RW>(md, d_hM, win + 1, nhi, nhi + 1, d_tab, rs, d_chain, d_ws, s);
  HIPCHK(hipMemcpyAsync(base2, d_chain + ((size_t)nhi * chain_rows_h(win + 1) + 1) * MP2::S4,
                        MP2::S4 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  build_tables_seg<MP2, RW>(md, base2, win, nwin - nhi, nwin - nhi, d_tab + ((size_t)nhi << (win + 1)) * rs, rs,
                            d_chain, d_ws, s);
}

// The chains alone of a key's table layout for the base d_hM in shape M, kept
// side by side for k_tab_to_pmd (the wide windows' chains first, then the
// narrow ones' from row nhi chain_rows(win + 1)), enqueued on `s`. d_chain:
// inv_chain_words<M>() words, d_ws: 4 rows.
template <class M>
size_t inv_chain_words(const KeyDev& kd) {
  return (size_t)(kd.nhi * chain_rows_h(kd.win + 1) + (kd.nwin - kd.nhi) * chain_rows_h(kd.win)) * M::S4;
}
template <class M>
void build_chains_m(const KeyDev& kd, const ModDev& md, const uint32_t* d_hM, uint32_t* d_chain, uint32_t* d_ws,
                    hipStream_t s) {
  const int win = kd.win, nwin = kd.nwin, nhi = kd.nhi;
  if (nhi == 0) {
    build_chains_seg<M>(md, d_hM, win, nwin, nwin, d_chain, d_ws, s);
    return;
  }
  // the base chain's last entry (window nhi) lands on the narrow chains'
  // first rows: copied out before they are built
  uint32_t* base2 = d_ws + 2 * M::S4;
  uint32_t* narrow = d_chain + (size_t)nhi * chain_rows_h(win + 1) * M::S4;
  build_chains_seg<M>(md, d_hM, win + 1, nhi, nhi + 1, d_chain, d_ws, s);
  HIPCHK(hipMemcpyAsync(base2, narrow + M::S4, M::S4 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  build_chains_seg<M>(md, base2, win, nwin - nhi, nwin - nhi, narrow, d_ws, s);
}

// The shapes keyconst.hpp derives a key's constants for, read from the types
// of the kernels that use them.
template <class Sh>
KeySpec key_spec(const xhe_key* k, int win) {
  KeySpec s{};
  s.K = Sh::K;
  s.priv = k->priv;
  s.djn = k->djn;
  s.win = win & 0xff;
  s.split = (win & XHE_WIN_SPLIT) != 0;
  s.mp2 = {Sh::MP2::S, Sh::MP2::W};
  s.mp2L = {Sh::MP2L::S, Sh::MP2L::W};
  s.mp2X = {Sh::MP2X::S, Sh::MP2X::W};
  s.mp = {Sh::MP::S, Sh::MP::W};
  s.mn2 = {Sh::MN2::S, Sh::MN2::W};
  s.mn2X = {Sh::MN2X::S, Sh::MN2X::W};
  if constexpr (Sh::K == 2048) {
    s.nd = {ND2048::K, ND2048::W};
    // the one-lane digit kernels are instantiated on 37 limbs (k_djn_pmd<MP2, 37>,
    // k_dec_pmd_*<37>): the mod-p limbs, whose R mod P they read as kd.p.R1
    static_assert(Sh::MP::S == 37 && Sh::MP::W == 28, "k_*_pmd<37> run on the mod-p limbs");
    s.pmd = s.mp;
    s.wave = {WaveN2::K_, WaveN2::W};
    static_assert(bar::S == Sh::MN2::S && bar::W == Sh::MN2::W, "Barrett constants are for 2048-bit keys");
    s.bar = {bar::S, bar::W};
  } else {
    using D = typename Sh::PDX;  // products, conversions and the decrypt share the digits
    static_assert(D::K == Sh::PDXO::K && D::K == Sh::PDXP::K, "one digit modulus per key size");
    s.pd = {D::K, D::W};
  }
  return s;
}

int64_t table_rows(const KeyDev& kd) { return (int64_t)(kd.nwin + kd.nhi) << kd.win; }

// Rewrites table rows as Montgomery digits in place: one launch per table
// (tpr threads per row), then a device synchronisation.
template <class F>
void rows_to_digits(int64_t rows, int tpr, unsigned block, int ntab, F&& launch_one) {
  const dim3 grid((unsigned)((rows * tpr + block - 1) / block));
  for (int i = 0; i < ntab; ++i) launch_one(i, grid, dim3(block));
  HIPCHK(hipDeviceSynchronize());
}

// Private DJN keys: h^(d 2^..) mod p^2 and mod q^2 as packed rows of Shape::RW
// = K/32 words (p^2 < 2^K), then rewritten as the digit rows k_djn_pmd reads
// (2048: the first digit e and the log digit lhat, k_tab_to_pmd) or the digit
// pairs (e, f) of k_djn_pmdx.
void build_private_tables(xhe_key* k, const KeyImage& im) {
  KeyDev& kd = k->kd;
  const int64_t rows = table_rows(kd);
  const size_t tab_words = (size_t)rows * (size_t)(k->K / 32);
  HIPCHK(hipMalloc(&k->d_tab, 2 * tab_words * sizeof(uint32_t)));
  kd.tab_rs = k->K / 32;
  kd.tab_p2 = k->d_tab;
  kd.tab_q2 = k->d_tab + tab_words;
  const ModDev mds[2] = {kd.p2, kd.q2};
  const uint32_t* hms[2] = {k->d_blob + im.hM_p2[0], k->d_blob + im.hM_p2[1]};
  uint32_t* tabs[2] = {k->d_tab, k->d_tab + tab_words};
  with_shape(k->K, [&](auto sh) {
    using Sh = decltype(sh);
    if constexpr (Sh::K == 2048) {
      // the chains of h^-1 mod p, q (the rows' inverses for their log digits),
      // on streams of their own under the table build
      using MP = typename Sh::MP;
      const ModDev mp[2] = {kd.p, kd.q};
      hipStream_t st[2];
      uint32_t *inv[2], *ws[2];
      for (int i = 0; i < 2; ++i) {
        HIPCHK(hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking));
        HIPCHK(hipMalloc(&inv[i], inv_chain_words<MP>(kd) * sizeof(uint32_t)));
        HIPCHK(hipMalloc(&ws[i], MP::S4 * sizeof(uint32_t) * 4));  // rows 0, 2: build_chains_m; 3: the base
        uint32_t* base = ws[i] + 3 * MP::S4;
        HIPCHK(hipMemcpy(base, im.hinvM_p[i].data(), MP::S4 * sizeof(uint32_t), hipMemcpyHostToDevice));
        build_chains_m<MP>(kd, mp[i], base, inv[i], ws[i], st[i]);
      }
      build_tables_sync<typename Sh::MP2, Sh::RW>(k, mds, hms, tabs, 2);
      for (int i = 0; i < 2; ++i) HIPCHK(hipStreamSynchronize(st[i]));
      kd.pmd = 1;
      rows_to_digits(rows, 1, 256, 2, [&](int i, dim3 grid, dim3 block) {
        launch((k_tab_to_pmd<MP, Sh::RW>), grid, block, nullptr, mp[i], mp[i].N, inv[i], kd.win, kd.nhi, tabs[i], rows,
               (int64_t)kd.tab_rs);
      });
      for (int i = 0; i < 2; ++i) {
        HIPCHK(hipFree(inv[i]));
        HIPCHK(hipFree(ws[i]));
        HIPCHK(hipStreamDestroy(st[i]));
      }
    } else {
      build_tables_sync<typename Sh::MP2, Sh::RW>(k, mds, hms, tabs, 2);
      kd.pmdx = 1;
      using D = typename Sh::PDXO;
      rows_to_digits(rows, D::TPI, 128, 2, [&](int i, dim3 grid, dim3 block) {
        launch((k_tab_to_pmdx<D, Sh::RW>), grid, block, nullptr, kd, i, tabs[i], rows, (int64_t)kd.tab_rs);
      });
    }
  });
}

// Public DJN keys: h^(d 2^(win w)) mod n^2 as packed rows of Shape::RW2 = n2w
// words, uniform windows; at 2048 bits rewritten as canonical Montgomery
// digits of n (e, f < n: 64 + 64 words, still 512 B) for k_djn_pub_nd.
void build_public_tables(xhe_key* k, const KeyImage& im) {
  KeyDev& kd = k->kd;
  const int64_t rows = table_rows(kd);
  HIPCHK(hipMalloc(&k->d_tab, (size_t)rows * (size_t)(k->K / 16) * sizeof(uint32_t)));
  kd.tab_n2 = k->d_tab;
  const uint32_t* hm = k->d_blob + im.hM_n2;
  uint32_t* tab = k->d_tab;
  with_shape(k->K, [&](auto sh) {
    using Sh = decltype(sh);
    build_tables_sync<typename Sh::MN2, Sh::RW2>(k, &kd.n2, &hm, &tab, 1);
    if constexpr (Sh::K == 2048) {
      if (!pins().ndig_pub) return;  // Montgomery n^2 tables kept (k_djn_pub; A/B)
      kd.pub_nd = 1;
      rows_to_digits(rows, ND2048::TPI, 128, 1, [&](int, dim3 grid, dim3 block) {
        launch((k_tab_to_pmdx<ND2048, Sh::RW2>), grid, block, nullptr, kd, 2, tab, rows, (int64_t)Sh::RW2);
      });
    }
  });
}

// Derive the constants on the host (keyconst.hpp), upload them as one blob,
// point the KeyDev into it, then build the DJN fixed-base tables.
void key_create_impl(xhe_key* k, const BigU& n, const BigU* p, const BigU* q, const BigU* h, int win) {
  const KeySpec spec = with_shape(k->K, [&](auto sh) { return key_spec<decltype(sh)>(k, win); });
  const KeyImage im = derive_key_constants(spec, n, p, q, h);
  k->rand_bits = im.rand_bits;
  k->rand_words = im.rand_words;
  HIPCHK(hipMalloc(&k->d_blob, im.words.size() * sizeof(uint32_t)));
  HIPCHK(hipMemcpy(k->d_blob, im.words.data(), im.words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  k->kd = im.bind(k->d_blob);
  if (!k->djn) return;
  if (k->priv) build_private_tables(k, im);
  else build_public_tables(k, im);
}

// Workspaces of the kernel entry points. Normally stream-ordered pool
// allocations; inside a host pipeline's chunk (t_ws set) they come from that
// chunk slot's cache and are kept for the whole call: with the pool, a
// workspace freed on one slot's stream and wanted by the next slot's call
// made hipMallocAsync hold the host until the first stream drained, which
// serialised the pipeline. Reuse within a slot is safe: its calls run in
// stream order, and a slot is reused only after its stream has drained.
struct WsCache {
  struct Blk {
    void* p;
    size_t bytes;
    bool used;
  };
  std::vector<Blk> blk;
  hipStream_t s = nullptr;
  WsCache() = default;
  WsCache(const WsCache&) = delete;
  WsCache& operator=(const WsCache&) = delete;
  ~WsCache() {
    for (auto& b : blk) (void)hipFreeAsync(b.p, s);
  }
};
thread_local WsCache* t_ws = nullptr;

// Outside a host pipeline, a workspace freed on stream s is kept on s's free
// list for the next call on s (stream order makes that reuse safe) instead of
// going back to the pool: a pipelined Paillier.encrypt alternates its pieces
// between two streams, and a request on one stream for memory the other had
// just freed made hipMallocAsync hold the host until that stream drained
// (the launches serialised behind each other). At most kStreamWsKeep bytes
// are kept per stream; a block is reused for requests of at least half its
// size.
constexpr size_t kStreamWsKeep = (size_t)2 << 30;
struct StreamWs {
  struct Blk {
    void* p;
    size_t bytes;
  };
  std::mutex mu;
  std::unordered_map<hipStream_t, std::vector<Blk>> free;  // oldest first
  std::unordered_map<void*, size_t> size;                  // blocks handed out
};
StreamWs& stream_ws() {
  static StreamWs* w = new StreamWs();  // process lifetime (no teardown order with the runtime)
  return *w;
}

void ws_alloc(void** p, size_t bytes, hipStream_t s) {
  if (t_ws) {
    for (auto& b : t_ws->blk)
      if (!b.used && b.bytes >= bytes) {
        b.used = true;
        *p = b.p;
        return;
      }
    HIPCHK(hipMallocAsync(p, bytes, s));
    t_ws->blk.push_back({*p, bytes, true});
    return;
  }
  StreamWs& w = stream_ws();
  {
    std::lock_guard<std::mutex> g(w.mu);
    auto it = w.free.find(s);
    if (it != w.free.end()) {
      std::vector<StreamWs::Blk>& v = it->second;
      size_t best = v.size();
      for (size_t i = 0; i < v.size(); ++i)
        if (v[i].bytes >= bytes && v[i].bytes / 2 <= bytes && (best == v.size() || v[i].bytes < v[best].bytes))
          best = i;
      if (best < v.size()) {
        *p = v[best].p;
        w.size[*p] = v[best].bytes;
        v.erase(v.begin() + (ptrdiff_t)best);
        return;
      }
    }
  }
  HIPCHK(hipMallocAsync(p, bytes, s));
  std::lock_guard<std::mutex> g(w.mu);
  w.size[*p] = bytes;
}

// Called from WsScope's destructor: errors of the stream-ordered free are
// dropped; a failed host allocation in the bookkeeping (bad_alloc from the
// free lists) ends the process, as in any destructor.
void ws_free(void* p, hipStream_t s) noexcept {
  if (t_ws)
    for (auto& b : t_ws->blk)
      if (b.p == p) {
        b.used = false;
        return;
      }
  StreamWs& w = stream_ws();
  std::vector<void*> drop;
  {
    std::lock_guard<std::mutex> g(w.mu);
    auto it = w.size.find(p);
    if (it == w.size.end()) {
      drop.push_back(p);  // not one of ours (allocated inside a host pipeline's cache, never here)
    } else {
      std::vector<StreamWs::Blk>& v = w.free[s];
      v.push_back({p, it->second});
      w.size.erase(it);
      size_t total = 0;
      for (const auto& b : v) total += b.bytes;
      while (total > kStreamWsKeep && !v.empty()) {
        total -= v.front().bytes;
        drop.push_back(v.front().p);
        v.erase(v.begin());
      }
    }
  }
  for (void* q : drop) (void)hipFreeAsync(q, s);
}

// The workspaces of one entry-point call: get() allocates through ws_alloc;
// at scope exit (also when a launch throws) they go back through ws_free in
// allocation order. That is the order of the explicit frees this replaces,
// and the stream free lists above depend on it: which block the next call
// reuses, and which one is dropped first over kStreamWsKeep.
class WsScope {
  static constexpr int kMax = 8;  // encrypt_impl and dec_pmdx_launch hold 4
  hipStream_t s_;
  void* held_[kMax];
  int n_ = 0;

 public:
  explicit WsScope(hipStream_t s) : s_(s) {}
  WsScope(const WsScope&) = delete;
  WsScope& operator=(const WsScope&) = delete;
  ~WsScope() {
    for (int i = 0; i < n_; ++i) ws_free(held_[i], s_);
  }
  template <class T>
  T* get(size_t bytes) {
    if (n_ == kMax) throw std::logic_error("WsScope: too many workspaces in one call (raise kMax)");
    ws_alloc(&held_[n_], bytes, s_);
    return (T*)held_[n_++];
  }
};

// Owner of a stream-ordered allocation that bypasses the workspace caches.
// Released by a synchronous hipFree, or with kAsync by hipFreeAsync on the
// allocating stream (no host sync: for buffers no host frame feeds). Where a
// call holds several, they are declared empty in reverse and filled in
// allocation order, so that scope exit frees them in allocation order as the
// explicit frees did (the pool hands blocks out by that order).
struct DevBuf {
  enum Release { kSync, kAsync };
  void* p = nullptr;
  hipStream_t s = nullptr;
  Release rel = kSync;
  DevBuf() = default;
  DevBuf(size_t bytes, hipStream_t st, Release r = kSync) : s(st), rel(r) {
    HIPCHK(hipMallocAsync(&p, std::max<size_t>(bytes, 4), s));
  }
  DevBuf(DevBuf&& o) noexcept : p(o.p), s(o.s), rel(o.rel) { o.p = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {  // releases what it held, at this point
    std::swap(p, o.p);
    std::swap(s, o.s);
    std::swap(rel, o.rel);
    o.reset();
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)(rel == kAsync ? hipFreeAsync(p, s) : hipFree(p));
    p = nullptr;
  }
  template <class T>
  T* as() const { return (T*)p; }
};

constexpr int64_t kChunk = 1 << 20;  // elements per launch chunk (bounds workspace)

// ---- optional per-kernel timing (hipEvents on the launch stream)
struct ProfRec {
  std::string name;
  hipEvent_t a, b;
};
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfRec> g_prof;

struct ProfScope {
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t s;
  const char* name;
  bool on;
  ProfScope(const char* n, hipStream_t st) : s(st), name(n) {
    {
      std::lock_guard<std::mutex> lk(g_prof_mu);
      on = g_prof_on;
    }
    if (on) {
      HIPCHK(hipEventCreate(&a));
      HIPCHK(hipEventCreate(&b));
      HIPCHK(hipEventRecord(a, s));
    }
  }
  ~ProfScope() {
    if (!on) return;
    if (hipEventRecord(b, s) != hipSuccess) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.push_back({name, a, b});
  }
};

// CRT of the two prime rows in ws into ciphertext words (k_crt_enc; the
// one-lane shape writes through LDS so its stores are whole lines)
template <class Sh, class MP2 = typename Sh::MP2>
void crt_enc_launch(const xhe_key* k, int64_t n, uint32_t* ws, uint32_t* ct, hipStream_t s) {
  const int blocks = (int)((n * MP2::TPI + 255) / 256);
  if constexpr (MP2::TPI == 1)
    launch((k_crt_enc_w<MP2, 2 * Sh::K / 32>), dim3(blocks), dim3(256), s, k->kd, k->kd.p2.N, n, ws, ct);
  else
    launch(k_crt_enc<MP2>, dim3(blocks), dim3(256), s, k->kd, k->kd.p2.N, n, ws, ct);
}

template <class Sh>
void encrypt_impl(const xhe_key* k, const uint32_t* m, const uint32_t* r, int64_t count, uint32_t* ct, hipStream_t s) {
  using MP2 = typename Sh::MP2;
  int64_t chunk = std::min<int64_t>(count, kChunk);
  WsScope wsc(s);
  uint32_t* ws = wsc.get<uint32_t>((size_t)2 * 2 * MP2::S4 * chunk * sizeof(uint32_t));
  uint2* xst = nullptr;  // k_djn_pmdx workspaces (allocated on first use)
  uint32_t *xrows = nullptr, *xwords = nullptr;
  for (int64_t off = 0; off < count; off += chunk) {
    int64_t n = std::min(chunk, count - off);
    switch (paths::enc_djn(Sh::K, MP2::TPI, k->kd.pmd, k->kd.pmdx, n, pins())) {
      case paths::EncDjn::PMD:
        if constexpr (Sh::K == 2048) {
          ProfScope ps("k_djn_pmd", s);  // (the label's time includes the CRT launch)
          // small batches split each element's windows over G lanes (latency:
          // ~nwin/G + log2 G dependent products instead of nwin)
          const int G = paths::pmd_split(n, pins());
          const dim3 grid((unsigned)((n * G + 127) / 128), 2);
          auto run = [&](auto kern) {
            launch(kern, grid, dim3(128), s, k->kd, k->kd.p.N, k->kd.q.N,
                   m + (size_t)off * k->nw, r + (size_t)off * k->rand_words, k->rand_words, n, ws);
          };
          if (G == 16) run(k_djn_pmd<MP2, 37, Sh::RW, 16>);
          else if (G == 4) run(k_djn_pmd<MP2, 37, Sh::RW, 4>);
          else run(k_djn_pmd<MP2, 37, Sh::RW, 1>);
          crt_enc_launch<Sh>(k, n, ws, ct + (size_t)off * k->n2w, s);
          continue;
        } else no_path("encrypt (k_djn_pmd)");
      case paths::EncDjn::PMDX:
        if constexpr (Sh::K != 2048) {
          using D = typename Sh::PDX;
          if (!xst) {
            xst = wsc.get<uint2>((size_t)2 * D::K * chunk * sizeof(uint2));
            xrows = wsc.get<uint32_t>((size_t)2 * 2 * Sh::PDXO::MN::S4 * chunk * sizeof(uint32_t));
            xwords = wsc.get<uint32_t>((size_t)2 * chunk * Sh::RW * sizeof(uint32_t));
          }
          const dim3 g4((unsigned)((n * D::TPI + 127) / 128), 2);
          {
            ProfScope ps("k_djn_pmdx", s);
            launch((k_djn_pmdx<D, Sh::RW>), g4, dim3(128), s, k->kd, r + (size_t)off * k->rand_words, k->rand_words, n,
                   xst);
          }
          using DO = typename Sh::PDXO;  // the same state layout ([pair][count]) whatever the lanes per element
          launch((k_pmdx_enc_out<DO, Sh::RW>), dim3((unsigned)((n * DO::TPI + 127) / 128), 2), dim3(128), s, k->kd,
                 m + (size_t)off * k->nw, n, xst, xrows, xwords);
          launch(k_words_to_rows<MP2>, dim3((unsigned)((n * MP2::TPI + 255) / 256), 2), dim3(256), s, xwords, Sh::RW,
                 n, ws);
          crt_enc_launch<Sh>(k, n, ws, ct + (size_t)off * k->n2w, s);
          continue;
        } else no_path("encrypt (k_djn_pmdx)");
      case paths::EncDjn::POW_X: {
        // small batch: one 16-lane DPP row per residue (latency-bound regime)
        using MX = typename Sh::MP2X;
        launch((k_djn_pow_x<MX, MP2::S4, Sh::RW>), dim3((unsigned)((n * MX::TPI + 255) / 256), 2), dim3(256), s, k->kd,
               m + (size_t)off * k->nw, r + (size_t)off * k->rand_words, k->rand_words, n, ws);
        break;
      }
      // labelled by the kernel rocprof shows (k_djn_pow_lds / k_djn_pow)
      case paths::EncDjn::POW_LDS:
        if constexpr (MP2::TPI == 1) {  // table rows staged in LDS by LDS-DMA bursts
          ProfScope ps("k_djn_pow_lds", s);
          const dim3 grid((unsigned)((n + 127) / 128), 2);
          launch((k_djn_pow_lds<MP2, Sh::RW>), grid, dim3(128), s, k->kd, k->kd.p2.N, k->kd.q2.N,
                 m + (size_t)off * k->nw, r + (size_t)off * k->rand_words, k->rand_words, n, ws);
          break;
        } else no_path("encrypt (k_djn_pow_lds)");
      case paths::EncDjn::POW:
        if constexpr (MP2::TPI != 1) {
          ProfScope ps("k_djn_pow", s);
          const int blocks = (int)((n * MP2::TPI + 255) / 256);
          launch((k_djn_pow<MP2, Sh::RW>), dim3(blocks, 2), dim3(256), s, k->kd, k->kd.p2.N, k->kd.q2.N,
                 m + (size_t)off * k->nw, r + (size_t)off * k->rand_words, k->rand_words, n, ws);
          break;
        } else no_path("encrypt (k_djn_pow)");
      default:
        no_path("encrypt");
    }
    crt_enc_launch<Sh>(k, n, ws, ct + (size_t)off * k->n2w, s);
  }
}

// grid for per-group-workspace (grid-stride) kernels
template <class M_>
int pow_grid(int64_t count, int cap_blocks) {
  return (int)std::min<int64_t>((count * M_::TPI + 255) / 256, cap_blocks);
}

template <class Sh>
void encrypt_pub_djn_impl(const xhe_key* k, const uint32_t* m, const uint32_t* r, int64_t count, uint32_t* ct,
                          hipStream_t s) {
  if (paths::enc_pub_djn(Sh::K, k->kd.pub_nd) == paths::EncPubDjn::PUB_ND) {
    if constexpr (Sh::K == 2048) {
      // fixed-base products in Montgomery digits of n (k_djn_pub_nd), then
      // (1 + n m) folded in base n on the way out (k_ndig_out)
      using D = ND2048;
      const int64_t chunk = std::min<int64_t>(count, kChunk);
      WsScope wsc(s);
      uint2* st = wsc.get<uint2>((size_t)D::K * chunk * sizeof(uint2));
      uint32_t* rows = wsc.get<uint32_t>((size_t)2 * D::MN::S4 * chunk * sizeof(uint32_t));
      for (int64_t off = 0; off < count; off += chunk) {
        const int64_t n = std::min(chunk, count - off);
        const int eb = (int)((n * D::TPI + 127) / 128);
        {
          ProfScope ps("k_djn_pub", s);
          launch((k_djn_pub_nd<D, Sh::RW2>), dim3(eb), dim3(128), s, k->kd, r + (size_t)off * k->rand_words,
                 k->rand_words, n, st);
        }
        launch((k_ndig_out<D, true>), dim3(eb), dim3(128), s, k->kd, st, m + (size_t)off * k->nw, n,
               ct + (size_t)off * k->n2w, rows);
      }
      return;
    } else no_path("encrypt (k_djn_pub_nd)");
  }
  using MN2 = typename Sh::MN2;
  int64_t chunk = std::min<int64_t>(count, kChunk);
  WsScope wsc(s);
  uint32_t* ws = wsc.get<uint32_t>((size_t)MN2::S4 * chunk * sizeof(uint32_t));
  for (int64_t off = 0; off < count; off += chunk) {
    int64_t n = std::min(chunk, count - off);
    int blocks = (int)((n * MN2::TPI + 255) / 256);
    ProfScope ps("k_djn_pub", s);
    launch((k_djn_pub<MN2, Sh::RW2>), dim3(blocks), dim3(256), s, k->kd, k->kd.n2.N, m + (size_t)off * k->nw,
           r + (size_t)off * k->rand_words, k->rand_words, n, ws, ct + (size_t)off * k->n2w);
  }
}

// The mod-n^2 digit kernels of 2048-bit keys (k_ndig_*):
// in -> exponentiation -> out over chunks of up to kChunk elements; the
// exponentiation runs grid-stride over at most 1024 blocks (32 element groups
// each, one digit table per group slot)
template <class IN, class POW, class OUT>
void ndig_run(int64_t count, hipStream_t s, IN&& in, POW&& pw, OUT&& out) {
  using D = ND2048;
  const int64_t chunk = std::min<int64_t>(count, kChunk);
  const int pblocks = (int)std::min<int64_t>((chunk + NdigWs<D>::GPB - 1) / NdigWs<D>::GPB, 1024);
  WsScope wsc(s);
  uint2* st = wsc.get<uint2>((size_t)D::K * chunk * sizeof(uint2));
  uint2* tab = wsc.get<uint2>(NdigWs<D>::tab_bytes_per_slot() * (size_t)pblocks * NdigWs<D>::GPB);
  uint32_t* rows = wsc.get<uint32_t>((size_t)2 * D::MN::S4 * chunk * sizeof(uint32_t));
  for (int64_t off = 0; off < count; off += chunk) {
    const int64_t n = std::min(chunk, count - off);
    const int eblocks = (int)((n * D::TPI + 127) / 128);
    in(eblocks, off, n, st);
    pw(std::min<int>(pblocks, (int)((n + NdigWs<D>::GPB - 1) / NdigWs<D>::GPB)), off, n, st, tab);
    out(eblocks, off, n, st, rows);
  }
}

// Private non-DJN encryption of 2048-bit keys in Montgomery digits: r mod
// P^2 -> digits (k_dec_pmd_in), r^(e_P) by the decrypt's digit
// exponentiation (k_dec_pmd_pow, the exponent e_P = n mod phi(P^2) shared by
// every lane), (1 + n m) folded in on the way out (k_nodjn_pmd_out), CRT.
template <class Sh>
void encrypt_nodjn_pmd(const xhe_key* k, const uint32_t* m, const uint32_t* r, int64_t count, uint32_t* ct,
                       hipStream_t s) {
  using MP2 = typename Sh::MP2;
  constexpr int NQ = PMD<37>::NQ;
  const int64_t chunk = std::min<int64_t>(count, kChunk);
  const int pow_blocks = (int)std::min<int64_t>((chunk + 127) / 128, 1024);
  const int64_t lanes = (int64_t)pow_blocks * 128;
  WsScope wsc(s);
  uint4* ws = wsc.get<uint4>((size_t)2 * 16 * NQ * lanes * sizeof(uint4));
  uint4* st = wsc.get<uint4>((size_t)2 * NQ * chunk * sizeof(uint4));
  uint32_t* rows = wsc.get<uint32_t>((size_t)2 * 2 * MP2::S4 * chunk * sizeof(uint32_t));
  for (int64_t off = 0; off < count; off += chunk) {
    const int64_t n = std::min(chunk, count - off);
    const dim3 g1((unsigned)((n + 127) / 128), 2);
    launch((k_dec_pmd_in<MP2, 37>), g1, dim3(128), s, k->kd, k->kd.p.N, k->kd.q.N, k->kd.p2.N, k->kd.q2.N,
           r + (size_t)off * k->rand_words, k->rand_words, n, st);
    {
      ProfScope ps("k_nodjn_crt", s);
      launch((k_dec_pmd_pow<37>), dim3((unsigned)std::min<int64_t>((n + 127) / 128, pow_blocks), 2), dim3(128), s,
             k->kd, k->kd.p.N, k->kd.q.N, 1, n, st, ws);
    }
    launch((k_nodjn_pmd_out<MP2, 37>), g1, dim3(128), s, k->kd, k->kd.p.N, k->kd.q.N, k->kd.p2.N, k->kd.q2.N,
           m + (size_t)off * k->nw, n, st, rows);
    crt_enc_launch<Sh>(k, n, rows, ct + (size_t)off * k->n2w, s);
  }
}

template <class Sh>
void encrypt_nodjn_impl(const xhe_key* k, const uint32_t* m, const uint32_t* r, int64_t count, uint32_t* ct,
                        hipStream_t s) {
  switch (paths::enc_nodjn(Sh::K, k->priv, k->kd.ndig, count, pins())) {
    case paths::EncNoDjn::PMD:
      if constexpr (Sh::K == 2048) {
        encrypt_nodjn_pmd<Sh>(k, m, r, count, ct, s);
        return;
      } else no_path("encrypt (k_dec_pmd_pow)");
    case paths::EncNoDjn::PUB_WAVE:
      if constexpr (Sh::K == 2048) {
        // (a pinned large batch: grid.x holds it, a block per element)
        ProfScope ps("k_nodjn_pub_wave", s);
        launch((k_nodjn_pub_wave<WaveN2::K_, 16>), dim3((unsigned)count), dim3(1024), s, k->kd, m, r, k->rand_words, count, ct);
        return;
      } else no_path("encrypt (k_nodjn_pub_wave)");
    case paths::EncNoDjn::CRT: {
      using MP2 = typename Sh::MP2;
      // 2-lane batch shapes (3072 bits, 55 limbs per lane) spill in this
      // variable-base exponentiation (9.7 k enc/s): run it in the 4-lane shape.
      constexpr bool wide = MP2::TPI == 2;
      using MPE = std::conditional_t<wide, typename Sh::MP2L, MP2>;
      int64_t chunk = std::min<int64_t>(count, kChunk);
      int pb = pow_grid<MPE>(chunk, 512);
      int64_t groups = (int64_t)pb * 256 / MPE::TPI;
      WsScope wsc(s);
      uint32_t* ws = wsc.get<uint32_t>((size_t)2 * 18 * MPE::S4 * groups * sizeof(uint32_t));
      uint32_t* rows = wsc.get<uint32_t>((size_t)2 * 2 * MP2::S4 * chunk * sizeof(uint32_t));
      for (int64_t off = 0; off < count; off += chunk) {
        int64_t n = std::min(chunk, count - off);
        {
          ProfScope ps("k_nodjn_crt", s);
          const ModDev& mp = wide ? k->kd.p2L : k->kd.p2;
          const ModDev& mq = wide ? k->kd.q2L : k->kd.q2;
          launch((k_nodjn_crt<MPE, wide ? 1 : 0, MP2::S4>), dim3(pb, 2), dim3(256), s, k->kd, mp.N, mq.N,
                 m + (size_t)off * k->nw, r + (size_t)off * k->rand_words, k->rand_words, n, rows, ws);
        }
        crt_enc_launch<Sh>(k, n, rows, ct + (size_t)off * k->n2w, s);
      }
      return;
    }
    case paths::EncNoDjn::NDIG:
      if constexpr (Sh::K == 2048) {
        ndig_run(
            count, s,
            [&](int b, int64_t off, int64_t n, uint2* st) {
              launch((k_ndig_in<ND2048, false>), dim3(b), dim3(128), s, k->kd, r + (size_t)off * k->rand_words,
                     k->rand_words, n, st);
            },
            [&](int b, int64_t, int64_t n, uint2* st, uint2* tab) {
              ProfScope ps("k_nodjn_pub", s);
              launch(k_ndig_pow_n<ND2048>, dim3(b), dim3(128), s, k->kd, n, st, tab);
            },
            [&](int b, int64_t off, int64_t n, uint2* st, uint32_t* rows) {
              launch((k_ndig_out<ND2048, true>), dim3(b), dim3(128), s, k->kd, st, m + (size_t)off * k->nw, n,
                     ct + (size_t)off * k->n2w, rows);
            });
        return;
      } else no_path("encrypt (k_ndig_pow_n)");
    case paths::EncNoDjn::PUB: {
      using MN2 = typename Sh::MN2;
      int64_t chunk = std::min<int64_t>(count, kChunk);
      int pb = pow_grid<MN2>(chunk, 512);
      int64_t groups = (int64_t)pb * 256 / MN2::TPI;
      WsScope wsc(s);
      uint32_t* ws = wsc.get<uint32_t>((size_t)18 * MN2::S4 * groups * sizeof(uint32_t));
      for (int64_t off = 0; off < count; off += chunk) {
        int64_t n = std::min(chunk, count - off);
        ProfScope ps("k_nodjn_pub", s);
        launch(k_nodjn_pub<MN2>, dim3(pb), dim3(256), s, k->kd, k->kd.n2.N, m + (size_t)off * k->nw,
               r + (size_t)off * k->rand_words, k->rand_words, n, ct + (size_t)off * k->n2w, ws);
      }
      return;
    }
    default:
      no_path("encrypt");
  }
}

// n^2 constants of the MN2 shape (see n2dev in xhe_kernels.hpp).
template <class MN2>
const ModDev& n2h(const xhe_key* k) {
  if constexpr (MN2::TPI == 16) return k->kd.n2X;
  else return k->kd.n2;
}

// The n^2 ciphertext ops below run in the shape their entry point chose
// (paths::n2_shape): MN2 is Sh::MN2X for ROW16, else the batch shape.

template <class Sh, class MN2 = typename Sh::MN2>
void mulmod_impl(const xhe_key* k, const uint32_t* a, const int32_t* ea, const uint32_t* b, const int32_t* eb,
                 int64_t count, int dmax, uint32_t* out, int32_t* eout, hipStream_t s) {
  switch (paths::add(Sh::K, MN2::TPI, count, dmax, pins())) {
    case paths::Add::WAVE:
      if constexpr (Sh::K == 2048) {
        launch((k_mulmod_wave<WaveN2::K_, 16>), dim3((unsigned)count), dim3(1024), s, k->kd, a, ea, b, eb, count, out, eout);
        return;
      } else no_path("mulmod (k_mulmod_wave)");
    case paths::Add::BARRETT:
      if constexpr (Sh::K == 2048 && MN2::TPI == 4) {
        ProfScope ps("k_add_barrett", s);
        const int64_t blocks = (count + bar::EPB - 1) / bar::EPB;
        launch(k_add_barrett, dim3((unsigned)blocks), dim3(bar::TPB), s, k->kd, a, ea, b, eb, count, out, eout);
        return;
      } else no_path("mulmod (k_add_barrett)");
    case paths::Add::MONT:
      break;
    default:
      no_path("mulmod");
  }
  int64_t chunk = std::min<int64_t>(count, kChunk);
  WsScope wsc(s);
  uint32_t* ws = wsc.get<uint32_t>((size_t)2 * MN2::S4 * chunk * sizeof(uint32_t));
  for (int64_t off = 0; off < count; off += chunk) {
    int64_t n = std::min(chunk, count - off);
    int blocks = (int)((n * MN2::TPI + 255) / 256);
    launch(k_mulmod_n2<MN2>, dim3(blocks), dim3(256), s, k->kd, n2h<MN2>(k).N, a + (size_t)off * k->n2w,
           ea ? ea + off : nullptr, b + (size_t)off * k->n2w, eb ? eb + off : nullptr, n, dmax,
           out + (size_t)off * k->n2w, eout ? eout + off : nullptr, ws);
  }
}

template <class Sh, class MN2 = typename Sh::MN2>
void powmod_impl(const xhe_key* k, const uint32_t* c, const uint32_t* kw_, int kw, int kbits, int64_t count,
                 uint32_t* out, hipStream_t s) {
  if (paths::powmod(Sh::K, MN2::TPI, k->kd.ndig, pins()) == paths::Pow::NDIG) {
    if constexpr (Sh::K == 2048 && MN2::TPI == 4) {
      ndig_run(
          count, s,
          [&](int b, int64_t off, int64_t n, uint2* st) {
            launch((k_ndig_in<ND2048, true>), dim3(b), dim3(128), s, k->kd, c + (size_t)off * k->n2w, k->n2w, n, st);
          },
          [&](int b, int64_t off, int64_t n, uint2* st, uint2* tab) {
            ProfScope ps("k_powmod_n2", s);
            launch(k_ndig_pow_k<ND2048>, dim3(b), dim3(128), s, k->kd, kw_ + (size_t)off * kw, kw, kbits, n, st, tab);
          },
          [&](int b, int64_t off, int64_t n, uint2* st, uint32_t* rows) {
            launch((k_ndig_out<ND2048, false>), dim3(b), dim3(128), s, k->kd, st, nullptr, n,
                   out + (size_t)off * k->n2w, rows);
          });
      return;
    } else no_path("powmod (k_ndig_pow_k)");
  }
  int64_t chunk = std::min<int64_t>(count, kChunk);
  int pb = pow_grid<MN2>(chunk, 512);
  int64_t groups = (int64_t)pb * 256 / MN2::TPI;
  WsScope wsc(s);
  uint32_t* ws = wsc.get<uint32_t>((size_t)17 * MN2::S4 * groups * sizeof(uint32_t));
  for (int64_t off = 0; off < count; off += chunk) {
    int64_t n = std::min(chunk, count - off);
    ProfScope ps("k_powmod_n2", s);
    launch(k_powmod_n2<MN2>, dim3(pb), dim3(256), s, k->kd, n2h<MN2>(k).N, c + (size_t)off * k->n2w,
           kw_ + (size_t)off * kw, kw, kbits, n, out + (size_t)off * k->n2w, ws);
  }
}

// Ciphertext packing (xhe_pack): groups of kk ciphertexts folded by Horner.
// MONT: one launch of k_pack_n2 (no workspace). NDIG: digits of every input,
// the fold per group, digits -> words per output, over chunks of groups whose
// inputs fit kChunk elements.
template <class Sh, class MN2 = typename Sh::MN2>
void pack_impl(const xhe_key* k, paths::Pow arith, const uint32_t* c, int64_t count, int kk, int shift, uint32_t* out,
               hipStream_t s) {
  const int64_t ngroups = (count + kk - 1) / kk;
  if (arith == paths::Pow::NDIG) {
    if constexpr (Sh::K == 2048 && MN2::TPI == 4) {
      using D = ND2048;
      constexpr int GPB = NdigWs<D>::GPB;
      const int64_t gchunk = std::min<int64_t>(ngroups, std::max<int64_t>(1, kChunk / kk));
      WsScope wsc(s);
      uint2* st = wsc.get<uint2>((size_t)D::K * gchunk * kk * sizeof(uint2));
      uint2* sto = wsc.get<uint2>((size_t)D::K * gchunk * sizeof(uint2));
      uint32_t* rows = wsc.get<uint32_t>((size_t)2 * D::MN::S4 * gchunk * sizeof(uint32_t));
      for (int64_t g0 = 0; g0 < ngroups; g0 += gchunk) {
        const int64_t ng = std::min(gchunk, ngroups - g0);
        const int64_t e0 = g0 * kk, n = std::min<int64_t>(ng * kk, count - e0);
        launch((k_ndig_in<D, true>), dim3((unsigned)((n * D::TPI + 127) / 128)), dim3(128), s, k->kd,
               c + (size_t)e0 * k->n2w, k->n2w, n, st);
        {
          ProfScope ps("k_pack", s);
          launch(k_ndig_pack<D>, dim3((unsigned)std::min<int64_t>((ng + GPB - 1) / GPB, 1024)), dim3(128), s, k->kd, n,
                 kk, shift, ng, st, sto);
        }
        launch((k_ndig_out<D, false>), dim3((unsigned)((ng * D::TPI + 127) / 128)), dim3(128), s, k->kd, sto, nullptr,
               ng, out + (size_t)g0 * k->n2w, rows);
      }
      return;
    } else no_path("pack (k_ndig_pack)");
  }
  const int blocks = (int)std::min<int64_t>((ngroups * MN2::TPI + 255) / 256, 1 << 16);
  ProfScope ps("k_pack", s);
  launch(k_pack_n2<MN2>, dim3(blocks), dim3(256), s, k->kd, n2h<MN2>(k).N, c, count, kk, shift, ngroups, out);
}

// Batch inversion mod n^2 via a product tree (Montgomery's trick in parallel).
template <class Sh, class MN2 = typename Sh::MN2>
int invert_impl(const xhe_key* k, const uint32_t* c, int64_t count, uint32_t* out, hipStream_t s) {
  const int S4 = MN2::S4;
  std::vector<int64_t> sizes{count};
  while (sizes.back() > 1) sizes.push_back((sizes.back() + 1) / 2);
  std::vector<size_t> offs;
  size_t tot = 0;
  for (auto n : sizes) {
    offs.push_back(tot);
    tot += (size_t)S4 * n;
  }
  if (paths::invert(Sh::K, MN2::TPI, count) == paths::Invert::WTREE) {
  if constexpr (Sh::K == 2048 && MN2::TPI == 16) {  // (a 1024-thread block: the 16-lane 2048-bit shape's registers)
    // small batch: a product tree of whole-block products (dec_wave.hpp
    // k_wtree_*), one launch per level
    constexpr int KW = WaveN2::K_;
    std::vector<int64_t> woff;
    int64_t wtot = 0;
    for (auto n : sizes) {
      woff.push_back(wtot);
      wtot += n;
    }
    const int nlev = (int)sizes.size();
    DevBuf wds_, inv_, lv_;
    lv_ = DevBuf((size_t)wtot * KW * 4, s, DevBuf::kAsync);
    inv_ = DevBuf((size_t)wtot * KW * 4, s, DevBuf::kAsync);
    wds_ = DevBuf((size_t)2 * k->n2w * 4, s, DevBuf::kAsync);
    uint32_t *lv = lv_.as<uint32_t>(), *inv = inv_.as<uint32_t>(), *wds = wds_.as<uint32_t>();
    auto node = [&](uint32_t* b, int l) { return b + (size_t)woff[l] * KW; };
    launch((k_wtree_in<KW, 16>), dim3((unsigned)count), dim3(1024), s, k->kd, c, lv);
    for (int l = 1; l < nlev; ++l) {
      launch((k_wtree_up<KW, 16>), dim3((unsigned)sizes[l]), dim3(1024), s, k->kd, node(lv, l - 1), sizes[l - 1],
             node(lv, l));
    }
    launch((k_wtree_out<KW, 16>), dim3(1), dim3(1024), s, k->kd, node(lv, nlev - 1), wds);
    std::vector<uint32_t> root(k->n2w), yinv(k->n2w);
    HIPCHK(hipMemcpyAsync(root.data(), wds, (size_t)k->n2w * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (!modinv_words(root.data(), k->n2_host.data(), k->n2w, yinv.data()))
      return fail(XHE_ENOINV, "invert(a, b) no inverse exists");
    HIPCHK(hipMemcpyAsync(wds + k->n2w, yinv.data(), (size_t)k->n2w * 4, hipMemcpyHostToDevice, s));
    launch((k_wtree_in<KW, 16>), dim3(1), dim3(1024), s, k->kd, wds + k->n2w, node(inv, nlev - 1));
    for (int l = nlev - 2; l >= 0; --l) {
      launch((k_wtree_down<KW, 16>), dim3((unsigned)sizes[l]), dim3(1024), s, k->kd, node(inv, l + 1), node(lv, l),
             sizes[l], node(inv, l));
    }
    launch((k_wtree_out<KW, 16>), dim3((unsigned)count), dim3(1024), s, k->kd, inv, out);
    HIPCHK(hipStreamSynchronize(s));  // yinv is host memory of this frame
    return XHE_OK;
  } else no_path("invert (k_wtree_*)");
  }
  // (freed synchronously on return; st_ is read by no kernel, kept so that the call allocates as it did)
  DevBuf st_, scr_, inv_, lv_;
  lv_ = DevBuf(tot * 4, s);
  inv_ = DevBuf(tot * 4, s);
  scr_ = DevBuf((size_t)(4 * (k->n2w + 1) + 2 * k->n2w + 8) * 4, s);
  st_ = DevBuf(4, s);
  uint32_t *lv = lv_.as<uint32_t>(), *inv = inv_.as<uint32_t>(), *scr = scr_.as<uint32_t>();
  auto blocks = [&](int64_t n) { return dim3((unsigned)((n * MN2::TPI + 255) / 256)); };
  launch(k_to_mont_rows<MN2>, blocks(count), dim3(256), s, k->kd, n2h<MN2>(k).N, c, count, lv);
  for (size_t l = 1; l < sizes.size(); ++l) {
    launch(k_tree_up<MN2>, blocks(sizes[l]), dim3(256), s, k->kd, n2h<MN2>(k).N, lv + offs[l - 1], sizes[l - 1],
           lv + offs[l], sizes[l]);
  }
  size_t top = offs.back();
  uint32_t* y_words = scr + 4 * (k->n2w + 1);
  uint32_t* r_words = y_words + k->n2w;
  launch(k_row_pack<MN2>, dim3(1), dim3(64), s, k->kd, n2h<MN2>(k).N, lv + top, r_words);
  // The one scalar inverse of the batch (the tree root, (prod c_i) R) is a
  // sequential extended Euclid: ~1 ms on a host core vs a single GPU lane's
  // tens of milliseconds. Everything per element stays on the device.
  std::vector<uint32_t> root(k->n2w), yinv(k->n2w);
  HIPCHK(hipMemcpyAsync(root.data(), r_words, (size_t)k->n2w * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (!modinv_words(root.data(), k->n2_host.data(), k->n2w, yinv.data()))
    return fail(XHE_ENOINV, "invert(a, b) no inverse exists");
  HIPCHK(hipMemcpyAsync(y_words, yinv.data(), (size_t)k->n2w * 4, hipMemcpyHostToDevice, s));
  launch(k_inv_to_row<MN2>, dim3(1), dim3(64), s, k->kd, n2h<MN2>(k).N, y_words, inv + top);
  for (size_t l = sizes.size() - 1; l >= 1; --l) {
    launch(k_tree_down<MN2>, blocks(sizes[l - 1]), dim3(256), s, k->kd, n2h<MN2>(k).N, inv + offs[l], sizes[l],
           lv + offs[l - 1], sizes[l - 1], inv + offs[l - 1]);
  }
  launch(k_from_mont_rows<MN2>, blocks(count), dim3(256), s, k->kd, n2h<MN2>(k).N, inv, count, out);
  HIPCHK(hipStreamSynchronize(s));
  return XHE_OK;
}

// Small host -> device uploads made while enqueuing (the segment plans):
// copied into a pinned slot whose previous copy has completed (one event per
// slot), so the enqueue never waits for the stream. A pageable source would
// need the stream synchronised before the frame that owns it returns - which
// made every groupby sum wait for the previous call's kernels.
class HostStage {
  struct Slot {
    void* p = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    int dev = -1;
  };
  std::mutex mu_;
  std::vector<Slot> slots_;

 public:
  void upload(void* dst, const void* src, size_t n, hipStream_t s, int dev) {
    std::lock_guard<std::mutex> g(mu_);
    Slot* use = nullptr;
    for (Slot& sl : slots_)
      if (sl.dev == dev && sl.cap >= n && hipEventQuery(sl.ev) == hipSuccess) {
        use = &sl;
        break;
      }
    if (!use) {
      Slot sl;
      sl.dev = dev;
      sl.cap = std::max<size_t>(n, 64 << 10);
      HIPCHK(hipHostMalloc(&sl.p, sl.cap, hipHostMallocDefault));
      HIPCHK(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
      slots_.push_back(sl);
      use = &slots_.back();
    }
    memcpy(use->p, src, n);
    HIPCHK(hipMemcpyAsync(dst, use->p, n, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(use->ev, s));
  }
};
HostStage& host_stage() {
  static HostStage* st = new HostStage();  // process lifetime (no teardown order with the runtime)
  return *st;
}

// Reduce segment-ordered rows [S4][count] to one Montgomery row per segment
// (seg: nseg+1 offsets) by levels of k_chunk_prod (C rows per chunk). The
// input rows are Montgomery rows, or plain residues with raw = true (the
// first level then returns each chunk to Montgomery form). Returns the
// [S4][nseg] rows (`rows` itself when there is nothing to multiply); an empty
// segment yields the Montgomery one.
template <class Sh, class MN2 = typename Sh::MN2>
DevBuf reduce_segments(const xhe_key* k, DevBuf rows, int64_t count, std::vector<int64_t> seg, hipStream_t s,
                       bool raw = false, const uint32_t* words = nullptr) {
  // words: raw input as ciphertext words ([count][n2w]) instead of rows
  // (the first level unpacks them itself; rows is then unused)
  const int S4 = MN2::S4;
  const int64_t nseg = (int64_t)seg.size() - 1;
  // Lane groups the chip holds at 2 waves per SIMD: while a level has at least
  // that many chunks of kRawChunk rows it is throughput-bound and takes long
  // chunks; above that the levels are latency-bound (a chunk is a chain of
  // dependent products), and chunks of 4 give the shortest chain in all
  // (log4 levels x 4 products, against log32 levels x 32).
  constexpr int64_t kFill = 131072 / MN2::TPI;
  auto blocks = [&](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n * MN2::TPI + 255) / 256)); };
  // segments of one length (the mat-vec): the chunks are computed in the
  // kernel, no plan upload and no host sync
  bool uniform = nseg > 0;
  for (int64_t i = 1; i < nseg && uniform; ++i) uniform = seg[i + 1] - seg[i] == seg[1] - seg[0];
  uniform = uniform && seg[1] - seg[0] > 0;
  // plan every level on the host first: (first, stride, count) of every chunk
  // of every level go up in one copy, and the levels run back to back
  struct Level {
    size_t plan_off;
    int64_t n_in, n_out, seg_len, ncs;
    bool raw;
  };
  std::vector<int64_t> all;
  std::vector<Level> plan;
  int64_t n_cur = count;
  bool first = true;
  while (true) {
    bool ones = true;  // every segment is one row: nothing left to multiply
    for (int64_t i = 0; i < nseg; ++i)
      if (seg[i + 1] - seg[i] != 1) {
        ones = false;
        break;
      }
    if (ones && !(first && raw)) break;  // (plain rows still need Montgomery form)
    // the longest chunks that still leave kFill lane groups (4 .. kRawChunk):
    // a 100 k-row, 256-bin histogram took chunks of 32 on its first level (a
    // 33-product chain with a quarter of the chip busy) and now takes 4
    const int64_t C = std::max<int64_t>(4, std::min<int64_t>(kRawChunk, n_cur / kFill));
    std::vector<int64_t> nseg_b{0};
    const size_t off = all.size();
    int64_t seg_len = 0, ncs = 0;
    if (uniform) {
      seg_len = seg[1] - seg[0];
      ncs = (seg_len + C - 1) / C;
      for (int64_t i = 0; i < nseg; ++i) nseg_b.push_back(nseg_b.back() + ncs);
    } else {
      for (int64_t i = 0; i < nseg; ++i) {
        const int64_t len = seg[i + 1] - seg[i];
        const int64_t nch = std::max<int64_t>(1, (len + C - 1) / C);  // an empty segment: one (empty) chunk
        for (int64_t t = 0; t < nch; ++t) {
          all.push_back(seg[i] + t);
          all.push_back(nch);
          all.push_back(t < len ? (len - t + nch - 1) / nch : 0);
        }
        nseg_b.push_back(nseg_b.back() + nch);
      }
    }
    const int64_t n_out = nseg_b.back();
    plan.push_back({off, n_cur, n_out, seg_len, ncs, first && raw});
    n_cur = n_out;
    seg.swap(nseg_b);
    first = false;
  }
  if (plan.empty()) return rows;  // already one Montgomery row per segment
  DevBuf dplan_;
  if (!all.empty()) {
    dplan_ = DevBuf(all.size() * 8, s, DevBuf::kAsync);
    host_stage().upload(dplan_.p, all.data(), all.size() * 8, s, k->device);  // no host sync
  }
  const int64_t* dplan = dplan_.as<int64_t>();
  DevBuf cur = std::move(rows);
  for (const Level& L : plan) {
    DevBuf nxt((size_t)S4 * std::max<int64_t>(L.n_out, 1) * 4, s, DevBuf::kAsync);
    if (L.raw && words)
      launch((k_chunk_prod_words<MN2, Sh::RW2>), blocks(L.n_out), dim3(256), s, k->kd, n2h<MN2>(k).N, words,
             uniform ? nullptr : dplan + L.plan_off, L.seg_len, L.ncs, L.n_out, nxt.as<uint32_t>());
    else
      launch(k_chunk_prod<MN2>, blocks(L.n_out), dim3(256), s, k->kd, n2h<MN2>(k).N, cur.as<uint32_t>(), L.n_in,
             uniform ? nullptr : dplan + L.plan_off, L.seg_len, L.ncs, L.n_out, nxt.as<uint32_t>(), L.raw ? 1 : 0);
    cur = std::move(nxt);  // the level's input is freed here, in stream order
  }
  return cur;
}

// Segmented modular product: out[s] = prod_{i in seg s} c_i^(2^d_i) mod n^2.
// seg_begin: nseg+1 offsets into the (already segment-ordered) inputs.
template <class Sh, class MN2 = typename Sh::MN2>
void segprod_impl(const xhe_key* k, const uint32_t* c, const int32_t* d, int dmax, int64_t count,
                  const int64_t* seg_begin_host, int64_t nseg, uint32_t* out, hipStream_t s) {
  const int S4 = MN2::S4;
  auto blocks = [&](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n * MN2::TPI + 255) / 256)); };
  DevBuf rows, sq;
  // no alignment anywhere: the first level reads the ciphertext words itself
  // ($XHE_SUM_WORDS=0: the k_align_mont transpose first, A/B)
  const bool direct = paths::segprod_first(count, dmax, d != nullptr, pins()) == paths::SegFirst::WORDS;
  if (!direct) {
    rows = DevBuf((size_t)S4 * std::max<int64_t>(count, 1) * 4, s, DevBuf::kAsync);
    sq = DevBuf((size_t)S4 * std::max<int64_t>(count, 1) * 4, s, DevBuf::kAsync);
  }
  if (count > 0 && !direct) {
    launch(k_align_mont<MN2>, blocks(count), dim3(256), s, k->kd, n2h<MN2>(k).N, c, d, count, dmax,
           rows.as<uint32_t>(), sq.as<uint32_t>());
  }
  // stream-ordered frees: no host sync (the output is ready in stream order)
  const DevBuf cur = reduce_segments<Sh, MN2>(k, std::move(rows), count,
                                              std::vector<int64_t>(seg_begin_host, seg_begin_host + nseg + 1), s, true,
                                              direct ? c : nullptr);
  launch(k_from_mont_rows<MN2>, blocks(nseg), dim3(256), s, k->kd, n2h<MN2>(k).N, cur.as<uint32_t>(), nseg, out);
}

// Segmented inclusive prefix products: out[i] = prod of its segment's elements
// up to i (scan_plan.hpp). Down the levels a chunk pass each - level 0 reads
// the ciphertext words, the levels above scan the Montgomery rows of the chunk
// totals in place - then back up an apply pass each, which multiplies in the
// carries from the level above and leaves the level plain; the last one packs
// `out`. Per element one product on the chain and two off it (one in a
// segment's first chunk), plus 2 + 1/C per chunk for the levels above. Every
// level keeps its rows ([rows][S4] limbs) and a chunk index per row for the
// call; one plan upload, no host sync.
static_assert(scan::kChunkLen + 1 < kRpowRows, "a chunk's fix-up rows: R^(u+2) for u < kChunkLen");
template <class Sh, class MN2 = typename Sh::MN2>
void segscan_impl(const xhe_key* k, const uint32_t* c, int64_t count, const int64_t* seg_begin_host, int64_t nseg,
                  uint32_t* out, hipStream_t s) {
  constexpr int PW = Sh::RW2;
  const scan::Plan plan = scan::make_plan(seg_begin_host, nseg, scan::chunk_len(count));
  const size_t nl = plan.levels.size();
  auto blocks = [&](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n * MN2::TPI + 255) / 256)); };
  DevBuf dplan_(plan.chunks.size() * 8, s, DevBuf::kAsync);
  host_stage().upload(dplan_.p, plan.chunks.data(), plan.chunks.size() * 8, s, k->device);  // no host sync
  std::vector<DevBuf> rows(nl), cid(nl);
  for (size_t l = 0; l < nl; ++l) {
    rows[l] = DevBuf((size_t)MN2::S4 * plan.levels[l].rows * 4, s, DevBuf::kAsync);
    cid[l] = DevBuf((size_t)plan.levels[l].rows * 4, s, DevBuf::kAsync);
  }
  auto lplan = [&](size_t l) { return dplan_.as<int64_t>() + (size_t)plan.levels[l].chunk0 * scan::kFields; };
  auto above = [&](size_t l) { return l + 1 < nl ? rows[l + 1].as<uint32_t>() : nullptr; };
  ProfScope ps("k_segscan", s);
  for (size_t l = 0; l < nl; ++l) {
    const scan::Level& L = plan.levels[l];
    if (l == 0)
      launch((k_segscan_chunk<MN2, PW, true>), blocks(L.nchunks), dim3(256), s, k->kd, n2h<MN2>(k).N, c,
             rows[l].as<uint32_t>(), lplan(l), L.nchunks, cid[l].as<int32_t>(), above(l));
    else
      launch((k_segscan_chunk<MN2, PW, false>), blocks(L.nchunks), dim3(256), s, k->kd, n2h<MN2>(k).N, nullptr,
             rows[l].as<uint32_t>(), lplan(l), L.nchunks, cid[l].as<int32_t>(), above(l));
  }
  for (size_t l = nl; l-- > 0;) {
    const scan::Level& L = plan.levels[l];
    if (l == 0)
      launch((k_segscan_apply<MN2, PW, true>), blocks(L.rows), dim3(256), s, k->kd, n2h<MN2>(k).N, out,
             rows[l].as<uint32_t>(), L.rows, lplan(l), cid[l].as<int32_t>(), above(l));
    else
      launch((k_segscan_apply<MN2, PW, false>), blocks(L.rows), dim3(256), s, k->kd, n2h<MN2>(k).N, nullptr,
             rows[l].as<uint32_t>(), L.rows, lplan(l), cid[l].as<int32_t>(), above(l));
  }
}

// Window bits for a multi-exponentiation: minimise table products
// nbases*(2^c - 2) plus gathered products ncols*nterms*ceil(kbits/c), with the
// tables capped at ~2 GiB.
int mexp_window(int64_t nbases, int64_t ncols, int64_t nterms, int kbits, int s4) {
  int best = 1;
  double best_cost = 1e300;
  for (int c = 1; c <= 8; ++c) {
    if (c > 1 && (double)(nbases << c) * s4 * 4 > 2147483648.0) break;
    double cost = (double)nbases * ((1 << c) - 2) + (double)ncols * nterms * ((kbits + c - 1) / c) +
                  (double)ncols * kbits;
    if (cost < best_cost) {
      best_cost = cost;
      best = c;
    }
  }
  return best;
}

// Multi-exponentiation out[j] = prod_t bases[idx[j][t]]^k[j][t] mod n^2.
template <class Sh, class MN2 = typename Sh::MN2>
void multiexp_impl(const xhe_key* k, const uint32_t* bases, int64_t nbases, const int32_t* idx, const uint32_t* kx,
                   int kw, int kbits, int64_t ncols, int64_t nterms, int c, uint32_t* out, hipStream_t s) {
  const int S4 = MN2::S4;
  auto blocks = [&](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n * MN2::TPI + 255) / 256)); };
  const int nwin = std::max(1, (kbits + c - 1) / c);
  // every buffer here: stream-ordered frees, no host sync
  DevBuf sq, prod, tab;
  tab = DevBuf(((size_t)nbases << c) * S4 * 4, s, DevBuf::kAsync);
  {
    ProfScope ps("k_mexp_tab", s);
    // by levels of entries (c + 1 dependent products per base); one launch
    // per level
    for (int lvl = 1; lvl <= c; ++lvl) {
      const int64_t per = lvl <= 1 ? 1 : lvl < c ? ((int64_t)1 << (lvl - 1)) : ((int64_t)1 << (lvl - 1)) - 1;
      launch(k_mexp_tab_lvl<MN2>, blocks(nbases * per), dim3(256), s, k->kd, n2h<MN2>(k).N, bases, nbases, c, lvl,
             tab.as<uint32_t>());
    }
  }
  // enough lane groups to fill the chip, at least 2 terms per group
  const int64_t segs = ncols * nwin;
  const int64_t target_groups = 131072 / MN2::TPI;
  const int64_t chunk = std::max<int64_t>(2, std::min<int64_t>(64, (segs * nterms + target_groups - 1) / target_groups));
  const int64_t nchunks = (nterms + chunk - 1) / chunk;
  const int64_t n_out = segs * nchunks;
  DevBuf rows((size_t)S4 * n_out * 4, s, DevBuf::kAsync);
  {
    ProfScope ps("k_mexp_gather", s);
    launch(k_mexp_gather<MN2>, blocks(n_out), dim3(256), s, k->kd, n2h<MN2>(k).N, tab.as<uint32_t>(), c, idx, kx, kw,
           nterms, nwin, nchunks, chunk, n_out, rows.as<uint32_t>());
  }
  std::vector<int64_t> seg(segs + 1);
  for (int64_t i = 0; i <= segs; ++i) seg[i] = i * nchunks;
  prod = reduce_segments<Sh, MN2>(k, std::move(rows), n_out, std::move(seg), s);
  const uint32_t* P = prod.as<uint32_t>();
  sq = DevBuf((size_t)S4 * ncols * 4, s, DevBuf::kAsync);
  {
    ProfScope ps("k_mexp_horner", s);
    switch (paths::mexp_horner(Sh::K, MN2::TPI, ncols, pins())) {
      case paths::Horner::WAVE:
        // small batches: one 16-wave block per column (latency; k_mexp_horner_wave)
        if constexpr (Sh::K == 2048 && MN2::TPI == 16) {
          launch((k_mexp_horner_wave<WaveN2::K_, 16>), dim3((unsigned)ncols), dim3(1024), s, k->kd, P, nwin, c, ncols, out);
          break;
        } else no_path("multiexp (k_mexp_horner_wave)");
      case paths::Horner::LANES:
        launch(k_mexp_horner<MN2>, blocks(ncols), dim3(256), s, k->kd, n2h<MN2>(k).N, P, nwin, c, ncols,
               sq.as<uint32_t>(), out);
        break;
      default:
        no_path("multiexp");
    }
  }
}

template <class Sh>
void raw_encrypt_impl(const xhe_key* k, const uint32_t* m, int64_t count, uint32_t* ct, hipStream_t s) {
  using MP2 = typename Sh::MP2;
  int64_t chunk = std::min<int64_t>(count, kChunk);
  WsScope wsc(s);
  uint32_t* ws = wsc.get<uint32_t>((size_t)2 * MP2::S4 * chunk * sizeof(uint32_t));
  for (int64_t off = 0; off < count; off += chunk) {
    int64_t n = std::min(chunk, count - off);
    int blocks = (int)((n * MP2::TPI + 255) / 256);
    launch(k_raw_enc<MP2>, dim3(blocks), dim3(256), s, k->kd, m + (size_t)off * k->nw, n, ws,
           ct + (size_t)off * k->n2w);
  }
}

// The decrypt exponentiation in the lane shape paths::decrypt chose (SHAPE 2:
// MP2X, one 16-lane row per residue; 1: MP2L, 4 lanes; 0: the batch shape).
template <class MP2S, int SHAPE, class MP2>
void dec_pow_launch(const xhe_key* k, const uint32_t* ct, int64_t n, int64_t chunk, uint32_t* xrows,
                    hipStream_t s) {
  int pow_blocks = (int)std::min<int64_t>((chunk * MP2S::TPI + 255) / 256, 512);
  int64_t groups = (int64_t)pow_blocks * 256 / MP2S::TPI;
  WsScope wsc(s);
  uint32_t* ws = wsc.get<uint32_t>((size_t)2 * 17 * MP2S::S4 * groups * sizeof(uint32_t));
  const ModDev& mp = SHAPE == 2 ? k->kd.p2X : SHAPE == 1 ? k->kd.p2L : k->kd.p2;
  const ModDev& mq = SHAPE == 2 ? k->kd.q2X : SHAPE == 1 ? k->kd.q2L : k->kd.q2;
  {
    ProfScope ps("k_dec_pow", s);
    launch((k_dec_pow<MP2S, SHAPE>), dim3(pow_blocks, 2), dim3(256), s, k->kd, mp.N, mq.N, ct, n, (int)MP2::S4, xrows,
           ws);
  }
}

// one lane per residue, exponentiation in Montgomery digits (2048-bit keys)
template <class MP2>
void dec_pmd_launch(const xhe_key* k, const uint32_t* ct, int64_t n, int64_t chunk, uint32_t* xrows, hipStream_t s) {
  constexpr int NQ = PMD<37>::NQ;
  const int pow_blocks = (int)std::min<int64_t>((chunk + 127) / 128, 1024);
  const int64_t lanes = (int64_t)pow_blocks * 128;
  WsScope wsc(s);
  uint4* ws = wsc.get<uint4>((size_t)2 * 16 * NQ * lanes * sizeof(uint4));
  uint4* st = wsc.get<uint4>((size_t)2 * NQ * chunk * sizeof(uint4));
  const dim3 g1((unsigned)((n + 127) / 128), 2);
  launch((k_dec_pmd_in<MP2, 37>), g1, dim3(128), s, k->kd, k->kd.p.N, k->kd.q.N, k->kd.p2.N, k->kd.q2.N, ct, k->n2w, n,
         st);
  {
    ProfScope ps("k_dec_pow", s);
    launch((k_dec_pmd_pow<37>), dim3(pow_blocks, 2), dim3(128), s, k->kd, k->kd.p.N, k->kd.q.N, 0, n, st, ws);
  }
  launch((k_dec_pmd_out<MP2, 37>), g1, dim3(128), s, k->kd, k->kd.p.N, k->kd.q.N, k->kd.p2.N, k->kd.q2.N, n, st,
         (int)MP2::S4, xrows);
}

// 3072/4096-bit decrypt in Montgomery digits up to m_P (k_dec_pmdx_*, see
// xhe_kernels.hpp): writes mrows [prime][2 S4][count] as k_dec_fin does
template <class Sh>
void dec_pmdx_launch(const xhe_key* k, const uint32_t* ct, int64_t n, int64_t chunk, uint32_t* mrows,
                     hipStream_t s) {
  using DO = typename Sh::PDXO;  // conversions (register room)
  using DP = typename Sh::PDXP;  // the exponentiation
  using MP2L = typename Sh::MP2L;
  using MP = typename Sh::MP;
  constexpr int RW = Sh::RW, NWH = Sh::K / 64;
  constexpr int SCR = MP2L::S4 > DO::MN::S4 ? MP2L::S4 : DO::MN::S4;
  constexpr int GPB = 128 / DP::TPI;
  const int pow_blocks = (int)std::min<int64_t>((chunk + GPB - 1) / GPB, 1024);
  const int64_t gs = (int64_t)pow_blocks * GPB;
  WsScope wsc(s);
  uint32_t* words = wsc.get<uint32_t>((size_t)2 * chunk * RW * sizeof(uint32_t));
  uint32_t* scr = wsc.get<uint32_t>((size_t)2 * SCR * chunk * sizeof(uint32_t));
  uint2* st = wsc.get<uint2>((size_t)2 * DP::K * chunk * sizeof(uint2));
  uint2* tab = wsc.get<uint2>((size_t)2 * 16 * DP::K * gs * sizeof(uint2));
  launch((k_p2_reduce_words<MP2L, RW>), dim3((unsigned)((n * MP2L::TPI + 255) / 256), 2), dim3(256), s, k->kd, ct, n,
         scr, words);
  const dim3 go((unsigned)((n * DO::TPI + 127) / 128), 2);
  launch((k_dec_pmdx_in<DO, RW>), go, dim3(128), s, k->kd, words, n, st);
  {
    ProfScope ps("k_dec_pow", s);
    const int pb = (int)std::min<int64_t>((n + GPB - 1) / GPB, pow_blocks);
    launch(k_dec_pmdx_pow<DP>, dim3(pb, 2), dim3(128), s, k->kd, n, st, tab);
  }
  launch((k_dec_pmdx_out<DO, NWH>), go, dim3(128), s, k->kd, n, st, scr, words);
  launch(k_words_to_rows<MP>, dim3((unsigned)((n * MP::TPI + 255) / 256), 2), dim3(256), s, words, NWH, n, mrows);
}

template <class Sh>
void decrypt_impl(const xhe_key* k, const uint32_t* ct, int64_t count, uint32_t* m, hipStream_t s) {
  using MP2 = typename Sh::MP2;
  using MP = typename Sh::MP;
  const paths::Dec path = paths::decrypt(Sh::K, MP2::TPI, k->kd.pmdx_dec, k->kd.rns, count, pins());
  int64_t chunk = std::min<int64_t>(count, kChunk);
  WsScope wsc(s);
  uint32_t* xrows = wsc.get<uint32_t>((size_t)2 * MP2::S4 * chunk * sizeof(uint32_t));
  uint32_t* mrows = wsc.get<uint32_t>((size_t)2 * 2 * MP::S4 * chunk * sizeof(uint32_t));
  for (int64_t off = 0; off < count; off += chunk) {
    int64_t n = std::min(chunk, count - off);
    const uint32_t* cto = ct + (size_t)off * k->n2w;
    const int blocks = (int)((n * MP::TPI + 255) / 256);
    // the exponentiation into xrows (PMDX goes on to m_P itself: it writes mrows)
    switch (path) {
      case paths::Dec::PMDX:
        if constexpr (Sh::K != 2048) {
          dec_pmdx_launch<Sh>(k, cto, n, chunk, mrows, s);
          launch(k_crt_dec<MP>, dim3(blocks), dim3(256), s, k->kd, k->kd.p.N, n, mrows, m + (size_t)off * k->nw);
          continue;
        } else no_path("decrypt (k_dec_pmdx_pow)");
      case paths::Dec::RNS:
        if constexpr (Sh::K == 2048) {
          static_assert(MP2::S == 74 && MP2::W == 28, "k_dec_wave / k_dec_rns share the MP2 limbs");
          ProfScope ps("k_dec_rns", s);
          launch(k_dec_rns, dim3((unsigned)n, 2), dim3(rns::NT), s, k->kd, cto, n, (int)MP2::S4, xrows);
        } else no_path("decrypt (k_dec_rns)");
        break;
      case paths::Dec::WAVE:
        if constexpr (Sh::K == 2048) {
          ProfScope ps("k_dec_wave", s);
          launch((k_dec_wave<74, XHE_DEC_NWV>), dim3((unsigned)n, 2), dim3(64 * XHE_DEC_NWV), s, k->kd, cto, n,
                 (int)MP2::S4, xrows);
        } else no_path("decrypt (k_dec_wave)");
        break;
      case paths::Dec::ROW16:
        dec_pow_launch<typename Sh::MP2X, 2, MP2>(k, cto, n, chunk, xrows, s);
        break;
      case paths::Dec::QUAD4:
        dec_pow_launch<typename Sh::MP2L, 1, MP2>(k, cto, n, chunk, xrows, s);
        break;
      case paths::Dec::PMD1:
        if constexpr (Sh::K == 2048) dec_pmd_launch<MP2>(k, cto, n, chunk, xrows, s);
        else no_path("decrypt (k_dec_pmd_pow)");
        break;
      case paths::Dec::POW1:
        if constexpr (Sh::K != 2048) dec_pow_launch<MP2, 0, MP2>(k, cto, n, chunk, xrows, s);
        else no_path("decrypt (k_dec_pow, batch shape)");
        break;
      default:
        no_path("decrypt");
    }
    launch((k_dec_fin<MP2, MP>), dim3(blocks, 2), dim3(256), s, k->kd, k->kd.p.N, k->kd.q.N, n, xrows, mrows);
    launch(k_crt_dec<MP>, dim3(blocks), dim3(256), s, k->kd, k->kd.p.N, n, mrows, m + (size_t)off * k->nw);
  }
}

template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const HipError& e) {
    return fail(XHE_EHIP, e.what());
  } catch (const std::exception& e) {
    return fail(XHE_EINVAL, e.what());
  }
}

}  // namespace

int xhe_segprod(const xhe_key* key, const uint32_t* c_dev, const int32_t* d_dev, int dmax, int64_t count,
                const int64_t* seg_begin, int64_t nseg, uint32_t* out_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key || !seg_begin || nseg <= 0 || (count > 0 && !c_dev) || !out_dev || dmax < 0)
      return fail(XHE_EINVAL, "xhe_segprod: bad argument");
    if (seg_begin[0] != 0 || seg_begin[nseg] != count) return fail(XHE_EINVAL, "xhe_segprod: bad segment offsets");
    for (int64_t i = 0; i < nseg; ++i)
      if (seg_begin[i + 1] < seg_begin[i]) return fail(XHE_EINVAL, "xhe_segprod: offsets must be non-decreasing");
    DevGuard dg(key->device);
    const bool row = paths::n2_shape(count, pins()) == paths::N2Shape::ROW16;
    hipStream_t hs = (hipStream_t)stream;
    with_shape(key->K, [&](auto sh) {
      using Sh = decltype(sh);
      if (row) segprod_impl<Sh, typename Sh::MN2X>(key, c_dev, d_dev, dmax, count, seg_begin, nseg, out_dev, hs);
      else segprod_impl<Sh>(key, c_dev, d_dev, dmax, count, seg_begin, nseg, out_dev, hs);
    });
    return XHE_OK;
  });
}

namespace {
int segscan_args(const xhe_key* key, const uint32_t* c, int64_t count, const int64_t* seg_begin, int64_t nseg,
                 const uint32_t* out, const char* who) {
  if (!key || !seg_begin || nseg <= 0 || count < 0 || (count > 0 && (!c || !out)))
    return fail(XHE_EINVAL, std::string(who) + ": bad argument");
  if (seg_begin[0] != 0 || seg_begin[nseg] != count) return fail(XHE_EINVAL, std::string(who) + ": bad segment offsets");
  for (int64_t i = 0; i < nseg; ++i)
    if (seg_begin[i + 1] < seg_begin[i]) return fail(XHE_EINVAL, std::string(who) + ": offsets must be non-decreasing");
  if (count > 0 && out < c + (size_t)count * key->n2w && c < out + (size_t)count * key->n2w)
    return fail(XHE_EINVAL, std::string(who) + ": out overlaps c");
  return XHE_OK;
}
}  // namespace

int xhe_segscan(const xhe_key* key, const uint32_t* c_dev, int64_t count, const int64_t* seg_begin, int64_t nseg,
                uint32_t* out_dev, void* stream) {
  return guarded([&]() -> int {
    if (int rc = segscan_args(key, c_dev, count, seg_begin, nseg, out_dev, "xhe_segscan")) return rc;
    if (count == 0) return XHE_OK;
    DevGuard dg(key->device);
    const bool row = paths::n2_shape(count, pins()) == paths::N2Shape::ROW16;
    hipStream_t hs = (hipStream_t)stream;
    with_shape(key->K, [&](auto sh) {
      using Sh = decltype(sh);
      if (row) segscan_impl<Sh, typename Sh::MN2X>(key, c_dev, count, seg_begin, nseg, out_dev, hs);
      else segscan_impl<Sh>(key, c_dev, count, seg_begin, nseg, out_dev, hs);
    });
    return XHE_OK;
  });
}

namespace {
struct Stream {
  hipStream_t s = nullptr;
  Stream() { HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  ~Stream() {
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
  }
};

// After a ciphertext add whose alignment gap reaches key->dneg: the
// reference's _decrease_exponent_to raises the operand of larger exponent to
// the scalar 1 << d through _raw_mul, whose negative branch (1 << d >=
// min_value_for_negative) gives c^(2^d - n) where the add kernel computed
// c^(2^d) (paillier.py:79-86, 173-187). out *= x^-n with x = that operand on
// those elements and 1 elsewhere: x^n by the per-element power, one batch
// inversion, one product. Only reached when dmax >= dneg (gaps of ~bitlen(n)
// exponent steps: precision=None values around 1e+-300).
template <class Sh, class MN2>
int mulmod_gap_fix(const xhe_key* k, const uint32_t* a, const int32_t* ea, const uint32_t* b, const int32_t* eb,
                   int64_t count, uint32_t* out, hipStream_t s) {
  const size_t cb = (size_t)k->n2w * 4;
  DevBuf x(count * cb, s), kx((size_t)count * k->nw * 4, s), z(count * cb, s), zi(count * cb, s), t(count * cb, s);
  launch(k_gap_pick, dim3((unsigned)((count + 255) / 256)), dim3(256), s, k->kd, a, ea, b, eb, count, k->dneg,
         x.as<uint32_t>(), kx.as<uint32_t>());
  powmod_impl<Sh, MN2>(k, x.as<uint32_t>(), kx.as<uint32_t>(), k->nw, k->n_bits, count, z.as<uint32_t>(), s);
  const int rc = invert_impl<Sh, MN2>(k, z.as<uint32_t>(), count, zi.as<uint32_t>(), s);
  if (rc != XHE_OK) return rc;
  mulmod_impl<Sh, MN2>(k, out, nullptr, zi.as<uint32_t>(), nullptr, count, 0, t.as<uint32_t>(), nullptr, s);
  HIPCHK(hipMemcpyAsync(out, t.p, count * cb, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipStreamSynchronize(s));  // the DevBufs are freed on return
  return XHE_OK;
}

// The stream-ordered allocator (hipMallocAsync, the entry points'
// workspaces) returns freed memory to the device at each synchronisation by
// default (release threshold 0), so every synchronised call would map its
// workspaces afresh. Keep up to kPoolKeep bytes cached in the device's
// default pool instead (set once per device, at key creation) - small next to
// the tables, so HBM stays available to the caller (torch's allocator does not
// draw from this pool).
#ifndef XHE_POOL_KEEP_MB
#define XHE_POOL_KEEP_MB 2048
#endif
constexpr uint64_t kPoolKeep = (uint64_t)XHE_POOL_KEEP_MB << 20;
void keep_pool_memory(int device) {
  static std::mutex mu;
  static bool done[64] = {};
  std::lock_guard<std::mutex> g(mu);
  if (device < 0 || device >= 64 || done[device] || kPoolKeep == 0) return;
  hipMemPool_t pool;
  if (hipDeviceGetDefaultMemPool(&pool, device) == hipSuccess) {
    uint64_t keep = kPoolKeep;
    (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
  }
  done[device] = true;
}

// Pinned staging ring for the host-buffer entry points. A copy between the
// device and pageable memory goes through the runtime's small bounce buffers
// (~10 GB/s) and holds the calling thread; from or into pinned memory it is
// one DMA at the link rate and asynchronous. One ring per device is kept for
// the process lifetime and grown on demand; a call that finds it in use by
// another thread gets a ring of its own. Slot b holds one chunk's parts
// (inputs and outputs) at fixed offsets.
class PinnedSlots {
 public:
  PinnedSlots(int device, int depth, const std::vector<size_t>& part_bytes) {
    size_t off = 0;
    for (size_t b : part_bytes) {
      off_.push_back(off);
      off += (b + 255) & ~(size_t)255;
    }
    slot_ = off;
    const size_t need = std::max<size_t>(slot_ * depth, 256);
    Ring& r = ring(device);
    lock_ = std::unique_lock<std::mutex>(r.mu, std::try_to_lock);
    if (lock_.owns_lock()) {
      if (r.bytes < need) {
        if (r.p) HIPCHK(hipHostFree(r.p));
        r.p = nullptr;
        r.bytes = 0;
        HIPCHK(hipHostMalloc((void**)&r.p, need, hipHostMallocDefault));
        r.bytes = need;
      }
      base_ = r.p;
    } else {
      HIPCHK(hipHostMalloc((void**)&own_, need, hipHostMallocDefault));
      base_ = own_;
    }
  }
  ~PinnedSlots() {
    if (own_) (void)hipHostFree(own_);
  }
  PinnedSlots(const PinnedSlots&) = delete;
  PinnedSlots& operator=(const PinnedSlots&) = delete;
  uint8_t* at(int b, int k) const { return base_ + (size_t)b * slot_ + off_[k]; }

 private:
  struct Ring {
    std::mutex mu;
    uint8_t* p = nullptr;
    size_t bytes = 0;
  };
  static Ring& ring(int device) {
    static Ring rings[64];
    return rings[device & 63];
  }
  std::vector<size_t> off_;
  size_t slot_ = 0;
  std::unique_lock<std::mutex> lock_;
  uint8_t* base_ = nullptr;
  uint8_t* own_ = nullptr;
};

// A per-element host buffer of an element-chunked host call: elem_bytes per
// element; host == nullptr marks an absent optional argument.
struct HostPart {
  const void* host;
  size_t elem_bytes;
};

// Elements per chunk of the host-buffer pipelines for the encryption kernels
// ($XHE_HOST_CHUNK overrides, for A/B runs).
int64_t host_chunk(int64_t dflt) {
  static const int64_t v = env_str("XHE_HOST_CHUNK") ? std::max<int64_t>(1024, env_int("XHE_HOST_CHUNK", 0)) : 0;
  return v ? v : dflt;
}

// RAII hipEvent without timing (ordering only)
struct Event {
  hipEvent_t e = nullptr;
  Event() { HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
  ~Event() { (void)hipEventDestroy(e); }
};

// Element-chunked host-buffer call. Chunk c uses slot b = c % depth and
// stream b: host threads copy its inputs into pinned slot b (xhe_host_copy),
// the upload, run(b, off, n, din, dout, stream)'s kernels and the download
// into the slot follow in stream order, and once the download has landed host
// threads copy the results into the caller's buffers. Chunk c + depth - 1 is
// staged and enqueued before chunk c is drained, so the host copies and both
// DMA directions overlap the kernels. The kernels of chunk c wait for those of
// chunk c - 1 (an event): kernels of different chunks do not share the CUs (a
// big kernel next to a small one on another stream stretches the small one
// from microseconds to milliseconds and stalls the chain behind it), while
// each copy stays in its own stream behind its own kernels, where the runtime
// gives it to a DMA engine (a cross-stream wait in front of a copy made the
// runtime run it as a blit kernel on the CUs instead). Batches whose chunk
// moves < 1 MiB copy straight from and to the caller's memory.
template <class Run>
int host_pipeline(const xhe_key* key, int64_t count, int64_t chunk, const std::vector<HostPart>& in,
                  const std::vector<HostPart>& out, Run&& run) {
  if (count <= 0) return XHE_OK;
  static const bool trace = env_str("XHE_HOST_TRACE") != nullptr;  // per-chunk timings to stderr
  // Kernels of consecutive chunks run one after another ($XHE_HOST_OVERLAP
  // lets them overlap instead: then the three streams' chunks advance in
  // lockstep - each one's small kernels wait for CU slots behind the others'
  // big ones - and the copy-out comes in bursts; 17.6-18.8 vs 19.5-20.4 M/s).
  static const bool serial = env_str("XHE_HOST_OVERLAP") == nullptr;
  chunk = std::max<int64_t>(1, std::min(chunk, count));
  const int64_t nch = (count + chunk - 1) / chunk;
  const int D = (int)std::min<int64_t>(nch, 3);
  const int ni = (int)in.size(), no = (int)out.size();
  std::vector<size_t> parts;
  size_t per_chunk = 0;
  for (auto& h : in) parts.push_back(h.elem_bytes * chunk), per_chunk += h.elem_bytes * chunk;
  for (auto& h : out) parts.push_back(h.elem_bytes * chunk), per_chunk += h.elem_bytes * chunk;
  const bool staged = per_chunk >= ((size_t)1 << 20);
  // only as many streams/events as slots: a one-chunk call (small batches:
  // the LR operators' per-batch calls) pays for one stream, as a plain call
  std::vector<std::unique_ptr<Stream>> st_;
  std::vector<std::unique_ptr<Event>> ev_;
  for (int b = 0; b < D; ++b) {
    st_.emplace_back(new Stream());
    ev_.emplace_back(new Event());
  }
  auto st = [&](int b) -> Stream& { return *st_[b]; };
  auto ev_k = [&](int b) -> Event& { return *ev_[b]; };
  WsCache wsc[3];  // destroyed before the streams (frees are stream-ordered)
  for (int b = 0; b < D; ++b) wsc[b].s = st(b).s;
  std::vector<std::unique_ptr<DevBuf>> dev;  // [slot][part]
  for (int b = 0; b < D; ++b)
    for (size_t k = 0; k < parts.size(); ++k) dev.emplace_back(new DevBuf(parts[k], st(b).s));
  std::unique_ptr<PinnedSlots> pin;
  if (staged) pin.reset(new PinnedSlots(key->device, D, parts));
  // Declared after `pin`, so destroyed before it: on every exit (a non-OK rc,
  // a HIPCHK throw) the slot streams drain before the pinned ring goes back to
  // the device's pool, where another caller may take it while this call's
  // copies are still landing in it.
  struct Drain {
    std::vector<std::unique_ptr<Stream>>& s;
    ~Drain() {
      for (auto& x : s) (void)hipStreamSynchronize(x->s);
    }
  } drain{st_};
  // test hook: run() of this chunk fails (error-path tests). Armed only when
  // XHE_TEST_HOOKS=1 is set as well, so a stray variable cannot fail a call.
  static const int64_t fail_chunk = [] {
    const char* on = env_str("XHE_TEST_HOOKS");
    return (on && on[0] == '1') ? env_int("XHE_TEST_FAIL_CHUNK", -1) : (int64_t)-1;
  }();
  auto dptr = [&](int b, int k) { return dev[(size_t)b * parts.size() + k]->p; };
  auto enqueue = [&](int64_t c) -> int {
    const int b = (int)(c % D);
    static std::atomic<bool> fired{false};  // the hook fails one call per process
    if (c == fail_chunk && !fired.exchange(true))
      return fail(XHE_EINVAL, "host pipeline: injected failure (XHE_TEST_FAIL_CHUNK)");
    const int64_t off = c * chunk, n = std::min(chunk, count - off);
    hipStream_t s = st(b).s;
    const auto tin = std::chrono::steady_clock::now();
    std::vector<void*> din(ni), dout(no);
    for (int k = 0; k < ni; ++k) {
      din[k] = in[k].host ? dptr(b, k) : nullptr;
      if (!in[k].host) continue;
      const uint8_t* src = static_cast<const uint8_t*>(in[k].host) + (size_t)off * in[k].elem_bytes;
      const size_t nb = (size_t)n * in[k].elem_bytes;
      if (staged) {
        xhe_host_copy(pin->at(b, k), src, (int64_t)nb);
        src = pin->at(b, k);
      }
      HIPCHK(hipMemcpyAsync(din[k], src, nb, hipMemcpyHostToDevice, s));
    }
    if (trace)
      fprintf(stderr, "[host_pipeline] chunk %lld: staged inputs %.3f ms\n", (long long)c,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tin).count());
    if (serial && c > 0) HIPCHK(hipStreamWaitEvent(s, ev_k((int)((c - 1) % D)).e, 0));
    for (int k = 0; k < no; ++k) dout[k] = out[k].host ? dptr(b, ni + k) : nullptr;
    const auto tr = std::chrono::steady_clock::now();
    for (auto& w : wsc[b].blk) w.used = false;
    t_ws = &wsc[b];
    int rc;
    try {
      rc = run(b, off, n, din.data(), dout.data(), s);
    } catch (...) {
      t_ws = nullptr;
      throw;
    }
    t_ws = nullptr;
    if (rc != XHE_OK) return rc;
    HIPCHK(hipEventRecord(ev_k(b).e, s));
    const auto td = std::chrono::steady_clock::now();
    for (int k = 0; k < no; ++k)
      if (out[k].host) {
        void* dst = staged ? (void*)pin->at(b, ni + k)
                           : (void*)(static_cast<uint8_t*>(const_cast<void*>(out[k].host)) + (size_t)off * out[k].elem_bytes);
        HIPCHK(hipMemcpyAsync(dst, dout[k], (size_t)n * out[k].elem_bytes, hipMemcpyDeviceToHost, s));
      }
    if (trace)
      fprintf(stderr, "[host_pipeline] chunk %lld: run %.3f ms, d2h enqueue %.3f ms\n", (long long)c,
              std::chrono::duration<double, std::milli>(td - tr).count(),
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - td).count());
    return XHE_OK;
  };
  int rc = XHE_OK;
  for (int64_t c = 0; c + 1 < D; ++c)
    if ((rc = enqueue(c)) != XHE_OK) return rc;
  for (int64_t c = 0; c < nch; ++c) {
    // slot (c - 1) % D was drained last iteration (its stream has finished)
    if (c + D - 1 < nch && (rc = enqueue(c + D - 1)) != XHE_OK) return rc;
    const int b = (int)(c % D);
    const int64_t off = c * chunk, n = std::min(chunk, count - off);
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipStreamSynchronize(st(b).s));
    const auto t1 = std::chrono::steady_clock::now();
    if (staged)
      for (int k = 0; k < no; ++k)
        if (out[k].host)
          xhe_host_copy(static_cast<uint8_t*>(const_cast<void*>(out[k].host)) + (size_t)off * out[k].elem_bytes,
                        pin->at(b, ni + k), (int64_t)((size_t)n * out[k].elem_bytes));
    if (trace) {
      const auto t2 = std::chrono::steady_clock::now();
      fprintf(stderr, "[host_pipeline] chunk %lld: wait %.3f ms, copy-out %.3f ms\n", (long long)c,
              std::chrono::duration<double, std::milli>(t1 - t0).count(),
              std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
  }
  return XHE_OK;
}
}  // namespace

namespace {
// Draws for elements [base, base + count) of the stream (seed32, nonce).
void rand_impl(const xhe_key* key, const uint8_t* seed32, uint64_t nonce, int64_t base, int64_t count,
               uint32_t* rand_dev, int32_t* status_dev, hipStream_t s) {
  ChaChaKey ck;
  memcpy(ck.k, seed32, 32);
  ck.nonce0 = (uint32_t)nonce;
  ck.nonce1 = (uint32_t)(nonce >> 32);
  if (key->djn) {
    // no rejection: one thread per ChaCha20 block, the element's lanes adjacent
    int tpe = 1;
    while (tpe < (key->rand_words + 15) / 16) tpe <<= 1;
    int blocks = (int)((count * tpe + 255) / 256);
    launch(k_rand_djn, dim3(blocks), dim3(256), s, ck, base, count, key->rand_words, key->rand_bits, tpe, rand_dev,
           status_dev);
  } else {
    int blocks = (int)((count + 255) / 256);
    launch(k_rand_below, dim3(blocks), dim3(256), s, ck, base, count, key->rand_words, key->rand_bits, key->kd.n_words,
           rand_dev, status_dev);
  }
}
}  // namespace

// row gather (SCATTER = false: dst[i] = src[idx[i]]) or scatter (dst[idx[i]] =
// src[i]), one word per thread, grid-stride (xhe_gather_rows / xhe_scatter_rows)
template <bool SCATTER>
__global__ void k_move_rows(const uint32_t* __restrict__ src, const int64_t* __restrict__ idx, int64_t count,
                            int words, uint32_t* __restrict__ dst) {
  const int64_t tot = count * words;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < tot; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / words, w = t - i * words;
    if (SCATTER) dst[idx[i] * words + w] = src[t];
    else dst[t] = src[idx[i] * words + w];
  }
}

// rows[i] = the len[i] little-endian bytes at bytes[off[i] ..] of a received
// payload, zero-extended to n2w words (xhe_wire_unpack; the receiving side of
// Paillier.ciphertext_from, paillier.py:260-271). Flat over the count * n2w/4
// quads, grid-stride: consecutive lanes store consecutive 16 B of one row
// (n2w = 192 too, which no power-of-two lane group per row would serve) and
// read consecutive, overlapping dwords of one value. The per-quad work, with
// its clamps against hostile off / len, is wireu::unpack_quad.
__global__ void k_wire_unpack(const uint8_t* __restrict__ bytes, int64_t nbytes, const uint32_t* __restrict__ off,
                              const uint16_t* __restrict__ len, int64_t count, int n2w, uint32_t* __restrict__ rows) {
  const int qpr = n2w >> 2;
  const int64_t tot = count * qpr;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < tot; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / qpr;
    const int q = (int)(t - i * qpr);
    uint32_t w[4];
    xhe::wireu::unpack_quad(bytes, nbytes, off[i], len[i], n2w, q, w);
    reinterpret_cast<uint4*>(rows)[t] = make_uint4(w[0], w[1], w[2], w[3]);  // t < count * n2w/4: inside the rows
  }
}

// bit length of each row's value (little-endian words, row-major): what the
// wire layout of Paillier.serialize needs per element (its LONG1/LONG4 byte
// count, paillier.py:244-258), so the host can size the payload before the
// ciphertext words come down
__global__ void k_row_bits(const uint32_t* __restrict__ w, int64_t count, int n2w, int16_t* __restrict__ bits) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t* r = w + (size_t)i * n2w;
  int k = n2w - 1;
  while (k >= 0 && r[k] == 0u) --k;
  bits[i] = (int16_t)(k < 0 ? 0 : 32 * k + 32 - __clz((int)r[k]));
}

extern "C" {

#if XHE_RNS_PROBE
// (probe builds only) k_dec_rns's cycle probe of its last launch: 16 values
int xhe_rns_probe_read(unsigned long long* out) {
  return guarded([&]() -> int {
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rns_probe), 16 * sizeof(unsigned long long), 0,
                               hipMemcpyDeviceToHost));
    return XHE_OK;
  });
}
#endif

int xhe_rns_constants(const uint32_t* p_words, int pw, uint32_t* shared_out, uint32_t* prime_out) {
  return guarded([&]() -> int {
    if (!p_words || pw <= 0 || !shared_out || !prime_out) return fail(XHE_EINVAL, "xhe_rns_constants: bad argument");
    const BigU P = BigU::from_words(p_words, (size_t)pw);
    if (P.bits() > 1024 || P.bits() < 2) return fail(XHE_EINVAL, "xhe_rns_constants: P must have 2..1024 bits");
    const std::vector<uint32_t>& sh = rnsh::bases().shared;
    std::copy(sh.begin(), sh.end(), shared_out);
    const std::vector<uint32_t> pb = rnsh::prime_block(P);
    std::copy(pb.begin(), pb.end(), prime_out);
    return XHE_OK;
  });
}

int xhe_row_bits(const uint32_t* words_dev, int64_t count, int n2w, int16_t* bits_dev, void* stream) {
  return guarded([&]() -> int {
    if (count < 0 || n2w <= 0 || n2w > 1023) return fail(XHE_EINVAL, "xhe_row_bits: bad size");
    if (count == 0) return XHE_OK;
    if (!words_dev || !bits_dev) return fail(XHE_EINVAL, "xhe_row_bits: null argument");
    launch(k_row_bits, dim3((unsigned)((count + 255) / 256)), dim3(256), (hipStream_t)stream, words_dev, count, n2w,
           bits_dev);
    return XHE_OK;
  });
}

int xhe_key_create(int device, int key_bits, const uint32_t* n_words, const uint32_t* p_words,
                   const uint32_t* q_words, const uint32_t* h_pow_n_words, int win_bits, xhe_key** out) {
  return guarded([&]() -> int {
    if (!out || !n_words) return fail(XHE_EINVAL, "xhe_key_create: null argument");
    *out = nullptr;
    if (!key_bits_supported(key_bits))
      return fail(XHE_ENOTSUP, "xhe_key_create: key_bits must be 2048, 3072, 4096 or 8192");
    if ((p_words == nullptr) != (q_words == nullptr)) return fail(XHE_EINVAL, "xhe_key_create: need both p and q");
    if (win_bits == 0) {
      const char* ev = env_str("XHE_WIN_BITS");  // "23" or "23s" (split layout), as _native.parse_win
      win_bits = ev ? atoi(ev) : 16;
      if (ev && win_bits > 0 && ev[strlen(ev) - 1] == 's') win_bits |= XHE_WIN_SPLIT;
    }
    const int wbase = win_bits & ~XHE_WIN_SPLIT;
    if (wbase < 2 || wbase > ((win_bits & XHE_WIN_SPLIT) ? 23 : 24))
      return fail(XHE_EINVAL, "xhe_key_create: win_bits must be in [2, 24] (split: [2, 23])");
    std::unique_ptr<xhe_key> k(new xhe_key());
    k->device = device;
    k->K = key_bits;
    k->nw = key_bits / 32;
    k->n2w = 2 * k->nw;
    k->priv = p_words != nullptr;
    k->djn = h_pow_n_words != nullptr;
    BigU n = BigU::from_words(n_words, k->nw);
    if ((int)n.bits() > key_bits || n.bits() + 2 < (size_t)key_bits)
      return fail(XHE_EINVAL, "xhe_key_create: n does not match key_bits");
    k->n_host.assign(n_words, n_words + k->nw);
    k->n2_host.assign(k->n2w, 0u);
    mul(n, n).to_words(k->n2_host.data(), k->n2w);
    k->n_bits = (int)n.bits();
    {
      BigU third, rem;
      divmod(n, BigU(3), &third, &rem);
      k->dneg = (int)sub(sub(n, third), BigU(1)).bits();  // 2^d >= t  <=>  d >= bitlen(t - 1)
    }
    BigU p, q, h;
    if (k->priv) {
      p = BigU::from_words(p_words, k->nw / 2);
      q = BigU::from_words(q_words, k->nw / 2);
      if (cmp(mul(p, q), n) != 0) return fail(XHE_EINVAL, "xhe_key_create: n != p*q");
      if (p.bits() * 2 > (size_t)key_bits + 0 || q.bits() * 2 > (size_t)key_bits)
        return fail(XHE_ENOTSUP, "xhe_key_create: p and q must each have key_bits/2 bits");
      if ((p.w[0] & 1) == 0 || (q.w[0] & 1) == 0) return fail(XHE_EINVAL, "xhe_key_create: p, q must be odd");
    }
    if (k->djn) h = BigU::from_words(h_pow_n_words, k->n2w);
    DevGuard dg(device);
    keep_pool_memory(device);
    key_create_impl(k.get(), n, k->priv ? &p : nullptr, k->priv ? &q : nullptr, k->djn ? &h : nullptr, win_bits);
    *out = k.release();
    return XHE_OK;
  });
}

void xhe_key_destroy(xhe_key* key) {
  if (!key) return;
  int prev = -1;
  if (hipGetDevice(&prev) == hipSuccess && prev != key->device) (void)hipSetDevice(key->device);
  if (key->d_blob) (void)hipFree(key->d_blob);
  if (key->d_tab) (void)hipFree(key->d_tab);
  if (prev >= 0 && prev != key->device) (void)hipSetDevice(prev);
  delete key;
}

int xhe_key_info(const xhe_key* key, int* key_bits, int* nw, int* n2w, int* rand_words, int* rand_bits, int* flags) {
  if (!key) return fail(XHE_EINVAL, "xhe_key_info: null key");
  if (key_bits) *key_bits = key->K;
  if (nw) *nw = key->nw;
  if (n2w) *n2w = key->n2w;
  if (rand_words) *rand_words = key->rand_words;
  if (rand_bits) *rand_bits = key->rand_bits;
  if (flags) *flags = (key->priv ? 1 : 0) | (key->djn ? 2 : 0);
  return XHE_OK;
}

int xhe_encode_f64(const xhe_key* key, const double* x_dev, int64_t count, int precision, int has_max,
                   int max_exponent, uint32_t* m_dev, int32_t* exp_dev, int32_t* status_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!x_dev || !m_dev || !exp_dev || !status_dev)))
      return fail(XHE_EINVAL, "xhe_encode_f64: null argument");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    int mode = precision < 0 ? 0 : 1;
    // -ceil(log2(10) * precision) (encoder.py:39), computed exactly as Python does in float64
    int e0 = precision < 0 ? 0 : -(int)std::ceil(std::log2(10.0) * (double)precision);
    int blocks = (int)((count * (key->nw / 4) + 255) / 256);  // one thread per 16-byte quad of m
    launch(k_encode_f64, dim3(blocks), dim3(256), (hipStream_t)stream, x_dev, count, mode, e0, has_max, max_exponent,
           key->kd.n_words, key->nw, m_dev, exp_dev, status_dev);
    return XHE_OK;
  });
}

int xhe_rand(const xhe_key* key, const uint8_t* seed32, uint64_t nonce, int64_t count, uint32_t* rand_dev,
             int32_t* status_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key || !seed32 || (count > 0 && !rand_dev)) return fail(XHE_EINVAL, "xhe_rand: null argument");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    rand_impl(key, seed32, nonce, 0, count, rand_dev, status_dev, (hipStream_t)stream);
    return XHE_OK;
  });
}

int xhe_encrypt(const xhe_key* key, const uint32_t* m_dev, const uint32_t* rand_dev, int64_t count, uint32_t* ct_dev,
                void* stream) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!m_dev || !ct_dev))) return fail(XHE_EINVAL, "xhe_encrypt: null argument");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    hipStream_t s = (hipStream_t)stream;
    if (!rand_dev) {
      with_shape(key->K, [&](auto sh) { raw_encrypt_impl<decltype(sh)>(key, m_dev, count, ct_dev, s); });
      return XHE_OK;
    }
    if (key->djn && key->priv) {
      with_shape(key->K, [&](auto sh) { encrypt_impl<decltype(sh)>(key, m_dev, rand_dev, count, ct_dev, s); });
    } else if (key->djn) {
      with_shape(key->K, [&](auto sh) { encrypt_pub_djn_impl<decltype(sh)>(key, m_dev, rand_dev, count, ct_dev, s); });
    } else {
      with_shape(key->K, [&](auto sh) { encrypt_nodjn_impl<decltype(sh)>(key, m_dev, rand_dev, count, ct_dev, s); });
    }
    return XHE_OK;
  });
}

// Obfuscators ahead of time: xhe_encrypt's own dispatch on zero plaintexts
// (1 + n 0 = 1, so the result is the factor itself). The zeros are one
// workspace of at most kObfFillZeroBytes, reused pass by pass: 1 M elements a
// pass at 2048 bits, the encryption's own launch chunk (with 64 MiB, four
// launches of 256 k, a 1 M fill ran 10 % below the direct rate). A pass is at
// least 65,536 elements, above every batch-size threshold of the encryption
// shapes, so a large fill runs the kernels a large encryption runs.
constexpr size_t kObfFillZeroBytes = (size_t)256 << 20;
int xhe_obf_fill(const xhe_key* key, const uint32_t* rand_dev, int64_t count, uint32_t* obf_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key || count < 0 || (count > 0 && (!rand_dev || !obf_dev)))
      return fail(XHE_EINVAL, "xhe_obf_fill: null argument or negative count");
    if (count == 0) return XHE_OK;
    DevGuard dg(key->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t row = (size_t)key->nw * sizeof(uint32_t);
    const int64_t pass = std::min<int64_t>(count, std::max<int64_t>(65536, (int64_t)(kObfFillZeroBytes / row)));
    WsScope wsc(s);
    uint32_t* zero = wsc.get<uint32_t>((size_t)pass * row);
    HIPCHK(hipMemsetAsync(zero, 0, (size_t)pass * row, s));
    for (int64_t off = 0; off < count; off += pass) {
      const int64_t n = std::min(pass, count - off);
      const int rc = xhe_encrypt(key, zero, rand_dev + (size_t)off * key->rand_words, n,
                                 obf_dev + (size_t)off * key->n2w, stream);
      if (rc != XHE_OK) return rc;
    }
    return XHE_OK;
  });
}

int xhe_encrypt_obf(const xhe_key* key, const uint32_t* m_dev, uint32_t* obf_dev, int64_t count, int wipe,
                    uint32_t* ct_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!m_dev || !obf_dev || !ct_dev)))
      return fail(XHE_EINVAL, "xhe_encrypt_obf: null argument");
    if (count < 0) return fail(XHE_EINVAL, "xhe_encrypt_obf: negative count");
    if (count == 0) return XHE_OK;
    const size_t words = (size_t)count * key->n2w;
    if (ct_dev < obf_dev + words && obf_dev < ct_dev + words)
      return fail(XHE_EINVAL, "xhe_encrypt_obf: ct overlaps the obfuscators");
    DevGuard dg(key->device);
    hipStream_t s = (hipStream_t)stream;
    with_shape(key->K, [&](auto sh) {
      using M = typename decltype(sh)::MP2L;
      // one launch: no workspace bounds the batch (a 256-thread block holds 256 / TPI elements)
      const int64_t blocks = (count * M::TPI + 255) / 256;
      if (blocks > 0x7fffffff) throw std::invalid_argument("xhe_encrypt_obf: count too large for one launch");
      ProfScope ps("k_enc_obf", s);
      launch(k_enc_obf<M>, dim3((unsigned)blocks), dim3(256), s, key->kd, m_dev, obf_dev, count, wipe, ct_dev);
    });
    return XHE_OK;
  });
}

int xhe_decrypt(const xhe_key* key, const uint32_t* ct_dev, int64_t count, uint32_t* m_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!ct_dev || !m_dev))) return fail(XHE_EINVAL, "xhe_decrypt: null argument");
    if (!key->priv) return fail(XHE_EINVAL, "Try to decrypt a paillier ciphertext by a public key.");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    with_shape(key->K, [&](auto sh) { decrypt_impl<decltype(sh)>(key, ct_dev, count, m_dev, (hipStream_t)stream); });
    return XHE_OK;
  });
}

int xhe_decode(const xhe_key* key, const uint32_t* m_dev, const int32_t* exp_dev, int64_t count, double* f64_dev,
               float* f32_dev, int32_t* status_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!m_dev || !exp_dev || !f64_dev || !f32_dev || !status_dev)))
      return fail(XHE_EINVAL, "xhe_decode: null argument");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    int blocks = (int)((count + 255) / 256);
    launch(k_decode, dim3(blocks), dim3(256), (hipStream_t)stream, m_dev, exp_dev, count, key->kd, f64_dev, f32_dev,
           status_dev);
    return XHE_OK;
  });
}

}  // extern "C"

namespace {
// The packing geometry the kernels handle: whole-word slots of 64..256 bits,
// a precision that keeps every digit / 2^precision a normal double, and all
// the slots below n's top bit (|x| < 2^(slots * bits - 1) < n / 2).
bool pack_geometry_ok(const xhe_key* key, int slots, int interval_bits, int precision) {
  return interval_bits >= 64 && interval_bits <= 256 && interval_bits % 32 == 0 && precision >= 0 &&
         precision <= interval_bits - 2 && slots >= 1 && (int64_t)slots * interval_bits <= key->n_bits - 1;
}

void embed_launch(const xhe_key* key, const double* cols_dev, int64_t cstride, int ncols, int64_t count,
                  int interval_bits, int precision, uint32_t* m_dev, int32_t* status_dev, hipStream_t s) {
  int blocks = (int)((count * (key->nw / 4) + 255) / 256);  // one thread per 16-byte quad of m
  launch(k_embed_f64, dim3(blocks), dim3(256), s, cols_dev, cstride, ncols, count, interval_bits, precision,
         key->kd.n_words, key->nw, m_dev, status_dev);
}

void umbed_launch(const xhe_key* key, const uint32_t* m_dev, int64_t count, int num, int interval_bits, int precision,
                  double* f64_dev, float* f32_dev, int64_t ostride, int32_t* status_dev, hipStream_t s) {
  int blocks = (int)((count + 255) / 256);
  launch(k_umbed, dim3(blocks), dim3(256), s, m_dev, count, num, interval_bits, precision, key->kd, f64_dev, f32_dev,
         ostride, status_dev);
}
}  // namespace

extern "C" {

int xhe_embed_f64(const xhe_key* key, const double* cols_dev, int ncols, int64_t count, int interval_bits,
                  int precision, uint32_t* m_dev, int32_t* status_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!cols_dev || !m_dev || !status_dev)))
      return fail(XHE_EINVAL, "xhe_embed_f64: null argument");
    if (!pack_geometry_ok(key, ncols, interval_bits, precision))
      return fail(XHE_EINVAL, "xhe_embed_f64: unsupported packing geometry");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    embed_launch(key, cols_dev, count, ncols, count, interval_bits, precision, m_dev, status_dev, (hipStream_t)stream);
    return XHE_OK;
  });
}

int xhe_umbed(const xhe_key* key, const uint32_t* m_dev, int64_t count, int num, int interval_bits, int precision,
              double* f64_dev, float* f32_dev, int32_t* status_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!m_dev || !f64_dev || !f32_dev || !status_dev)))
      return fail(XHE_EINVAL, "xhe_umbed: null argument");
    if (!pack_geometry_ok(key, num, interval_bits, precision))
      return fail(XHE_EINVAL, "xhe_umbed: unsupported packing geometry");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    umbed_launch(key, m_dev, count, num, interval_bits, precision, f64_dev, f32_dev, count, status_dev,
                 (hipStream_t)stream);
    return XHE_OK;
  });
}

// The packed host calls go chunk by chunk on one stream (columns are
// contiguous per column, not per element, so they do not fit host_pipeline's
// per-element parts): the columns of a chunk sit side by side in one device
// buffer whose column stride is the chunk size.
int xhe_embed_f64_host(const xhe_key* key, const double* cols, int ncols, int64_t count, int interval_bits,
                       int precision, uint32_t* m, int32_t* status) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!cols || !m || !status))) return fail(XHE_EINVAL, "xhe_embed_f64_host: null argument");
    if (!pack_geometry_ok(key, ncols, interval_bits, precision))
      return fail(XHE_EINVAL, "xhe_embed_f64_host: unsupported packing geometry");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    Stream st;
    const int64_t chunk = std::min<int64_t>(host_chunk(1 << 18), count);
    const size_t mb = (size_t)key->nw * 4;
    DevBuf dc((size_t)ncols * chunk * 8, st.s), dm((size_t)chunk * mb, st.s), ds((size_t)chunk * 4, st.s);
    for (int64_t off = 0; off < count; off += chunk) {
      const int64_t n = std::min(chunk, count - off);
      for (int j = 0; j < ncols; ++j)
        HIPCHK(hipMemcpyAsync(dc.as<double>() + (size_t)j * chunk, cols + (size_t)j * count + off, (size_t)n * 8,
                              hipMemcpyHostToDevice, st.s));
      embed_launch(key, dc.as<double>(), chunk, ncols, n, interval_bits, precision, dm.as<uint32_t>(),
                   ds.as<int32_t>(), st.s);
      HIPCHK(hipMemcpyAsync(m + (size_t)off * key->nw, dm.p, (size_t)n * mb, hipMemcpyDeviceToHost, st.s));
      HIPCHK(hipMemcpyAsync(status + off, ds.p, (size_t)n * 4, hipMemcpyDeviceToHost, st.s));
      HIPCHK(hipStreamSynchronize(st.s));
    }
    return XHE_OK;
  });
}

int xhe_decrypt_umbed_host(const xhe_key* key, const uint32_t* ct, int64_t count, int num, int interval_bits,
                           int precision, double* f64, float* f32, int32_t* status) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!ct || !f64 || !f32 || !status)))
      return fail(XHE_EINVAL, "xhe_decrypt_umbed_host: null argument");
    if (!key->priv) return fail(XHE_EINVAL, "Try to decrypt a paillier ciphertext by a public key.");
    if (!pack_geometry_ok(key, num, interval_bits, precision))
      return fail(XHE_EINVAL, "xhe_decrypt_umbed_host: unsupported packing geometry");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    Stream st;
    const int64_t chunk = std::min<int64_t>(host_chunk(1 << 17), count);
    const size_t cb = (size_t)key->n2w * 4;
    DevBuf dct((size_t)chunk * cb, st.s), dm((size_t)chunk * key->nw * 4, st.s), d64((size_t)num * chunk * 8, st.s),
        d32((size_t)num * chunk * 4, st.s), ds((size_t)chunk * 4, st.s);
    for (int64_t off = 0; off < count; off += chunk) {
      const int64_t n = std::min(chunk, count - off);
      HIPCHK(hipMemcpyAsync(dct.p, ct + (size_t)off * key->n2w, (size_t)n * cb, hipMemcpyHostToDevice, st.s));
      int rc = xhe_decrypt(key, dct.as<uint32_t>(), n, dm.as<uint32_t>(), st.s);
      if (rc != XHE_OK) return rc;
      umbed_launch(key, dm.as<uint32_t>(), n, num, interval_bits, precision, d64.as<double>(), d32.as<float>(), chunk,
                   ds.as<int32_t>(), st.s);
      for (int j = 0; j < num; ++j) {
        HIPCHK(hipMemcpyAsync(f64 + (size_t)j * count + off, d64.as<double>() + (size_t)j * chunk, (size_t)n * 8,
                              hipMemcpyDeviceToHost, st.s));
        HIPCHK(hipMemcpyAsync(f32 + (size_t)j * count + off, d32.as<float>() + (size_t)j * chunk, (size_t)n * 4,
                              hipMemcpyDeviceToHost, st.s));
      }
      HIPCHK(hipMemcpyAsync(status + off, ds.p, (size_t)n * 4, hipMemcpyDeviceToHost, st.s));
      HIPCHK(hipStreamSynchronize(st.s));
    }
    return XHE_OK;
  });
}

int xhe_encrypt_host(const xhe_key* key, const uint32_t* m, const uint32_t* rand, int64_t count, uint32_t* ct) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!m || !ct))) return fail(XHE_EINVAL, "xhe_encrypt_host: null argument");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    return host_pipeline(key, count, 1 << 17, {{m, (size_t)key->nw * 4}, {rand, (size_t)key->rand_words * 4}},
                         {{ct, (size_t)key->n2w * 4}},
                         [&](int, int64_t, int64_t n, void* const* din, void* const* dout, hipStream_t s) -> int {
                           return xhe_encrypt(key, (const uint32_t*)din[0], (const uint32_t*)din[1], n,
                                              (uint32_t*)dout[0], s);
                         });
  });
}

int xhe_decrypt_host(const xhe_key* key, const uint32_t* ct, int64_t count, uint32_t* m) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!ct || !m))) return fail(XHE_EINVAL, "xhe_decrypt_host: null argument");
    if (!key->priv) return fail(XHE_EINVAL, "Try to decrypt a paillier ciphertext by a public key.");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    return host_pipeline(key, count, 1 << 17, {{ct, (size_t)key->n2w * 4}}, {{m, (size_t)key->nw * 4}},
                         [&](int, int64_t, int64_t n, void* const* din, void* const* dout, hipStream_t s) -> int {
                           return xhe_decrypt(key, (const uint32_t*)din[0], n, (uint32_t*)dout[0], s);
                         });
  });
}

int xhe_mulmod(const xhe_key* key, const uint32_t* a_dev, const int32_t* ea_dev, const uint32_t* b_dev,
               const int32_t* eb_dev, int64_t count, int dmax, uint32_t* out_dev, int32_t* eout_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!a_dev || !b_dev || !out_dev)) || dmax < 0)
      return fail(XHE_EINVAL, "xhe_mulmod: bad argument");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    const bool row = paths::n2_shape(count, pins()) == paths::N2Shape::ROW16;
    hipStream_t hs = (hipStream_t)stream;
    return with_shape(key->K, [&](auto sh) -> int {
      using Sh = decltype(sh);
      if (row) mulmod_impl<Sh, typename Sh::MN2X>(key, a_dev, ea_dev, b_dev, eb_dev, count, dmax, out_dev, eout_dev, hs);
      else mulmod_impl<Sh>(key, a_dev, ea_dev, b_dev, eb_dev, count, dmax, out_dev, eout_dev, hs);
      // a NULL exponent array means all exponents 0 (include/xhe.h), so one
      // array alone can still carry a gap >= dneg
      if ((ea_dev || eb_dev) && dmax >= key->dneg)
        return row ? mulmod_gap_fix<Sh, typename Sh::MN2X>(key, a_dev, ea_dev, b_dev, eb_dev, count, out_dev, hs)
                   : mulmod_gap_fix<Sh, typename Sh::MN2>(key, a_dev, ea_dev, b_dev, eb_dev, count, out_dev, hs);
      return XHE_OK;
    });
  });
}

int xhe_powmod(const xhe_key* key, const uint32_t* c_dev, const uint32_t* k_dev, int kw, int kbits, int64_t count,
               uint32_t* out_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!c_dev || !k_dev || !out_dev)) || kw <= 0 || kbits < 0 || kbits > 32 * kw)
      return fail(XHE_EINVAL, "xhe_powmod: bad argument");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    const bool row = paths::n2_shape(count, pins()) == paths::N2Shape::ROW16;
    hipStream_t hs = (hipStream_t)stream;
    with_shape(key->K, [&](auto sh) {
      using Sh = decltype(sh);
      if (row) powmod_impl<Sh, typename Sh::MN2X>(key, c_dev, k_dev, kw, kbits, count, out_dev, hs);
      else powmod_impl<Sh>(key, c_dev, k_dev, kw, kbits, count, out_dev, hs);
    });
    return XHE_OK;
  });
}

namespace {
// k >= 1, shift_bits >= 1 and k * shift_bits <= bitlen(n) - 2: the packed
// plaintext keeps the sign bit xhe_umbed reads
int pack_args(const xhe_key* key, const void* c, int64_t count, int k, int shift_bits, const void* out,
              const char* who) {
  if (!key || count < 0 || (count > 0 && (!c || !out))) return fail(XHE_EINVAL, std::string(who) + ": bad argument");
  if (k < 1 || shift_bits < 1 || (int64_t)k * shift_bits > key->n_bits - 2)
    return fail(XHE_EINVAL, std::string(who) + ": k >= 1, shift_bits >= 1 and k * shift_bits <= bitlen(n) - 2 required");
  return XHE_OK;
}
}  // namespace

int xhe_pack(const xhe_key* key, const uint32_t* c_dev, int64_t count, int k, int shift_bits, uint32_t* out_dev,
             void* stream) {
  return guarded([&]() -> int {
    if (int rc = pack_args(key, c_dev, count, k, shift_bits, out_dev, "xhe_pack")) return rc;
    if (count == 0) return XHE_OK;
    const int64_t ngroups = (count + k - 1) / k;
    if (out_dev < c_dev + (size_t)count * key->n2w && c_dev < out_dev + (size_t)ngroups * key->n2w)
      return fail(XHE_EINVAL, "xhe_pack: out overlaps c");
    DevGuard dg(key->device);
    hipStream_t hs = (hipStream_t)stream;
    with_shape(key->K, [&](auto sh) {
      using Sh = decltype(sh);
      const paths::Pack plan = paths::pack(Sh::K, Sh::MN2::TPI, key->kd.ndig, ngroups, pins());
      if (plan.shape == paths::N2Shape::ROW16)
        pack_impl<Sh, typename Sh::MN2X>(key, plan.arith, c_dev, count, k, shift_bits, out_dev, hs);
      else pack_impl<Sh>(key, plan.arith, c_dev, count, k, shift_bits, out_dev, hs);
    });
    return XHE_OK;
  });
}

int xhe_pack_host(const xhe_key* key, const uint32_t* c, int64_t count, int k, int shift_bits, uint32_t* out) {
  return guarded([&]() -> int {
    if (int rc = pack_args(key, c, count, k, shift_bits, out, "xhe_pack_host")) return rc;
    if (count == 0) return XHE_OK;
    DevGuard dg(key->device);
    const int64_t ngroups = (count + k - 1) / k;
    const size_t cb = (size_t)key->n2w * 4;
    Stream st;
    DevBuf dc((size_t)count * cb, st.s), dout((size_t)ngroups * cb, st.s);
    HIPCHK(hipMemcpyAsync(dc.p, c, (size_t)count * cb, hipMemcpyHostToDevice, st.s));
    int rc = xhe_pack(key, dc.as<uint32_t>(), count, k, shift_bits, dout.as<uint32_t>(), st.s);
    if (rc != XHE_OK) return rc;
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)ngroups * cb, hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipStreamSynchronize(st.s));
    return XHE_OK;
  });
}

int xhe_invert(const xhe_key* key, const uint32_t* c_dev, int64_t count, uint32_t* out_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!c_dev || !out_dev))) return fail(XHE_EINVAL, "xhe_invert: null argument");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    const bool row = paths::n2_shape(count, pins()) == paths::N2Shape::ROW16;
    hipStream_t hs = (hipStream_t)stream;
    return with_shape(key->K, [&](auto sh) -> int {
      using Sh = decltype(sh);
      return row ? invert_impl<Sh, typename Sh::MN2X>(key, c_dev, count, out_dev, hs)
                 : invert_impl<Sh>(key, c_dev, count, out_dev, hs);
    });
  });
}


int xhe_encrypt_f64_host(const xhe_key* key, const double* x, int64_t count, int precision, int has_max,
                         int max_exponent, int obfuscate, const uint8_t* seed32, uint64_t nonce, uint32_t* ct,
                         int32_t* exps, int32_t* status) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!x || !ct || !exps || !status)) || (obfuscate && !seed32))
      return fail(XHE_EINVAL, "xhe_encrypt_f64_host: null argument");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    // chunks of 256 k elements through host_pipeline (with the kernels of
    // consecutive chunks serialised, a chunk's last partial round of waves is
    // idle time: 128 k chunks ran 21.8 M/s device-resident, 256 k 25.8 M/s,
    // tools/chunk_rate.py); the randomness is drawn at global element
    // positions, so the ciphertexts do not depend on the chunking
    const int64_t chunk = host_chunk(1 << 18), cmax = std::min<int64_t>(chunk, count);
    std::unique_ptr<DevBuf> dm[3], dr[3];
    return host_pipeline(
        key, count, chunk, {{x, 8}}, {{ct, (size_t)key->n2w * 4}, {exps, 4}, {status, 4}},
        [&](int b, int64_t off, int64_t n, void* const* din, void* const* dout, hipStream_t s) -> int {
          if (!dm[b]) {
            dm[b].reset(new DevBuf((size_t)cmax * key->nw * 4, s));
            dr[b].reset(new DevBuf(obfuscate ? (size_t)cmax * key->rand_words * 4 : 4, s));
          }
          int rc = xhe_encode_f64(key, (const double*)din[0], n, precision, has_max, max_exponent,
                                  dm[b]->as<uint32_t>(), (int32_t*)dout[1], (int32_t*)dout[2], s);
          if (rc != XHE_OK) return rc;
          if (obfuscate) rand_impl(key, seed32, nonce, off, n, dr[b]->as<uint32_t>(), nullptr, s);
          return xhe_encrypt(key, dm[b]->as<uint32_t>(), obfuscate ? dr[b]->as<uint32_t>() : nullptr, n,
                             (uint32_t*)dout[0], s);
        });
  });
}

int xhe_encrypt_words_host(const xhe_key* key, const uint32_t* m, int64_t count, int obfuscate,
                           const uint8_t* seed32, uint64_t nonce, uint32_t* ct) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!m || !ct)) || (obfuscate && !seed32))
      return fail(XHE_EINVAL, "xhe_encrypt_words_host: null argument");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    const int64_t chunk = host_chunk(1 << 18), cmax = std::min<int64_t>(chunk, count);
    std::unique_ptr<DevBuf> dr[3];
    return host_pipeline(
        key, count, chunk, {{m, (size_t)key->nw * 4}}, {{ct, (size_t)key->n2w * 4}},
        [&](int b, int64_t off, int64_t n, void* const* din, void* const* dout, hipStream_t s) -> int {
          if (obfuscate) {
            if (!dr[b]) dr[b].reset(new DevBuf((size_t)cmax * key->rand_words * 4, s));
            rand_impl(key, seed32, nonce, off, n, dr[b]->as<uint32_t>(), nullptr, s);
          }
          return xhe_encrypt(key, (const uint32_t*)din[0], obfuscate ? dr[b]->as<uint32_t>() : nullptr, n,
                             (uint32_t*)dout[0], s);
        });
  });
}

int xhe_decrypt_decode_host(const xhe_key* key, const uint32_t* ct, const int32_t* exps, int64_t count, double* f64,
                            float* f32, int32_t* status, uint32_t* m_out) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!ct || !exps || !f64 || !f32 || !status)))
      return fail(XHE_EINVAL, "xhe_decrypt_decode_host: null argument");
    if (!key->priv) return fail(XHE_EINVAL, "Try to decrypt a paillier ciphertext by a public key.");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    const int64_t chunk = host_chunk(1 << 17), cmax = std::min<int64_t>(chunk, count);
    std::unique_ptr<DevBuf> dm[3];
    return host_pipeline(
        key, count, chunk, {{ct, (size_t)key->n2w * 4}, {exps, 4}},
        {{f64, 8}, {f32, 4}, {status, 4}, {m_out, (size_t)key->nw * 4}},
        [&](int b, int64_t, int64_t n, void* const* din, void* const* dout, hipStream_t s) -> int {
          uint32_t* m = (uint32_t*)dout[3];
          if (!m) {
            if (!dm[b]) dm[b].reset(new DevBuf((size_t)cmax * key->nw * 4, s));
            m = dm[b]->as<uint32_t>();
          }
          int rc = xhe_decrypt(key, (const uint32_t*)din[0], n, m, s);
          if (rc != XHE_OK) return rc;
          return xhe_decode(key, m, (const int32_t*)din[1], n, (double*)dout[0], (float*)dout[1],
                            (int32_t*)dout[2], s);
        });
  });
}

int xhe_mulmod_host(const xhe_key* key, const uint32_t* a, const int32_t* ea, const uint32_t* b, const int32_t* eb,
                    int64_t count, int dmax, uint32_t* out, int32_t* eout) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!a || !b || !out))) return fail(XHE_EINVAL, "xhe_mulmod_host: null argument");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    const size_t cb = (size_t)key->n2w * 4;
    return host_pipeline(
        key, count, 1 << 16, {{a, cb}, {ea, 4}, {b, cb}, {eb, 4}}, {{out, cb}, {eout, 4}},
        [&](int, int64_t, int64_t n, void* const* din, void* const* dout, hipStream_t s) -> int {
          return xhe_mulmod(key, (const uint32_t*)din[0], (const int32_t*)din[1], (const uint32_t*)din[2],
                            (const int32_t*)din[3], n, dmax, (uint32_t*)dout[0], (int32_t*)dout[1], s);
        });
  });
}

int xhe_powmod_host(const xhe_key* key, const uint32_t* c, const uint32_t* k, int kw, int kbits, int64_t count,
                    int invert_first, uint32_t* out) {
  return guarded([&]() -> int {
    if (!key || (count > 0 && (!c || !k || !out))) return fail(XHE_EINVAL, "xhe_powmod_host: null argument");
    if (count <= 0) return XHE_OK;
    DevGuard dg(key->device);
    const size_t cb = (size_t)key->n2w * 4;
    const int64_t chunk = 1 << 16, cmax = std::min<int64_t>(chunk, count);
    std::unique_ptr<DevBuf> dinv[3];
    return host_pipeline(
        key, count, chunk, {{c, cb}, {k, (size_t)kw * 4}}, {{out, cb}},
        [&](int b, int64_t, int64_t n, void* const* din, void* const* dout, hipStream_t s) -> int {
          const uint32_t* base = (const uint32_t*)din[0];
          if (invert_first) {
            if (!dinv[b]) dinv[b].reset(new DevBuf((size_t)cmax * cb, s));
            int rc = xhe_invert(key, base, n, dinv[b]->as<uint32_t>(), s);
            if (rc != XHE_OK) return rc;
            base = dinv[b]->as<uint32_t>();
          }
          return xhe_powmod(key, base, (const uint32_t*)din[1], kw, kbits, n, (uint32_t*)dout[0], s);
        });
  });
}

int xhe_segprod_host(const xhe_key* key, const uint32_t* c, const int32_t* d, int dmax, int64_t count,
                     const int64_t* seg_begin, int64_t nseg, uint32_t* out) {
  return guarded([&]() -> int {
    if (!key || !seg_begin || nseg <= 0 || (count > 0 && !c) || !out) return fail(XHE_EINVAL, "xhe_segprod_host: bad argument");
    DevGuard dg(key->device);
    Stream st;
    size_t cw = (size_t)std::max<int64_t>(count, 1) * key->n2w * 4;
    DevBuf dc(cw, st.s), dd((size_t)std::max<int64_t>(count, 1) * 4, st.s), dout((size_t)nseg * key->n2w * 4, st.s);
    if (count > 0) HIPCHK(hipMemcpyAsync(dc.p, c, (size_t)count * key->n2w * 4, hipMemcpyHostToDevice, st.s));
    if (d && count > 0) HIPCHK(hipMemcpyAsync(dd.p, d, count * 4, hipMemcpyHostToDevice, st.s));
    int rc = xhe_segprod(key, dc.as<uint32_t>(), d ? dd.as<int32_t>() : nullptr, dmax, count, seg_begin, nseg,
                         dout.as<uint32_t>(), st.s);
    if (rc != XHE_OK) return rc;
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)nseg * key->n2w * 4, hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipStreamSynchronize(st.s));
    return XHE_OK;
  });
}

int xhe_segscan_host(const xhe_key* key, const uint32_t* c, int64_t count, const int64_t* seg_begin, int64_t nseg,
                     uint32_t* out) {
  return guarded([&]() -> int {
    if (int rc = segscan_args(key, c, count, seg_begin, nseg, out, "xhe_segscan_host")) return rc;
    if (count == 0) return XHE_OK;
    DevGuard dg(key->device);
    const size_t bytes = (size_t)count * key->n2w * 4;
    Stream st;
    DevBuf dc(bytes, st.s), dout(bytes, st.s);
    HIPCHK(hipMemcpyAsync(dc.p, c, bytes, hipMemcpyHostToDevice, st.s));
    int rc = xhe_segscan(key, dc.as<uint32_t>(), count, seg_begin, nseg, dout.as<uint32_t>(), st.s);
    if (rc != XHE_OK) return rc;
    HIPCHK(hipMemcpyAsync(out, dout.p, bytes, hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipStreamSynchronize(st.s));
    return XHE_OK;
  });
}

int xhe_multiexp(const xhe_key* key, const uint32_t* bases_dev, int64_t nbases, const int32_t* idx_dev,
                 const uint32_t* k_dev, int kw, int kbits, int64_t ncols, int64_t nterms, int win_bits,
                 uint32_t* out_dev, void* stream) {
  return guarded([&]() -> int {
    if (!key || nbases <= 0 || ncols <= 0 || nterms <= 0 || !bases_dev || !idx_dev || !k_dev || !out_dev || kw <= 0 ||
        kbits < 0 || kbits > 32 * kw || win_bits < 0 || win_bits > 8)
      return fail(XHE_EINVAL, "xhe_multiexp: bad argument");
    if (ncols * nterms > (int64_t)1 << 31 || nbases > (int64_t)1 << 30)
      return fail(XHE_EINVAL, "xhe_multiexp: problem too large for one call");
    DevGuard dg(key->device);
    const bool row = paths::n2_shape(std::max(nbases, ncols), pins()) == paths::N2Shape::ROW16;
    const int s4 = with_shape(key->K, [&](auto sh) -> int {
      using Sh = decltype(sh);
      return row ? Sh::MN2X::S4 : Sh::MN2::S4;
    });
    const int c = win_bits ? win_bits : mexp_window(nbases, ncols, nterms, std::max(kbits, 1), s4);
    const int kb = std::max(kbits, 1);
    hipStream_t hs = (hipStream_t)stream;
    with_shape(key->K, [&](auto sh) {
      using Sh = decltype(sh);
      if (row)
        multiexp_impl<Sh, typename Sh::MN2X>(key, bases_dev, nbases, idx_dev, k_dev, kw, kb, ncols, nterms, c, out_dev,
                                             hs);
      else
        multiexp_impl<Sh>(key, bases_dev, nbases, idx_dev, k_dev, kw, kb, ncols, nterms, c, out_dev, hs);
    });
    return XHE_OK;
  });
}

int xhe_multiexp_host(const xhe_key* key, const uint32_t* bases, int64_t nbases, const int32_t* idx, const uint32_t* k,
                      int kw, int kbits, int64_t ncols, int64_t nterms, int win_bits, uint32_t* out) {
  return guarded([&]() -> int {
    if (!key || nbases <= 0 || ncols <= 0 || nterms <= 0 || !bases || !idx || !k || !out || kw <= 0)
      return fail(XHE_EINVAL, "xhe_multiexp_host: bad argument");
    for (int64_t i = 0; i < ncols * nterms; ++i)
      if (idx[i] < 0 || idx[i] >= nbases) return fail(XHE_EINVAL, "xhe_multiexp_host: base index out of range");
    DevGuard dg(key->device);
    Stream st;
    DevBuf db((size_t)nbases * key->n2w * 4, st.s), di((size_t)ncols * nterms * 4, st.s),
        dk((size_t)ncols * nterms * kw * 4, st.s), dout((size_t)ncols * key->n2w * 4, st.s);
    HIPCHK(hipMemcpyAsync(db.p, bases, (size_t)nbases * key->n2w * 4, hipMemcpyHostToDevice, st.s));
    HIPCHK(hipMemcpyAsync(di.p, idx, (size_t)ncols * nterms * 4, hipMemcpyHostToDevice, st.s));
    HIPCHK(hipMemcpyAsync(dk.p, k, (size_t)ncols * nterms * kw * 4, hipMemcpyHostToDevice, st.s));
    int rc = xhe_multiexp(key, db.as<uint32_t>(), nbases, di.as<int32_t>(), dk.as<uint32_t>(), kw, kbits, ncols, nterms,
                          win_bits, dout.as<uint32_t>(), st.s);
    if (rc != XHE_OK) return rc;
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)ncols * key->n2w * 4, hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipStreamSynchronize(st.s));
    return XHE_OK;
  });
}

int xhe_fermat2_host(int device, int bits, const uint32_t* starts, int nstarts, const int32_t* which,
                     const uint32_t* offs, int64_t count, uint8_t* pass) {
  return guarded([&]() -> int {
    if (bits <= 0 || bits % 32 || !fermat_bits_supported(bits))
      return fail(XHE_ENOTSUP, "xhe_fermat2_host: prime width " + std::to_string(bits) + " not built");
    if (count < 0 || count > (int64_t)1 << 24 || nstarts <= 0 || !starts || (count > 0 && (!which || !offs || !pass)))
      return fail(XHE_EINVAL, "xhe_fermat2_host: bad argument");
    if (count == 0) return XHE_OK;
    const int nw = bits / 32;
    // per start: top bit set; do the words above the lowest all carry on?
    std::vector<uint8_t> ripples((size_t)nstarts);
    for (int s = 0; s < nstarts; ++s) {
      const uint32_t* w = starts + (size_t)s * nw;
      if (!(w[nw - 1] >> 31)) return fail(XHE_EINVAL, "xhe_fermat2_host: a start is below 2^(bits-1)");
      bool ones = true;
      for (int k = 1; k < nw; ++k) ones = ones && w[k] == 0xffffffffu;
      ripples[s] = ones;
    }
    for (int64_t i = 0; i < count; ++i) {
      if (which[i] < 0 || which[i] >= nstarts) return fail(XHE_EINVAL, "xhe_fermat2_host: start index out of range");
      const uint32_t lo = starts[(size_t)which[i] * nw], sum = lo + offs[i];
      if (!(sum & 1u)) return fail(XHE_EINVAL, "xhe_fermat2_host: an even candidate");
      if (sum < lo && ripples[which[i]]) return fail(XHE_EINVAL, "xhe_fermat2_host: a candidate reaches 2^bits");
    }
    DevGuard dg(device);
    Stream st;
    const size_t sb = (size_t)nstarts * nw * 4, cb = (size_t)count * 4;
    DevBuf ds(sb, st.s), dw(cb, st.s), dof(cb, st.s), dp((size_t)count, st.s);
    HIPCHK(hipMemcpyAsync(ds.p, starts, sb, hipMemcpyHostToDevice, st.s));
    HIPCHK(hipMemcpyAsync(dw.p, which, cb, hipMemcpyHostToDevice, st.s));
    HIPCHK(hipMemcpyAsync(dof.p, offs, cb, hipMemcpyHostToDevice, st.s));
    with_fermat_shape(bits, [&](auto m, auto width) {
      using M = decltype(m);
      constexpr int BITS = decltype(width)::value;
      const int64_t gpw = 64 / M::TPI;  // candidates per wave
      ProfScope ps("k_fermat2", st.s);
      launch((k_fermat2<M, BITS>), dim3((unsigned)((count + gpw - 1) / gpw)), dim3(64), st.s, ds.as<uint32_t>(),
             dw.as<int32_t>(), dof.as<uint32_t>(), count, dp.as<uint8_t>());
    });
    HIPCHK(hipMemcpyAsync(pass, dp.p, (size_t)count, hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipStreamSynchronize(st.s));
    return XHE_OK;
  });
}

int xhe_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int xhe_gather_rows(const uint32_t* src_dev, const int64_t* idx_dev, int64_t count, int words, uint32_t* dst_dev,
                    void* stream) {
  return guarded([&]() -> int {
    if (count < 0 || words <= 0) return fail(XHE_EINVAL, "xhe_gather_rows: bad size");
    if (count == 0) return XHE_OK;
    if (!src_dev || !idx_dev || !dst_dev) return fail(XHE_EINVAL, "xhe_gather_rows: null argument");
    const int64_t tot = count * words;
    const unsigned blocks = (unsigned)std::min<int64_t>((tot + 255) / 256, 65536);
    launch(k_move_rows<false>, dim3(blocks), dim3(256), (hipStream_t)stream, src_dev, idx_dev, count, words, dst_dev);
    return XHE_OK;
  });
}

int xhe_scatter_rows(const uint32_t* src_dev, const int64_t* idx_dev, int64_t count, int words, uint32_t* dst_dev,
                     void* stream) {
  return guarded([&]() -> int {
    if (count < 0 || words <= 0) return fail(XHE_EINVAL, "xhe_scatter_rows: bad size");
    if (count == 0) return XHE_OK;
    if (!src_dev || !idx_dev || !dst_dev) return fail(XHE_EINVAL, "xhe_scatter_rows: null argument");
    const int64_t tot = count * words;
    const unsigned blocks = (unsigned)std::min<int64_t>((tot + 255) / 256, 65536);
    launch(k_move_rows<true>, dim3(blocks), dim3(256), (hipStream_t)stream, src_dev, idx_dev, count, words, dst_dev);
    return XHE_OK;
  });
}

int xhe_wire_unpack(const uint8_t* bytes_dev, int64_t nbytes, const uint32_t* off_dev, const uint16_t* len_dev,
                    int64_t count, int n2w, uint32_t* rows_dev, void* stream) {
  return guarded([&]() -> int {
    if (count < 0 || nbytes < 0 || n2w <= 0 || n2w > 512 || n2w % 4) return fail(XHE_EINVAL, "xhe_wire_unpack: bad size");
    if (count == 0) return XHE_OK;
    if (!bytes_dev || !off_dev || !len_dev || !rows_dev) return fail(XHE_EINVAL, "xhe_wire_unpack: null argument");
    if (((uintptr_t)bytes_dev & 3) || ((uintptr_t)rows_dev & 15))
      return fail(XHE_EINVAL, "xhe_wire_unpack: bytes_dev must be 4-byte and rows_dev 16-byte aligned");
    const int64_t tot = count * (n2w / 4);
    const unsigned blocks = (unsigned)std::min<int64_t>((tot + 255) / 256, 65536);
    launch(k_wire_unpack, dim3(blocks), dim3(256), (hipStream_t)stream, bytes_dev, nbytes, off_dev, len_dev, count,
           n2w, rows_dev);
    return XHE_OK;
  });
}

int xhe_synchronize(void* stream) {
  hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) return fail(XHE_EHIP, hipGetErrorString(e));
  return XHE_OK;
}

int xhe_profile(int enable) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = enable != 0;
  for (auto& r : g_prof) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  g_prof.clear();
  return XHE_OK;
}

int xhe_profile_read(const char* kernel, double* total_ms, int64_t* launches) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  double t = 0;
  int64_t n = 0;
  for (auto& r : g_prof) {
    if (kernel && r.name != kernel) continue;
    if (hipEventSynchronize(r.b) != hipSuccess) return fail(XHE_EHIP, "xhe_profile_read: event sync failed");
    float ms = 0;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) return fail(XHE_EHIP, "xhe_profile_read: elapsed failed");
    t += ms;
    ++n;
  }
  if (total_ms) *total_ms = t;
  if (launches) *launches = n;
  return XHE_OK;
}


}  // extern "C"
