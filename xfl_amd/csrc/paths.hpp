// Which kernel path serves a call: every batch-size threshold, every $XHE_*
// kernel switch and every rule that combines them with the key's size and
// tables. Host-only and pure: standard headers, no HIP runtime call, no
// environment (parse_pins reads the switches through the lookup it is given),
// so the rules run - and are tested, tests/test_paths.py - on any machine.
// xhe.hip asks one function per decision and switches on the answer; the
// launches, grids and workspaces stay there.
//
// The functions take plain numbers: the key bits K, the lanes per residue of
// the limb shape in play (Mont<..>::TPI), the KeyDev flags that say which
// tables the key has, the element count the rule looks at, and the switches.
#pragma once
#include <cstdint>
#include <cstdlib>

namespace xhe {
namespace paths {

// ------------------------------------------------------------- switches
// One field per kernel switch (INTEGRATION.md "Other kernel switches"); the
// defaults are what an unset variable means. The integer pins hold an
// accepted value or their default: parse_pins drops everything else.
struct Pins {
  int enc_tpi = -1;   // $XHE_ENC_TPI: any value >= 0 pins (16 = the row shape, else not the row shape)
  int pmd_split = 0;  // $XHE_PMD_SPLIT: 1, 4 or 16 lanes per element of k_djn_pmd
  int pub_tpi = 0;    // $XHE_PUB_TPI: 64 (k_nodjn_pub_wave) or 4 (the lane kernels)
  int n2_tpi = 0;     // $XHE_N2_TPI: 4 or 16 lanes per n^2 residue
  int dec_tpi = 0;    // $XHE_DEC_TPI: 1, 4, 16 or 64
  // on unless the value starts with '0' (A/B measurements against the path each replaced)
  bool ndig_pub = true;   // $XHE_NDIG_PUB=0: public DJN keys keep Montgomery n^2 tables (k_djn_pub); read at key creation
  bool ndig = true;       // $XHE_NDIG=0: the Montgomery mod-n^2 kernels instead of the digit kernels
  bool nodjn_pmd = true;  // $XHE_NODJN_PMD=0: the Montgomery k_nodjn_crt
  bool add_wave = true;   // $XHE_ADD_WAVE=0: small adds keep the lane shapes
  bool add_bar = true;    // $XHE_ADD_BAR=0: the Montgomery pair (k_mulmod_n2) instead of k_add_barrett
  bool sum_words = true;  // $XHE_SUM_WORDS=0: the k_align_mont transpose before the first segment level
  bool mexp_wave = true;  // $XHE_MEXP_WAVE=0: k_mexp_horner in lanes
  bool dec_pmdx = true;   // $XHE_DEC_PMDX=0: the Montgomery decrypt shapes at 3072+ bits
  bool dec_rns = true;    // $XHE_DEC_RNS=0: k_dec_wave (the WaveMont product) instead of k_dec_rns
};

// lookup(name) -> const char* or null (xhe.hip passes getenv).
template <class Lookup>
Pins parse_pins(Lookup&& lookup) {
  auto on = [&](const char* name) {
    const char* e = lookup(name);
    return !(e && e[0] == '0');
  };
  auto num = [&](const char* name, int dflt) {
    const char* e = lookup(name);
    return e ? (int)atoll(e) : dflt;
  };
  auto one_of = [](int v, int a, int b, int c = 0, int d = 0) { return v && (v == a || v == b || v == c || v == d) ? v : 0; };
  Pins p;
  p.enc_tpi = num("XHE_ENC_TPI", -1);
  p.pmd_split = one_of(num("XHE_PMD_SPLIT", 0), 1, 4, 16);
  p.pub_tpi = one_of(num("XHE_PUB_TPI", 0), 4, 64);
  p.n2_tpi = one_of(num("XHE_N2_TPI", 0), 4, 16);
  p.dec_tpi = one_of(num("XHE_DEC_TPI", 0), 1, 4, 16, 64);
  p.ndig_pub = on("XHE_NDIG_PUB");
  p.ndig = on("XHE_NDIG");
  p.nodjn_pmd = on("XHE_NODJN_PMD");
  p.add_wave = on("XHE_ADD_WAVE");
  p.add_bar = on("XHE_ADD_BAR");
  p.sum_words = on("XHE_SUM_WORDS");
  p.mexp_wave = on("XHE_MEXP_WAVE");
  p.dec_pmdx = on("XHE_DEC_PMDX");
  p.dec_rns = on("XHE_DEC_RNS");
  return p;
}

// ------------------------------------------------- private DJN encryption
// Decided per launch chunk of n elements (a call over 2^20 elements may take
// another split on its tail).
enum class EncDjn {
  PMD,      // 2048: k_djn_pmd, one-lane Montgomery digits split over pmd_split(n) lanes
  PMDX,     // 3072+: k_djn_pmdx, digit pairs
  POW_X,    // keys without digit tables: k_djn_pow_x, one 16-lane DPP row per residue
  POW_LDS,  //   one lane per residue, table rows staged in LDS
  POW,      //   the batch shape's lanes
};

// DJN private encryption in the 16-lane shape up to kEncRowMax elements
// (tools/dec_shapes.py --enc: 64 elements 0.50 ms vs 1.95 ms one lane per
// residue, 16 k 1.86 vs 2.16 ms, 64 k 6.2 vs 3.8 ms); $XHE_ENC_TPI (16 or 0)
// pins it.
constexpr int64_t kEncRowMax = 20480;

inline EncDjn enc_djn(int K, int mp2_lanes, bool pmd, bool pmdx, int64_t n, const Pins& pins) {
  if (K == 2048 && pmd) return EncDjn::PMD;
  if (K != 2048 && pmdx) return EncDjn::PMDX;
  const bool row = pins.enc_tpi >= 0 ? pins.enc_tpi == 16 : n <= kEncRowMax;
  return row ? EncDjn::POW_X : mp2_lanes == 1 ? EncDjn::POW_LDS : EncDjn::POW;
}

// lanes per element of k_djn_pmd: 16 up to 2 k elements, 4 up to 16 k, else
// 1 (the chip holds ~128 k one-lane residues: 2 waves x 1024 SIMDs x 64);
// $XHE_PMD_SPLIT pins it (1, 4 or 16)
constexpr int64_t kPmdSplit16Max = 2048, kPmdSplit4Max = 16384;

inline int pmd_split(int64_t n, const Pins& pins) {
  if (pins.pmd_split) return pins.pmd_split;
  return n <= kPmdSplit16Max ? 16 : n <= kPmdSplit4Max ? 4 : 1;
}

// -------------------------------------------------- public DJN encryption
enum class EncPubDjn {
  PUB_ND,  // 2048: k_djn_pub_nd, fixed-base products in Montgomery digits of n
  PUB,     // k_djn_pub on Montgomery n^2 tables
};

// (Pins::ndig_pub acts where the tables are built: a key made with it off has no pub_nd)
inline EncPubDjn enc_pub_djn(int K, bool pub_nd) { return K == 2048 && pub_nd ? EncPubDjn::PUB_ND : EncPubDjn::PUB; }

// ----------------------------------------------------- non-DJN encryption
// Decided by the whole call's count.
enum class EncNoDjn {
  PMD,       // 2048, private: the decrypt's digit exponentiation (k_dec_pmd_pow), then CRT
  PUB_WAVE,  // 2048, public: k_nodjn_pub_wave, one 16-wave block per element
  CRT,       // private: k_nodjn_crt (a 2-lane batch shape runs it in the 4-lane shape)
  NDIG,      // 2048, public: the digit kernels k_ndig_*
  PUB,       // public: k_nodjn_pub
};

// Public non-DJN encryption of 2048-bit keys by batch size: one 16-wave block
// per element (k_nodjn_pub_wave) up to kPubWaveMax elements - the 4-lane digit
// kernels take the same time for 1 element as for 8 k (one wave's chain of
// products: 47.4 ms at 15, 48.9 ms at 8 k) - and the digit kernels beyond
// (tools/dec_shapes.py --pub, profiles/r9/pub_small/: 6.7 ms up to 256
// elements, one block a CU; 20.8 ms at 1 k, 40.4 vs 48.7 ms at 2 k, 79.6 vs
// 48.9 ms at 4 k). $XHE_PUB_TPI (64 or 4) pins one path (A/B measurement).
// Mirrored as xfl_amd._native.PUB_WAVE_MAX.
constexpr int64_t kPubWaveMax = 2048;

inline EncNoDjn enc_nodjn(int K, bool priv, bool ndig, int64_t count, const Pins& pins) {
  if (K == 2048 && priv && pins.nodjn_pmd) return EncNoDjn::PMD;
  if (K == 2048 && !priv && (pins.pub_tpi ? pins.pub_tpi == 64 : count <= kPubWaveMax)) return EncNoDjn::PUB_WAVE;
  if (priv) return EncNoDjn::CRT;
  return K == 2048 && ndig && pins.ndig ? EncNoDjn::NDIG : EncNoDjn::PUB;
}

// ------------------------------------------------------ n^2 ciphertext ops
// Shape of the n^2 ciphertext ops (mulmod, powmod, invert, segprod, multiexp)
// by batch size: one 16-lane DPP row per residue up to kN2RowMax elements
// (latency-bound: a few ciphertexts leave the chip idle and each element's
// chain of dependent products sets the time), the batch shape beyond (4 lanes
// at 2048 and 3072 bits). $XHE_N2_TPI (4 or 16) pins one shape (A/B
// measurement). Multiexp passes max(nbases, ncols).
// (xhe_segscan takes this shape too; its chunks and levels are planned in
// scan_plan.hpp, a pure header like this one.)
enum class N2Shape { ROW16, LANES4 };
constexpr int64_t kN2RowMax = 4096;

inline N2Shape n2_shape(int64_t count, const Pins& pins) {
  return (pins.n2_tpi ? pins.n2_tpi == 16 : count <= kN2RowMax) ? N2Shape::ROW16 : N2Shape::LANES4;
}

// The functions below take the lanes of the shape n2_shape chose (16, or the
// batch shape's: 4 at 2048 bits).

enum class Add {
  WAVE,     // 2048: k_mulmod_wave, one 16-wave block per element
  BARRETT,  // 2048, 4 lanes, equal exponents: the one-product k_add_barrett
  MONT,     // k_mulmod_n2
};

// Adds of a few elements run one 16-wave block per element (k_mulmod_wave,
// 2048-bit keys) up to kWaveAddMax elements, with or without alignment
// squarings (the plain product of the LR step's noise add, 15 elements, took
// 56 us in the 16-lane k_mulmod_n2).
constexpr int64_t kWaveAddMax = 256;

inline Add add(int K, int lanes, int64_t count, int dmax, const Pins& pins) {
  if (K == 2048 && count <= kWaveAddMax && pins.add_wave) return Add::WAVE;
  if (K == 2048 && lanes == 4 && dmax == 0 && pins.add_bar) return Add::BARRETT;
  return Add::MONT;
}

enum class Pow {
  NDIG,  // 2048, 4 lanes: the digit kernels k_ndig_*
  MONT,  // k_powmod_n2
};

inline Pow powmod(int K, int lanes, bool ndig, const Pins& pins) {
  return K == 2048 && lanes == 4 && ndig && pins.ndig ? Pow::NDIG : Pow::MONT;
}

// Ciphertext packing (xhe_pack): one lane group per output walks a chain of
// (k - 1) shift_bits dependent squarings, so the launch takes the chain's
// time whatever the batch and the wider shape wins for longer than in the
// other n^2 ops. The 16-lane row serves up to kPackRowMax outputs, the batch
// shape beyond - at 2048 bits in Montgomery digits (k_ndig_pack) where powmod
// would take them. $XHE_N2_TPI (4 or 16) pins the shape, $XHE_NDIG=0 the
// Montgomery-limb kernel (k_pack_n2).
// k = 7, shift_bits = 256 at 2048 bits (tools/bench_pack.py --shapes,
// profiles/r21/pack_shapes.json and pack_shapes_sweep.json), 16 lanes vs the
// 4-lane digits vs 4-lane Montgomery limbs: 512 outputs 18.7 / 28.2 / 45.0 ms,
// 2,341 18.9 / 28.1 / 44.9 ms, 4,096 18.9 / 28.2 / 45.2 ms, 16,384 54.9 /
// 48.9 / 45.6 ms. The 16-lane time steps up right behind 4,096 outputs (256
// blocks, one a CU: 5,120 - 8,192 outputs 30.0 vs 28.5 ms in digits; 12,288
// 42.8 vs 49.2 ms; 32,768 105 vs 50 ms), so the crossover stays where
// kN2RowMax has it.
struct Pack {
  N2Shape shape;
  Pow arith;  // NDIG: k_ndig_in / k_ndig_pack / k_ndig_out; MONT: k_pack_n2
};
constexpr int64_t kPackRowMax = kN2RowMax;

// lanes: the batch n^2 shape's lanes per residue (Shape::MN2::TPI)
inline Pack pack(int K, int lanes, bool ndig, int64_t ngroups, const Pins& pins) {
  const N2Shape shape =
      (pins.n2_tpi ? pins.n2_tpi == 16 : ngroups <= kPackRowMax) ? N2Shape::ROW16 : N2Shape::LANES4;
  return {shape, shape == N2Shape::LANES4 ? powmod(K, lanes, ndig, pins) : Pow::MONT};
}

enum class Invert {
  WTREE,  // 2048, 16 lanes: a product tree of whole-block products (k_wtree_*), one launch per level
  TREE,   // k_tree_up / k_tree_down in lanes
};
constexpr int64_t kWtreeMax = 256;

inline Invert invert(int K, int lanes, int64_t count) {
  return K == 2048 && lanes == 16 && count <= kWtreeMax ? Invert::WTREE : Invert::TREE;
}

// First level of a segmented product: with no alignment anywhere it reads the
// ciphertext words itself.
enum class SegFirst {
  WORDS,  // k_chunk_prod_words on the input
  ALIGN,  // the k_align_mont transpose (and squarings) first
};

inline SegFirst segprod_first(int64_t count, int dmax, bool has_d, const Pins& pins) {
  return count > 0 && (dmax == 0 || !has_d) && pins.sum_words ? SegFirst::WORDS : SegFirst::ALIGN;
}

enum class Horner {
  WAVE,   // 2048, 16 lanes: k_mexp_horner_wave, one 16-wave block per column (latency)
  LANES,  // k_mexp_horner
};
constexpr int64_t kMexpWaveMax = 4096;

inline Horner mexp_horner(int K, int lanes, int64_t ncols, const Pins& pins) {
  return K == 2048 && lanes == 16 && pins.mexp_wave && ncols <= kMexpWaveMax ? Horner::WAVE : Horner::LANES;
}

// ----------------------------------------------------------------- decrypt
// Decided by the whole call's count: every launch chunk takes the same path.
enum class Dec {
  PMDX,   // 3072+: the exponentiation in Montgomery digits (k_dec_pmdx_*)
  RNS,    // 2048: k_dec_rns, one block of 384 threads per residue
  WAVE,   // 2048: k_dec_wave, the WaveMont product
  ROW16,  // k_dec_pow, one 16-lane DPP row per residue
  QUAD4,  // k_dec_pow, 4 lanes per residue
  PMD1,   // 2048: one lane per residue in Montgomery digits (k_dec_pmd_*)
  POW1,   // 3072+: k_dec_pow in the batch shape (pinned only)
};

// Decrypt exponentiation shapes by batch size (latency- vs throughput-bound):
// one 16-lane DPP row per residue up to kDecRowMax elements, 4 lanes up to
// kDecQuadMax, one lane beyond (crossovers measured with tools/dec_shapes.py:
// 16 lanes 6.0 ms flat to 1 k elements, 8.9 ms at 4 k, 15.8 ms at 8 k vs
// 11.3/11.8/11.9 ms for 4 lanes; 4 lanes 20-21 ms at 16 k vs 36 ms for 1
// lane, 40 ms at 32 k vs 37 ms). $XHE_DEC_TPI (1, 4 or 16) pins one shape.
constexpr int64_t kDecRowMax = 5120;
// One block of rns::NT = 384 threads (six waves; two blocks per CU by its
// launch bounds) per residue (k_dec_rns, 2048-bit keys) up to kDecWaveMax
// elements (tools/dec_shapes.py, profiles/r6: 1,024 elements
// 5.68 ms vs 6.11 ms in 16 lanes, 1,536 8.34 vs 6.13 ms); $XHE_DEC_TPI=64
// pins it.
constexpr int64_t kDecWaveMax = 1024;
constexpr int64_t kDecQuadMax = 28672;

// mp2_lanes: lanes of the key size's batch p^2 shape (MP2::TPI). Multi-lane
// key sizes take the 4-lane shape for every larger batch: at 3072 bits the
// 2-lane batch shape (55 limbs per lane) decrypted 25.5 k/s where 4096 bits
// in 4 lanes reach 133 k/s (profiles/r1/keysizes/). The digit decrypt of the
// larger keys replaces the 4-lane shape where the batch size chose it, and
// the one-lane pin (the 16-lane shape keeps the small batches).
inline Dec decrypt(int K, int mp2_lanes, bool pmdx_dec, bool rns, int64_t count, const Pins& pins) {
  const int pin = pins.dec_tpi;
  const int tpi = pin ? (pin == 64 && K != 2048 ? 16 : pin)
                  : (K == 2048 && count <= kDecWaveMax)     ? 64
                  : count <= kDecRowMax                     ? 16
                  : (count <= kDecQuadMax || mp2_lanes > 1) ? 4
                                                            : 1;
  if (K != 2048 && pmdx_dec && pins.dec_pmdx && (pin ? pin == 1 : tpi == 4)) return Dec::PMDX;
  if (tpi == 64) return rns && pins.dec_rns ? Dec::RNS : Dec::WAVE;
  if (tpi == 16) return Dec::ROW16;
  if (tpi == 4) return Dec::QUAD4;
  return K == 2048 ? Dec::PMD1 : Dec::POW1;
}

}  // namespace paths
}  // namespace xhe
