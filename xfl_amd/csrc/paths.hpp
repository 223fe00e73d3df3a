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

// ------------------------------------------------------- fused histogram
// xhe_hist (hist_dev.hpp): elements per tile. About kRawChunk = 32 rows per
// (bin, tile) - one slice per bin, so a block's products are the elements'
// plus one per bin - that is 32 nbins rounded up to a power of two in
// [kHistTileMin, kHistTileMax], but at least a slice for each of a block's 64
// lane groups (32 x 64 rows: with 32 nbins alone a 2-bin histogram ran 2 of
// its 64 groups per block, 485 ms for config 5's rows against 23 ms at 256
// bins; the bins' further slices are combined in the block); halved while nfeat x tiles blocks would leave
// the chip short of two blocks per CU (kHistFillBlocks = 512 blocks of 256
// threads: the 131072 lanes reduce_segments' kFill counts), since a short grid
// costs more than the extra product per shorter slice. Runs in the batch n^2
// shape (Sh::MN2) whatever the count: $XHE_N2_TPI does not apply.
constexpr int kHistTileMin = 64, kHistTileMax = 8192;
constexpr int64_t kHistFillBlocks = 512;

inline bool hist_tile_ok(int tile_rows) {
  return tile_rows >= kHistTileMin && tile_rows <= kHistTileMax && (tile_rows & (tile_rows - 1)) == 0;
}

inline int hist_tile(int64_t count, int nfeat, int nbins) {
  int tile = kHistTileMin;
  while (tile < kHistTileMax && tile < 32 * (int64_t)(nbins > 64 ? nbins : 64)) tile <<= 1;
  while (tile > kHistTileMin && (int64_t)nfeat * ((count + tile - 1) / tile) < kHistFillBlocks) tile >>= 1;
  return tile;
}

// Dynamic LDS of k_hist_tile: two words per bin, the work list, the element list.
inline int64_t hist_lds_bytes(int tile_rows, int nbins) {
  return 8 * (int64_t)nbins + 4 * (int64_t)(tile_rows / 32) + 2 * (int64_t)tile_rows;
}

// Features per launch group: the partial rows (nbins per feature and tile)
// and the parked rows (tile_rows / 16 per block) of one group stay within
// cap_rows residue rows (the launch layer's kChunk), at least one feature.
inline int hist_group(int nfeat, int nbins, int tile_rows, int64_t tiles, int64_t cap_rows) {
  const int64_t per_feat = tiles * ((int64_t)nbins + tile_rows / 16);
  const int64_t g = cap_rows / (per_feat > 0 ? per_feat : 1);
  return (int)(g < 1 ? 1 : g > nfeat ? nfeat : g);
}

// ------------------------------------- histogram over mixed exponents
// xhe_hist_exp (hist_exp_dev.hpp): k_hexp_tile orders a tile by (bin, exponent)
// with a sort in LDS - a 4-byte key and a 2-byte index per element, two words
// per bin, the work list and the parked rows' exponents (2 bytes per 16
// elements). The tile is hist_tile's (the same products per block, plus the
// squarings), halved while that does not fit the 64 KB a launch gets without
// opting in (less the kernel's few static words): a capacity rule, no tuning.
// It bites from 1761 bins on (8192 rows), and leaves 4096 rows at 4096 bins.
// A caller's tile_rows goes through the same halving: the result does not
// depend on the tile.
constexpr int64_t kHistExpLdsMax = 65536 - 256;

inline int64_t hist_exp_lds_bytes(int tile_rows, int nbins) {
  return 6 * (int64_t)tile_rows + 8 * (int64_t)nbins + 4 * (int64_t)(tile_rows / 32) + 2 * (int64_t)(tile_rows / 16);
}

inline int hist_exp_fit(int tile_rows, int nbins) {
  while (tile_rows > kHistTileMin && hist_exp_lds_bytes(tile_rows, nbins) > kHistExpLdsMax) tile_rows >>= 1;
  return tile_rows;
}

inline int hist_exp_tile(int64_t count, int nfeat, int nbins) {
  return hist_exp_fit(hist_tile(count, nfeat, nbins), nbins);
}

// The largest exponent spread xhe_hist_exp serves for an n of n_bits bits:
// from n_bits - 1 on, 1 << gap reaches min_value_for_negative and the
// reference's alignment takes _raw_mul's negative branch (xhe_mulmod).
inline int hist_exp_dmax(int n_bits) { return n_bits - 2; }

// ------------------------------------------- level-wise histogram
// xhe_hist_level (hist_level_dev.hpp): every node of a tree level from one
// pass. The rows are ordered by node into tile slots that each lie inside one
// node, so the tile is hist_tile's, but not above the power of two at or
// above the mean node size n_rows / nnodes (floor kHistTileMin): most nodes
// are then one tile, the partial rows are about the output itself and the
// fold is nearly a copy. A node of c rows takes ceil(c / tile) slots; the sum
// over the nodes is at most floor(n_rows / tile) + nnodes, which the host
// knows without reading a count back: level_tiles_max sizes every grid and
// workspace (a slot behind the used ones returns at once). The LDS layout is
// k_hist_tile's (hist_lds_bytes) and the features run in hist_group's groups
// with level_tiles_max in place of the tile count.
constexpr int kLevelNodesMax = 4096;

inline int level_tile(int64_t n_rows, int nnodes, int nfeat, int nbins) {
  int tile = hist_tile(n_rows, nfeat, nbins);
  const int64_t mean = (n_rows + nnodes - 1) / (nnodes > 0 ? nnodes : 1);
  int cap = kHistTileMin;
  while (cap < kHistTileMax && cap < mean) cap <<= 1;
  return tile < cap ? tile : cap;
}

inline int64_t level_tiles_max(int64_t n_rows, int nnodes, int tile_rows) {
  return (n_rows + tile_rows - 1) / tile_rows + nnodes;
}

// Fold passes before the last one: a node's partial rows are folded in
// chunks of at most `chunk` (kRawChunk) until that many are left; no node has
// more than ceil(n_rows / tile) of them.
inline int level_fold_passes(int64_t n_rows, int tile_rows, int chunk) {
  int64_t t = (n_rows + tile_rows - 1) / tile_rows;
  int p = 0;
  for (; t > chunk; ++p) t = (t + chunk - 1) / chunk;
  return p;
}

// --------------------------------------------- histogram subtraction
// xhe_hist_level_sub (hist_sub_dev.hpp) multiplies only the smaller child of
// every pair of level slots from its rows and takes the sibling as parent /
// built. Products mod n^2 of a level, nfeat times
//   direct     n_rows
//   subtract   n_rows / 2 + 4 (nnodes / 2) nbins
// (the built children hold at most half the rows - the host does not know the
// real split, so the plan takes the balanced bound - and the sibling pass
// costs four products per built (pair, feature, bin) row). The route
// subtracts when direct >= kSubMinSaving x subtract, for an even nnodes >= 2.
// kSubMinSaving is a measured figure, not the model's 1 (DESIGN "Histogram
// subtraction", profiles/r27/hist_sub/): on config 5 (100 k rows x 64 features
// x 256 bins, 2048 bits) the balanced level was faster by subtraction at every
// node count measured, 2 to 64, by 2.7 ms of 24 at 64 nodes against a spread of
// 0.6 ms; 64 nodes is the model's ratio 1.208, the lowest one measured. The
// route subtracts down to that ratio and no further: nothing beyond 64 nodes
// (1.0 at 98 nodes) was measured.
constexpr double kSubMinSaving = 1.2;

inline bool level_sub(int64_t n_rows, int nnodes, int nfeat, int nbins) {
  if (nnodes < 2 || (nnodes & 1) || n_rows < 1 || nfeat < 1 || nbins < 1) return false;
  const double direct = (double)n_rows * nfeat;
  const double sub = (0.5 * (double)n_rows + 4.0 * (nnodes / 2) * nbins) * nfeat;
  return direct >= kSubMinSaving * sub;
}

// Rows per chunk of the sibling pass over M built rows: as many chunks as
// kSibFillGroups lane groups (131072 lanes of 4) while a chunk keeps at least
// kSibChunkMin rows - each chunk total costs the inversion tree about seven
// products more - and at most kSibChunkMax = kRawChunk, the exit rows of Rpow.
constexpr int kSibChunkMin = 4, kSibChunkMax = 32;
constexpr int64_t kSibFillGroups = 32768;

inline int sib_chunk(int64_t M) {
  const int64_t c = M / kSibFillGroups;
  return (int)(c < kSibChunkMin ? kSibChunkMin : c > kSibChunkMax ? kSibChunkMax : c);
}

// ------------------------------------------------ sparse-aware histogram
// xhe_hist_sparse (hist_sparse_dev.hpp) multiplies, per feature, only the
// entries outside the feature's zero bin and rebuilds that bin from the
// product T of all elements. The kept entries of a feature are compacted into
// tile slots that each lie inside one feature, so the tile is hist_tile's for
// the mean list length nnz_bound / nfeat and nbins + 1 internal bins, but not
// above the power of two at or above that mean (floor kHistTileMin):
// level_tile's reasoning with the feature in the node's place. A feature with
// c kept entries takes ceil(c / tile) slots; the sum is at most floor(
// nnz_bound / tile) + nfeat, which sizes every grid and workspace. Products
// mod n^2 of a call:
//   direct   nfeat count
//   sparse   nnz + (T given ? 0 : count) + (nbins + 1) slots + nfeat (nbins + 4)
// (a partial row per (slot, internal bin) to fold, and per feature the nbins
// rows of Q_f, its share of the inversion tree and the two products of the
// zero bin). The route takes the sparse call when direct >= kSparseMinSaving
// x sparse. kSparseMinSaving is a measured figure, not the model's 1 (DESIGN
// "Sparse-aware histogram", profiles/r28/hist_sparse/): on config 5 (100 k rows
// x 64 features x 256 bins, 2048 bits, bin 0 every feature's zero bin), ms of
// xhe_hist / xhe_hist_sparse and the model's ratio by the fraction d of rows
// outside the zero bin:
//   d      T given                  T computed
//   0.5    18.44 / 14.71   1.865    18.49 / 19.47   1.812   (slower)
//   0.25   18.44 / 10.03   3.493    18.54 / 14.74   3.312
//   0.1    18.15 /  5.72   7.673    17.96 / 10.33   6.852
//   0.05   17.41 /  4.51   12.455   17.18 /  9.07   10.426
//   0.01   16.58 /  2.85   28.166   16.47 /  7.33   19.558
// against a spread of 0.4 ms. 1.865 is the lowest ratio measured faster (by 3.7
// ms) and 1.812 the one measured slower (by 1 ms: computing T took 3.9 ms,
// thirteen times the `count` products the model charges), so the route stops
// between them. Nothing between 1.865 and 3.312 was measured without T.
constexpr int kSparseBinsMax = 4095;
constexpr double kSparseMinSaving = 1.86;

inline int sparse_tile(int64_t nnz_bound, int nfeat, int nbins) {
  const int64_t mean = (nnz_bound + nfeat - 1) / (nfeat > 0 ? nfeat : 1);
  int tile = hist_tile(mean, nfeat, nbins + 1);
  int cap = kHistTileMin;
  while (cap < kHistTileMax && cap < mean) cap <<= 1;
  return tile < cap ? tile : cap;
}

inline int64_t sparse_tiles_max(int64_t nnz_bound, int nfeat, int tile_rows) { return nnz_bound / tile_rows + nfeat; }

inline bool hist_sparse(int64_t count, int nfeat, int nbins, int64_t nnz, bool have_total) {
  if (count < 1 || nfeat < 1 || nbins < 1 || nbins > kSparseBinsMax || nnz < 0 || nnz > (int64_t)nfeat * count)
    return false;
  const double slots = (double)sparse_tiles_max(nnz, nfeat, sparse_tile(nnz, nfeat, nbins));
  const double direct = (double)nfeat * (double)count;
  const double sparse =
      (double)nnz + (have_total ? 0.0 : (double)count) + (nbins + 1.0) * slots + (double)nfeat * (nbins + 4.0);
  return direct >= kSparseMinSaving * sparse;
}

// ------------------------------------------- level-wise sparse histogram
// xhe_hist_level_sparse (hist_level_sparse_dev.hpp): xhe_hist_sparse with the
// nnodes x nfeat groups (node, feature) in the features' place. sparse_tile's
// reasoning holds per group: hist_tile for the mean list length nnz_bound /
// groups and nbins + 1 internal bins, but not above the power of two at or
// above that mean (floor kHistTileMin). At deep levels the mean group is a few
// dozen entries, the tile is the floor and most groups are one short slot: a
// larger tile would only lengthen the slot's LDS passes over ids it does not
// have. The slots are at most floor(nnz_bound / tile) + groups, which sizes
// every grid and workspace.
// The route's model counts in units of one entry of the dense level call (3.2
// ns on config 5), with weights fitted to the stage times of the measured
// tables (DESIGN "Level-wise sparse histogram", JSON in
// profiles/r29/hist_level_sparse/):
//   direct   nfeat n_rows + kLevelGroupCost groups nbins
//   sparse   kLspEntryCost nnz + kLspFoldCost (nbins + 1) slots + 4 groups + kLspFixedCost
//            + (totals given ? 0 : kLspTotalCost n_rows)
// - the dense call pays per (node, feature), but how much depends on the data:
//   with a heavy zero bin it takes 19 ms at 2 nodes, 33 to 40 at 64 and 108 at
//   256 for the same 6.4 M entries (5 us a group), with uniform bins (d = 1.0)
//   17 ms at 2 nodes and 23.6 at 64 (1.6 us a group). The model charges the
//   smaller figure, two entries' time per bin of every group, since the route
//   does not know the skew;
// - an entry of a slot costs 1.16 dense entries (the row id list in between);
// - a partial row per (slot, internal bin) to fold and reduce, 0.9 each (0.6
//   to 0.8 us a slot at 257 bins), and per group the inversion tree's share and
//   the two products of the zero bin;
// - 3 ms that no shape gets under - the order launches, the fold and zero
//   stages at their smallest, the synchronisation - as 930 k entries;
// - the totals: 5.2 to 5.8 ms per 100 k rows, seventeen entries a row.
// The route takes the sparse call when direct >= kLevelSparseMinSaving x
// sparse. Over the 48 measured points (1 to 256 nodes, d 0.05 to 1.0, with and
// without totals; ms of xhe_hist_level / xhe_hist_level_sparse) around the
// crossover:
//   ratio   nodes  d     totals     dense / sparse ms
//   0.916   1      0.8   given      18.48 / 20.04   slower
//   0.918   2      0.8   given      19.85 / 19.87   a tie
//   0.955   16     0.8   given      25.13 / 19.69   faster, not taken
//   1.001   2      0.5   computed   20.54 / 20.39   a tie
//   1.010   64     0.8   given      36.31 / 27.45   faster, not taken
//   1.024   16     0.5   computed   26.25 / 20.50   faster, not taken
//   1.059   64     0.5   computed   40.05 / 27.04   faster
//   1.092   1      0.65  given      18.76 / 15.15   faster
//   1.095   2      0.65  given      20.23 / 19.37   faster by 4 %
// Every point the route takes at 1.05 (23 of the 48) was measured faster, by 4
// % to 4.1 x; no point measured slower or tied has a ratio above 1.001 (full
// density, d = 1.0, is 0.63 to 0.85 at every node count and 1.3 to 1.8 x
// slower). The price of charging the dense call its uniform-bins cost is on
// the other side: between 0.84 and 1.03 five points measured faster by 7 to 32
// % are left to the dense call (sparse=True takes them). Only config 5's shape
// and key size were measured; the weights per bin and per slot follow the
// kernels' structure but were not measured at another nbins. Nothing above 256
// nodes was measured either: there the model promises the most and the
// accumulator rows double the call's memory, so the route leaves levels beyond
// kLevelSparseNodesMeasured to the dense call.
constexpr double kLevelSparseMinSaving = 1.05;
constexpr int kLevelSparseNodesMeasured = 256;
constexpr double kLevelGroupCost = 2.0, kLspEntryCost = 1.16, kLspFoldCost = 0.9, kLspFixedCost = 930000.0,
                 kLspTotalCost = 17.0;

inline int level_sparse_tile(int64_t nnz_bound, int nnodes, int nfeat, int nbins) {
  const int64_t groups = (int64_t)(nnodes > 0 ? nnodes : 1) * (nfeat > 0 ? nfeat : 1);
  const int64_t mean = (nnz_bound + groups - 1) / groups;
  int tile = hist_tile(mean, (int)(groups < (1 << 30) ? groups : (1 << 30)), nbins + 1);
  int cap = kHistTileMin;
  while (cap < kHistTileMax && cap < mean) cap <<= 1;
  return tile < cap ? tile : cap;
}

inline int64_t level_sparse_tiles_max(int64_t nnz_bound, int nnodes, int nfeat, int tile_rows) {
  return nnz_bound / tile_rows + (int64_t)nnodes * nfeat;
}

inline bool level_sparse(int64_t n_rows, int nnodes, int nfeat, int nbins, int64_t nnz, bool have_total) {
  if (n_rows < 1 || nnodes < 1 || nnodes > kLevelSparseNodesMeasured || nfeat < 1 || nbins < 1 ||
      nbins > kSparseBinsMax || nnz < 0 || nnz > (int64_t)nfeat * n_rows)
    return false;
  const int tile = level_sparse_tile(nnz, nnodes, nfeat, nbins);
  const double slots = (double)level_sparse_tiles_max(nnz, nnodes, nfeat, tile);
  const double groups = (double)nnodes * nfeat;
  const double direct = (double)nfeat * (double)n_rows + kLevelGroupCost * groups * nbins;
  const double sparse = kLspEntryCost * (double)nnz + kLspFoldCost * (nbins + 1.0) * slots + 4.0 * groups +
                        kLspFixedCost + (have_total ? 0.0 : kLspTotalCost * (double)n_rows);
  return direct >= kLevelSparseMinSaving * sparse;
}

// ------------------------------- subtraction on the sparse level histogram
// xhe_hist_level_sub_sparse (hist_sub_sparse_dev.hpp): the smaller child of
// every pair, and of it only the entries outside the zero bins. The build is
// the level-sparse call's on npairs = nnodes / 2 nodes; its tile and slot bound
// take the caller's whole nnz_bound (the device checks the built half against
// it: the host does not know the split), so
//   tile   level_sparse_tile(nnz_bound, npairs, ...)
//   slots  level_sparse_tiles_max(nnz_bound, npairs, ...)
// The inversion list holds the built cells with an entry outside their zero bin
// - no more than there are cells, M = npairs nfeat nbins, nor than entries -
// then one Q per group and one T per pair: sub_sparse_list bounds it and sizes
// the chains' grids, the parked prefixes and the chunk totals.
inline int64_t sub_sparse_list(int64_t M, int64_t nnz_bound, int64_t groups, int npairs) {
  return (nnz_bound < M ? nnz_bound : M) + groups + npairs;
}

// The route, in level_sparse's units (one entry of the dense level call, 3.2
// ns on config 5): three linear costs fitted by least squares to the measured
// table (DESIGN "Subtraction on the sparse level histogram",
// profiles/r30/hist_level_sub_sparse/: config 5 at 2, 16 and 64 uniformly
// drawn nodes, d = 0.05 .. 0.8 of the entries outside the zero bins, with and
// without totals). groups = nnodes nfeat, M = (nnodes / 2) nfeat nbins cells:
//   sparse    kSssSparseFixed + kSssSparseEntry nnz + kSssSparseGroup groups
//             + (totals given ? 0 : kSssSparseTotal n_rows)
//   sub       nfeat n_rows / 2 + kSssSubFixed + kSssSubEntry nnz + kSssSubCell M
//   combined  kSssFixed + kSssEntry nnz / 2 + kSssCell M + kSssListed min(nnz / 2, M)
//             + (totals given ? 0 : kSssTotal n_rows / 2)
// The planner does not know the split and takes the balanced one, as level_sub
// does. A listed cell costs 3.5 entries on top of the 2.6 every cell costs (the
// mark, the fill or the four chain products); the built children's totals cost
// what all the nodes' totals cost (hist_level_impl walks every row's node id).
// The fit is within 2.3 ms of every measured call, which is more than the 0.5 to
// 1.5 ms by which the combined call beats the sparse one at 64 nodes, so the
// route keeps margins: the combined call runs when the sparse call costs at
// least kSubSparseOverSparse and the subtraction at least kSubSparseOverSub
// times as much. The second margin is the skewed split's: with 10 % of every
// pair's rows in the built child the subtraction gains more than the combined
// call, and the measured sub / combined ratio fell from 1.05 to 0.82 (2 nodes, d
// = 0.8, totals given: the one point where the split turned a win into a loss)
// and from 1.39 to 1.12 at d = 0.5. At these margins the route takes five of
// the 24 measured (nodes, d, totals) points - 2 nodes at d = 0.2 and 0.5 and 16
// nodes at d = 0.5 with totals given, 64 nodes at d = 0.05 with and without -
// each measured faster than both others by 5 to 28 % in the uniform and in the
// skewed table; it takes no point measured slower in either, and leaves the
// other winners to subtract=True with sparse=True. It answers 1 only inside
// the measured range: an even nnodes of 2 .. kSubSparseNodesMeasured and
// kSubSparseDensityMin <= nnz / (nfeat n_rows) <= kSubSparseDensityMax. Only
// config 5's shape and key size were measured.
constexpr double kSssSparseFixed = 1114000.0, kSssSparseEntry = 0.958, kSssSparseGroup = 601.0, kSssSparseTotal = 17.0;
constexpr double kSssSubFixed = 1042000.0, kSssSubEntry = 0.132, kSssSubCell = 8.65;
constexpr double kSssFixed = 1223000.0, kSssEntry = 1.208, kSssCell = 2.566, kSssListed = 3.469, kSssTotal = 33.7;
constexpr double kSubSparseOverSparse = 1.10, kSubSparseOverSub = 1.40;
constexpr int kSubSparseNodesMeasured = 64;
constexpr double kSubSparseDensityMin = 0.05, kSubSparseDensityMax = 0.8;

// The combined call's cost above (an even nnodes)
inline double level_sub_sparse_cost(int64_t n_rows, int nnodes, int nfeat, int nbins, int64_t nnz, bool have_total) {
  const double half = 0.5 * (double)nnz, M = 0.5 * (double)nnodes * nfeat * nbins;
  return kSssFixed + kSssEntry * half + kSssCell * M + kSssListed * (half < M ? half : M) +
         (have_total ? 0.0 : kSssTotal * 0.5 * (double)n_rows);
}

inline bool level_sub_sparse(int64_t n_rows, int nnodes, int nfeat, int nbins, int64_t nnz, bool have_total) {
  if (n_rows < 1 || nnodes < 2 || (nnodes & 1) || nnodes > kSubSparseNodesMeasured || nfeat < 1 || nbins < 1 ||
      nbins > kSparseBinsMax || nnz < 0)
    return false;
  const double entries = (double)nfeat * (double)n_rows;
  if ((double)nnz < kSubSparseDensityMin * entries || (double)nnz > kSubSparseDensityMax * entries) return false;
  const double groups = (double)nnodes * nfeat, M = 0.5 * groups * nbins;
  const double combined = level_sub_sparse_cost(n_rows, nnodes, nfeat, nbins, nnz, have_total);
  const double sparse = kSssSparseFixed + kSssSparseEntry * (double)nnz + kSssSparseGroup * groups +
                        (have_total ? 0.0 : kSssSparseTotal * (double)n_rows);
  const double sub = 0.5 * entries + kSssSubFixed + kSssSubEntry * (double)nnz + kSssSubCell * M;
  return sparse >= kSubSparseOverSparse * combined && sub >= kSubSparseOverSub * combined;
}

enum class Horner {
  WAVE,   // 2048, 16 lanes: k_mexp_horner_wave, one 16-wave block per column (latency)
  LANES,  // k_mexp_horner
};
constexpr int64_t kMexpWaveMax = 4096;

inline Horner mexp_horner(int K, int lanes, int64_t ncols, const Pins& pins) {
  return K == 2048 && lanes == 16 && pins.mexp_wave && ncols <= kMexpWaveMax ? Horner::WAVE : Horner::LANES;
}

// ------------------------------------------------- multi-exponentiation
// Two device paths serve out[j] = prod_t base^k: Straus windows with per-base
// tables (xhe_multiexp) and buckets (xhe_bucketexp, bucket_dev.hpp). Both are
// planned by product counts.
//
// Straus: window bits minimising the table products nbases (2^c - 2) plus the
// gathered products ncols nterms ceil(kbits / c), with the tables (s4 words a
// row) capped at kMexpTabBytes.
constexpr int kMexpWinMax = 8;
constexpr double kMexpTabBytes = 2147483648.0;

struct MexpPlan {
  int c;
  double cost;  // products of the whole call
};

inline MexpPlan mexp_plan(int64_t nbases, int64_t ncols, int64_t nterms, int kbits, int s4) {
  MexpPlan best{1, 1e300};
  for (int c = 1; c <= kMexpWinMax; ++c) {
    if (c > 1 && (double)(nbases << c) * s4 * 4 > kMexpTabBytes) break;
    const double cost = (double)nbases * ((1 << c) - 2) + (double)ncols * nterms * ((kbits + c - 1) / c) +
                        (double)ncols * kbits;
    if (cost < best.cost) best = {c, cost};
  }
  return best;
}

inline int mexp_window(int64_t nbases, int64_t ncols, int64_t nterms, int kbits, int s4) {
  return mexp_plan(nbases, ncols, nterms, kbits, s4).c;
}

// Buckets: per column and window of c bits one product per term, one per
// (bin, tile) of the accumulation (k_hist_tile's slices and stage B, T tiles
// of the tile hist_tile chooses for ncols * nwin features) and 2 * 2^c for the
// fold:
//   cost(c) = nwin (nterms + nbins T) + nwin 2 2^c,   nwin = ceil(kbits / c),
//   nbins = (2^c - 1) * (sgn ? 2 : 1)   (<= 4094: c <= kBucketWinMax = 11)
constexpr int kBucketWinMax = 11;

inline int bucket_nbins(int c, bool sgn) { return ((1 << c) - 1) * (sgn ? 2 : 1); }

inline double bucket_cost(int64_t nterms, int64_t ncols, int kbits, bool sgn, int c) {
  const int nwin = (kbits + c - 1) / c > 1 ? (kbits + c - 1) / c : 1;
  const int nbins = bucket_nbins(c, sgn);
  const int64_t feat = ncols * nwin;
  const int tile = hist_tile(nterms, (int)(feat < (1 << 30) ? feat : (1 << 30)), nbins);
  const int64_t T = (nterms + tile - 1) / tile;
  return (double)nwin * ((double)nterms + (double)nbins * T) + (double)nwin * 2 * (1 << c);
}

inline int bucket_window(int64_t nterms, int64_t ncols, int kbits, bool sgn) {
  int best = 1;
  double best_cost = 1e300;
  for (int c = 1; c <= kBucketWinMax; ++c) {
    const double cost = bucket_cost(nterms, ncols, kbits, sgn, c);
    if (cost < best_cost) {
      best_cost = cost;
      best = c;
    }
  }
  return best;
}

// Which of the two serves a dense product of nterms bases and ncols columns,
// ninv of the bases under some negative scalar: Straus pays for ninv extra
// bases and their batch inversion (kInvProducts each: into Montgomery form,
// up and down the product tree, out again). Buckets only from
// kBucketMinTerms terms and a modelled saving of kBucketMinSaving: the
// regression steps (2048 x 15) and every small shape stay where they were.
// Measured at 2048 bits (DESIGN "Bucket multi-exponentiation",
// profiles/r25/bucketexp/): at 2048 x 15 x 60 bits (model 1.25) Straus is
// 1.86x faster; buckets are faster, beyond the spread, at 8197 x 2 (24 bits,
// model 1.98: 1.13x; 60 bits, model 1.77: 1.18x), at 100 k x 16 x 24 (model
// 2.49) 1.38x and at 1 M x 16 x 24 (model 7.6) 4.14x. The floor of 8192 terms
// stands between the first two; the saving is set just below the lowest
// modelled ratio at which buckets were measured faster. The model overstates
// the saving: per product a bucket row costs more than a gathered table row.
enum class MexpRoute {
  STRAUS,   // xhe_multiexp (the caller inverts the bases of negative terms)
  BUCKETS,  // xhe_bucketexp
};
constexpr int64_t kBucketMinTerms = 8192;  // mirrored as xfl_amd._native.BUCKET_MIN_TERMS
constexpr double kBucketMinSaving = 1.75;
constexpr int kInvProducts = 4;

inline MexpRoute multiexp_route(int64_t nterms, int64_t ncols, int kbits, int64_t ninv, int s4) {
  if (nterms < kBucketMinTerms || ncols < 1) return MexpRoute::STRAUS;
  const int kb = kbits > 1 ? kbits : 1;
  const double straus = mexp_plan(nterms + ninv, ncols, nterms, kb, s4).cost + (double)kInvProducts * ninv;
  const bool sgn = ninv > 0;
  const double buckets = (double)ncols * bucket_cost(nterms, ncols, kb, sgn, bucket_window(nterms, ncols, kb, sgn));
  return straus >= kBucketMinSaving * buckets ? MexpRoute::BUCKETS : MexpRoute::STRAUS;
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
