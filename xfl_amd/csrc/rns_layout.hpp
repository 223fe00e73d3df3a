// Layout of the RNS small-batch decrypt's constant blocks (k_dec_rns,
// rns_dev.hpp), shared by the kernel and by the host derivation
// (keyconst.hpp rnsh).
#pragma once
#include <cstdint>

namespace xhe {
namespace rns {

constexpr int RK = 74;      // moduli per base
constexpr int RKP = 76;     // limbs of M_i, M at the exit (28 bits)
constexpr int RT = 80;      // extension terms, zero-padded (two halves of 40)
constexpr int HT = RT / 2;
constexpr int NT = 384;     // threads per residue
constexpr int NSLOT = 160;  // constant slots: B channels 0..79, B' channels 80..159 (r: 154)
constexpr int RCH = 74;     // the B' waves' channel number of r
constexpr uint32_t LMASK = (1u << 28) - 1u;

// constant blocks (words): shared by every key (the bases), then per prime;
// per-slot arrays of NSLOT
constexpr int S_M = 0, S_MU = 160, S_T32 = 320, S_B = 480, S_BS = 640, S_C = 800, S_CS = 960, S_D = 1120;
constexpr int S_ROWS = 1280;                // [RT][NSLOT]: B: |M'_j|_(m_i); B': |M_i|_(m'_j); r: |M_i|_(2^32)
constexpr int S_MPOS = S_ROWS + RT * NSLOT; // [RK][RKP] 28-bit limbs of M_i = M / m_i
constexpr int S_MFULL = S_MPOS + RK * RKP;  // [RKP] limbs of M
constexpr int S_M2RINV = S_MFULL + RKP;     // M'^-1 mod 2^32
constexpr int S_WORDS = S_M2RINV + 4;
// per prime: P_A (B: |-N^-1 M_i^-1|; B': |N M^-1|; r: N mod 2^32) and its
// Shoup companion, P_A2 (B': |N M^-1 M'_j^-1|) and companion, M^3 mod N per
// channel, then the exponent P - 1 as a window schedule: P_NS entries, [0] =
// the start value's table index, then (squarings << 8) | (t + 1) (t + 1 = 0:
// no product)
constexpr int P_A = 0, P_AS = 160, P_A2 = 320, P_A2S = 480, P_M3 = 640, P_NS = 800, P_SCHED = 804;
constexpr int P_SCHED_MAX = 1280;
constexpr int P_WORDS = P_SCHED + P_SCHED_MAX + 4;

}  // namespace rns
}  // namespace xhe
