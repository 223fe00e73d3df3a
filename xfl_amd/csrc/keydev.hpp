// The device-visible description of a key: what a kernel knows about a key is
// the constant blob and this struct of pointers into it. Plain data, includable
// by a host compiler (keyconst.hpp derives it without the kernels).
#pragma once
#include <cstdint>

#include <hip/hip_vector_types.h>  // uint2

namespace xhe {

struct ModDev {
  const uint32_t* N;   // S W-limbs (row of S4 words)
  const uint32_t* R1;  // R mod N
  const uint32_t* R2;  // R^2 mod N
  const uint32_t* R3;  // R^3 mod N
  uint32_t n0inv;
  const uint32_t* Rpow;  // n^2 shapes: R^j mod N for j < kRpowRows, rows of S4 limbs (else null)
};

// Segment chunks of plain (non-Montgomery) residues are at most kRawChunk
// long; such a chunk's product comes back to Montgomery form by one product
// with R^(len + 1), so R^j is kept for j <= kRawChunk + 1.
constexpr int kRawChunk = 32;
constexpr int kRpowRows = kRawChunk + 2;

// All pointers are device pointers into the key blob. Limb rows are padded to
// a multiple of 4 words and 16-byte aligned.
struct KeyDev {
  int K, nw, n2w;  // key bits, 32-bit words of n and of n^2
  int priv, djn;
  const uint32_t* n_words;   // n (nw words)
  const uint32_t* n2_words;  // n^2 (n2w words)
  const uint32_t* maxpos;    // n // 3 (nw words)
  const uint32_t* minneg;    // n - n // 3 (nw words)
  const uint32_t* n_lim;     // n as MP2 limbs (raw encryption wide product)
  // ---- mod n^2 (shape MN2): public-key paths and homomorphic operations
  ModDev n2;
  const uint32_t* nR2_n2;     // n * R^2 mod n^2
  const uint32_t* tab_n2;     // [nwin][2^win][S4] h^(d*2^(win*w)) * R mod n^2 (public DJN)
  const uint32_t* ep_words;   // n mod phi(p^2) (nw words), non-DJN private obfuscation exponent
  const uint32_t* eq_words;
  int ep_bits, eq_bits, n_bits;
  // ---- mod p^2 / q^2 (shape MP2)
  ModDev p2, q2;
  ModDev p2L, q2L;            // the same moduli in the 4-lane decrypt shape (S = S4 of p2)
  ModDev p2X, q2X;            // and in the 16-lane (one DPP row) decrypt shape
  ModDev n2X;                 // n^2 in the 16-lane shape (small-batch ciphertext ops)
  const uint32_t* nR2_p2;     // n * R^2 mod p^2
  const uint32_t *nR_p2, *nR_q2;  // n * R mod P^2 (plain n m from a Montgomery product)
  // 16-lane (p2X/q2X, R' = 2^(W*80)) DJN shape on the one-lane tables: every
  // table product scales by R/R', so the start value carries C = (R'/R)^nwin:
  const uint32_t *nR2C_p2X, *nR2C_q2X;  // n * C * R'^2 mod P^2
  const uint32_t *R1C_p2X, *R1C_q2X;    // C * R' mod P^2
  const uint32_t* nR2_q2;     // n * R^2 mod q^2
  const uint32_t* nR2_p2L;    // n * R_L^2 mod p^2 / q^2 in the 4-lane (p2L) shape
  const uint32_t* nR2_q2L;
  const uint32_t* q2invR_p2;  // (q^2)^-1 * R mod p^2
  const uint32_t* q2_lim;     // q^2 (MP2 limbs)
  const uint32_t* p2x4_lim;   // 4 p^2 (MP2 limbs)
  const uint32_t* tab_p2;     // h^(d*2^bit(w)) * R mod p^2, packed rows, windows as win_digit()
  const uint32_t* tab_q2;
  int64_t tab_rs;             // words from one row of tab_p2 / tab_q2 to the next
  int win, nwin, nhi;         // nhi: the first nhi windows are win+1 bits wide (0: uniform)
  // ---- mod p / q (shape MP), decrypt
  ModDev p, q;
  const uint32_t* pm1_words;  // p - 1 (nw/2 words)
  const uint32_t* qm1_words;
  int pm1_bits, qm1_bits;
  const uint32_t* pinv_lim;   // p^-1 mod 2^(W*S) (MP limbs)
  const uint32_t* qinv_lim;
  const uint32_t* hpR;        // hp * R mod p
  const uint32_t* hqR;
  const uint32_t* qinvpR;     // (q^-1 mod p) * R mod p
  const uint32_t* q_lim;      // q (MP limbs)
  const uint32_t* p2x_lim;    // 2 p (MP limbs)
  const uint32_t* p_lim;      // p (MP limbs)
  // ---- Montgomery-digit DJN encryption (k_djn_pmd, 2048-bit keys): the
  // tables hold digit rows (pmd = 1) - words [0, K/64) the first digit e < P
  // of the row's pair (e, f), words [K/64, K/32) its log digit lhat = f y^-1
  // mod P < P (y the row's residue; pdigit_dev.hpp "Additive second digit") -
  // and MASK + ((1 - R) mod P) limbs per prime; mu_p = Q R^4 mod P and mu_q =
  // P R^4 mod Q (R = 2^(28*37), Mont<37, 28, 1> limbs; DJN keys): the factor
  // that turns a plaintext m into its log digit Q m R^2 mod P (1 + n m =
  // 1 + P (Q m); pdigit_dev.hpp "The plaintext as a logarithm"); ms_p = Q R^2
  // B mod P and ms_q = P R^2 B mod Q, B = 2^(28*4) (the same limbs; DJN keys):
  // the factor of a short plaintext +-s, s < B, whose log digit is +-s ms / B
  // by four Montgomery steps (pdigit_dev.hpp "Short plaintexts")
  int pmd;
  const uint32_t *topc_p, *topc_q;
  const uint32_t *mu_p, *mu_q;
  const uint32_t *ms_p, *ms_q;
  // ---- Montgomery digits mod n^2 (PMDX, 2048-bit keys, public or private):
  // n as 80 limbs of 27 bits (R = 2^2160), ceil(R/n) n^2 (160 limbs), R - n,
  // the digits of R^2 mod n^2 and of 1 (80 pairs each), MASK + E_i
  int ndig;
  ModDev nd;
  const uint32_t *nd_kn2, *nd_rmn, *nd_topc;
  const uint2 *nd_dw, *nd_d1;
  const uint2* nd_dwt;  // digits of R^2 R_MN2^-1 (public DJN table rows -> digits)
  int pub_nd;           // public DJN tables hold digits of n (k_djn_pub_nd)
  // ---- Montgomery digits mod P^2 over 4 lanes (PMDX, 3072/4096-bit DJN
  // private keys; k_djn_pmdx): P as K limbs of 27 bits, ceil(R/P) P^2, R - P,
  // MASK + E_i, the fold constant Q R^3 mod P (Q the other prime) and the
  // digits of R^2 R_MP2^-1 mod P^2 (the table rows' conversion constant)
  int pmdx;
  ModDev dp, dq;
  const uint32_t *x_kn2_p, *x_kn2_q, *x_rmn_p, *x_rmn_q, *x_topc_p, *x_topc_q, *x_fold_p, *x_fold_q;
  const uint2 *x_dwt_p, *x_dwt_q;
  // the same digits for the decrypt of every 3072/4096-bit private key
  // (k_dec_pmdx_*): the digits of R^2 mod P^2 and hp R mod P (27-bit limbs)
  int pmdx_dec;
  const uint2 *x_dw_p, *x_dw_q;
  const uint32_t *x_hpR_p, *x_hpR_q;
  // ---- one-wave decrypt exponentiation (k_dec_wave, 2048-bit keys): the
  // full Montgomery inverse -P^-2 mod R of the MP2 shape (R = 2^(28*74))
  const uint32_t *p2_nprime, *q2_nprime;
  // ---- RNS small-batch decrypt (k_dec_rns, rns_dev.hpp; 2048-bit private
  // keys): the bases' constant block and one block per prime (null: off)
  const uint32_t *rns, *rns_p, *rns_q;
  // ---- one-block Horner of the mat-vec mod n^2 (k_mexp_horner_wave, 2048-bit
  // keys): n^2 in 154 limbs of 27 bits (R_w = 2^4158), -n^-2 mod R_w and
  // C = R_w^2 R_X^-1 mod n^2 (R_X = 2^(27*160): the 16-lane shape's R)
  const uint32_t *n2w_N, *n2w_np, *n2w_C, *n2w_R2;  // (R2: R_w^2 mod n^2, k_mulmod_wave)
  // ---- Barrett reduction mod n^2 (k_add_barrett, 2048-bit keys):
  // floor(2^(27*304) / n^2) as 153 limbs of 27 bits
  const uint32_t* n2_mu;
  // ---- online encryption on a precomputed obfuscator (k_enc_obf,
  // enc_obf_dev.hpp; every key): n itself as a Montgomery modulus in the
  // 4-lane (p2L) limb shape, and n^2 as 2 S plain limbs of that shape
  ModDev nL;
  const uint32_t* n2_limL;
};

}  // namespace xhe
