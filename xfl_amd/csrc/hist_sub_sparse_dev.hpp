// Histogram subtraction on the sparse level-wise histogram
// (xhe_hist_level_sub_sparse): of every pair of level slots only the child
// with fewer rows is built (k_sub_pick), and of that child only the entries
// outside the features' zero bins are multiplied (the level-sparse order, tile,
// fold and out stages on the remapped node ids, with the npairs pairs as the
// nodes: M = npairs * nfeat * nbins built cells, G = npairs * nfeat groups).
// With z the zero bin of group g = (pair v, feature f), T the built child's
// product and Q_g the product of g's folded rows other than z (the hidden bin
// included):
//   built   [b != z] the folded product            [z] T / Q_g
//   sibling [b != z] parent / built                [z] parent[z] Q_g / T
// A built cell without an entry is the one and its sibling parent mod n^2:
// nothing to invert, so most cells of a sparse level never enter the chains.
//
//   mark    k_sss_mark, a thread per cell: the cells with an entry outside the
//           zero bin (count > 0, b != z) are compacted into one list - a
//           ballot per wave, one atomic per block, in no particular order. The
//           list's length stays on the device; the host sizes every grid by
//           its bound min(M, nnz_bound) + G + npairs (paths::sub_sparse_list).
//   fill    k_sss_fill, a lane group per cell that is neither listed nor a
//           zero bin: the one and parent mod n^2 (one product), the counts.
//           Independent of the inversion: it runs ahead of it.
//   chains  One batch inversion for everything that is inverted. Entry e of
//           the inversion list is cell cells[e] for e < ncell, then Q_g for the
//           G groups, then T for the npairs pairs; the three kinds differ only
//           in where the operand's words lie (sss_src). k_sss_fwd and
//           k_sss_bwd are k_sib_fwd's and k_sib_bwd's chains (hist_sub_dev.hpp:
//           unreduced states below 2 n^2, the R powers cancelled by one Rpow
//           row per chunk, prefixes parked limb-major) indexed through the
//           list: chunk k walks the entries k, k + nchunks, ... below the
//           list's length, which may leave a chunk short or empty (its total is
//           then the one). Backwards, x = t s_u / R = c_u^-1 R takes one more
//           product with a row of words - the parent row for a cell, which
//           gives the sibling as in k_sib_bwd, the one for a Q or T entry,
//           which gives the plain inverse - so both kinds share every product
//           and differ in the row they store to: `out`, or the G + npairs
//           inverse rows of a small workspace.
//   zero    k_sss_zero, a lane group per group behind the inversion: both
//           children's zero bin from T, Q_g and the two inverses (two and three
//           products), both counts.
#pragma once
#include "hist_level_sparse_dev.hpp"
#include "hist_sub_dev.hpp"

namespace xhe {

// The inversion list of one call. Rows of words are PW apart.
struct SssList {
  const int32_t* cells;   // the listed cells' ids (below M), cap of them allocated
  const int32_t* ncell;   // how many there are
  int64_t cap, G;
  int npairs;
  int total_by_node;      // total holds a row per level slot (the caller's), not one per pair
  const uint32_t* built;  // [M] the built cells as words (k_lsp_out)
  const uint32_t* qw;     // [G] Q_g as words
  const uint32_t* total;  // the built children's products T
  const uint32_t* pick;   // [npairs] k_sub_pick's
};

XHE_DEV int64_t sss_ncell(const SssList& L) {
  const int64_t n = *L.ncell;
  return n < L.cap ? n : L.cap;
}

// T of pair v
template <int PW>
XHE_DEV const uint32_t* sss_total(const SssList& L, int64_t v) {
  return L.total + (size_t)(L.total_by_node ? 2 * v + (L.pick[v] & kSubBuiltRight) : v) * PW;
}

// The words of entry e < nc + G + npairs; cell: its id for a cell entry, -1 otherwise
template <int PW>
XHE_DEV const uint32_t* sss_src(const SssList& L, int64_t nc, int64_t e, int64_t& cell) {
  if (e < nc) {
    cell = L.cells[e];
    return L.built + (size_t)cell * PW;
  }
  cell = -1;
  const int64_t q = e - nc;
  return q < L.G ? L.qw + (size_t)q * PW : sss_total<PW>(L, q - L.G);
}

// Thread i: cell i = (g, b) joins the list when hcnt[g][b] > 0 and b is not g's
// zero bin (hcnt: [G][nbins + 1], k_lsp_tile's). *ncell zeroed before the
// launch. one: a row of pw words that the first block sets to 1.
__global__ void __launch_bounds__(256) k_sss_mark(const int32_t* __restrict__ hcnt, const uint16_t* __restrict__ zero_bin,
                                                  int nfeat, int nbins, int64_t M, int64_t cap,
                                                  int32_t* __restrict__ cells, int32_t* __restrict__ ncell,
                                                  uint32_t* __restrict__ one, int pw) {
  __shared__ int s_w[4];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  if (blockIdx.x == 0)
    for (int j = tid; j < pw; j += 256) one[j] = j == 0 ? 1u : 0u;
  bool listed = false;
  if (i < M) {
    const int64_t g = i / nbins;
    const int b = (int)(i - g * nbins);
    listed = (uint32_t)b != zero_bin[g % nfeat] && hcnt[g * (nbins + 1) + b] > 0;
  }
  const unsigned long long m = __ballot(listed);
  if (lane == 0) s_w[w] = __popcll(m);
  __syncthreads();
  if (tid == 0) {
    const int n = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    s_base = n ? atomicAdd(ncell, n) : 0;
  }
  __syncthreads();
  if (!listed) return;
  int64_t at = (int64_t)s_base + __popcll(m & ((1ull << lane) - 1ull));
  for (int j = 0; j < w; ++j) at += s_w[j];
  if (at < cap) cells[at] = (int32_t)i;  // (ncell <= the entries outside the zero bins <= cap unless the flag is up)
}

// Lane group i: cell i unless it is listed or its group's zero bin. The built
// child's row is 1, the sibling's parent mod n^2 (1 for an empty pair), the
// counts 0 and parent_cnt (0). Nothing is written with the flag raised.
template <class MN2, int PW>
__global__ void __launch_bounds__(256, hist_waves<MN2>())
    k_sss_fill(KeyDev key, const uint32_t* __restrict__ Nn2, const int32_t* __restrict__ hcnt,
               const int32_t* __restrict__ flag, const uint16_t* __restrict__ zero_bin, int nfeat, int nbins, int64_t M,
               int64_t FB, const uint32_t* __restrict__ parent, const int32_t* __restrict__ parent_cnt,
               const uint32_t* __restrict__ pick, uint32_t* __restrict__ out, int32_t* __restrict__ cnt) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  if (i >= M || *flag) return;
  const int64_t g = i / nbins;
  const int b = (int)(i - g * nbins);
  if ((uint32_t)b == zero_bin[g % nfeat] || hcnt[g * (nbins + 1) + b] > 0) return;
  const int lg = MN2::G::g();
  const int64_t v = i / FB, col = i - v * FB;
  const uint32_t pk = pick[v];
  const int64_t ob = (2 * v + (pk & kSubBuiltRight)) * FB + col, os = (2 * v + 1 - (pk & kSubBuiltRight)) * FB + col;
  MN2 Mo;
  Mo.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t x[MN2::L];
  if (pk & kSubEmpty) {  // (uniform in the lane group)
#pragma unroll
    for (int j = 0; j < MN2::L; ++j) x[j] = (lg == 0 && j == 0) ? 1u : 0u;
  } else {
    Mo.load_row(x, n2dev<MN2>(key).Rpow + (size_t)MN2::S4);
    Mo.mul(x, ARowPacked<MN2::W, PW>{parent + (size_t)i * PW});  // R parent / R
    Mo.reduce_once(x);
  }
  Mo.store_words(x, out + (size_t)os * PW, PW);
  for (int w = lg; w < PW; w += MN2::TPI) out[(size_t)ob * PW + w] = w == 0 ? 1u : 0u;
  if (cnt && lg == 0) {
    cnt[ob] = 0;
    cnt[os] = (pk & kSubEmpty) ? 0 : parent_cnt[i];
  }
}

// Lane group k: the exclusive prefixes of chunk k's entries into pre ([S4][
// stride], column = the entry), its total as words into tot[k].
template <class MN2, int PW>
__global__ void __launch_bounds__(256, sib_fwd_waves<MN2>())
    k_sss_fwd(KeyDev key, const uint32_t* __restrict__ Nn2, SssList L, int64_t nchunks, int stride,
              uint32_t* __restrict__ pre, uint32_t* __restrict__ tot) {
  const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  if (k >= nchunks) return;
  const int64_t nc = sss_ncell(L);
  const int len = sib_len(k, nchunks, nc + L.G + L.npairs);
  MN2 Mo;
  Mo.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  const uint32_t* rp = n2dev<MN2>(key).Rpow;
  Mo.load_row(b, rp + (size_t)MN2::S4);
#pragma unroll 1
  for (int u = 0; u < len; ++u) {
    const int64_t e = k + (int64_t)u * nchunks;
    int64_t cell;
    const uint32_t* cw = sss_src<PW>(L, nc, e, cell);
    Mo.store_strided(b, pre + e, stride);
    Mo.mul(b, ARowPacked<MN2::W, PW>{cw});
    __builtin_amdgcn_sched_barrier(0);
  }
  Mo.mul(b, ARow{rp + (size_t)len * MN2::S4});
  Mo.reduce_once(b);
  Mo.store_words(b, tot + (size_t)k * PW, PW);
}

// Lane group k, backwards over chunk k with inv[k] = the inverse of its total.
// A cell entry writes out and cnt of both children (FB = nfeat * nbins; parent_cnt
// and cnt null together); a Q or T entry stores its inverse to sinv[e - ncell]
// (G + npairs rows). one: k_sss_mark's row.
template <class MN2, int PW>
__global__ void __launch_bounds__(256, sib_bwd_waves<MN2>())
    k_sss_bwd(KeyDev key, const uint32_t* __restrict__ Nn2, SssList L, const int32_t* __restrict__ hcnt, int nbins,
              const uint32_t* __restrict__ parent, const int32_t* __restrict__ parent_cnt, int64_t FB, int64_t nchunks,
              int stride, const uint32_t* pre, const uint32_t* __restrict__ inv, const uint32_t* __restrict__ one,
              uint32_t* __restrict__ sinv, uint32_t* __restrict__ out, int32_t* __restrict__ cnt) {
  const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  if (k >= nchunks) return;
  const int64_t nc = sss_ncell(L);
  const int len = sib_len(k, nchunks, nc + L.G + L.npairs);
  if (len == 0) return;
  const int g = MN2::G::g();
  MN2 Mo;
  Mo.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t t[MN2::L], x[MN2::L];
  Mo.load_words(t, inv + (size_t)k * PW, PW);
  Mo.mul(t, ARow{n2dev<MN2>(key).Rpow + (size_t)(len + 1) * MN2::S4});
#pragma unroll 1
  for (int u = len - 1; u >= 0; --u) {
    const int64_t e = k + (int64_t)u * nchunks;
    int64_t i;
    const uint32_t* cw = sss_src<PW>(L, nc, e, i);
    const uint32_t* second = one;
    uint32_t* dst = sinv + (size_t)(e - nc) * PW;
    int64_t ob = 0, os = 0;
    if (i >= 0) {
      const int64_t v = i / FB, col = i - v * FB;
      const uint32_t right = L.pick[v] & kSubBuiltRight;
      ob = (2 * v + right) * FB + col;
      os = (2 * v + 1 - right) * FB + col;
      second = parent + (size_t)i * PW;
      dst = out + (size_t)os * PW;
    }
#pragma unroll
    for (int j = 0; j < MN2::L; ++j) x[j] = t[j];
    Mo.mul(x, AStrided{pre + e, stride});  // c^-1 R
    __builtin_amdgcn_sched_barrier(0);
    Mo.mul(x, ARowPacked<MN2::W, PW>{second});  // parent / c, or c^-1
    Mo.reduce_once(x);
    Mo.store_words(x, dst, PW);
    if (i >= 0) {
      // (the built rows are k_lsp_out's: below n^2)
      for (int w = g; w < PW; w += MN2::TPI) out[(size_t)ob * PW + w] = cw[w];
      if (cnt && g == 0) {
        const int64_t gr = i / nbins;
        const int32_t bc = hcnt[gr * (nbins + 1) + (i - gr * nbins)];
        cnt[ob] = bc;
        cnt[os] = parent_cnt[i] - bc;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (u > 0) Mo.mul(t, ARowPacked<MN2::W, PW>{cw});
  }
}

// Lane group g = v * nfeat + f with a zero bin z: the built child's row at (f,
// z) is T Q_g^-1, the sibling's parent[v][f][z] Q_g T^-1 (sinv: Q_g^-1 at g,
// T^-1 at G + v), the counts node_cnt[built] - nzsum[g] and the rest of
// parent_cnt. An empty pair stores 1 and 0.
template <class MN2, int PW>
__global__ void __launch_bounds__(256, hist_waves<MN2>())
    k_sss_zero(KeyDev key, const uint32_t* __restrict__ Nn2, SssList L, const uint32_t* __restrict__ sinv, int nfeat,
               int nbins, const uint16_t* __restrict__ zero_bin, const int32_t* __restrict__ node_cnt,
               const int32_t* __restrict__ nzsum, const uint32_t* __restrict__ parent,
               const int32_t* __restrict__ parent_cnt, uint32_t* __restrict__ out, int32_t* __restrict__ cnt) {
  const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  if (g >= L.G) return;
  const int64_t v = g / nfeat, f = g - v * nfeat;
  const uint32_t z = zero_bin[f];
  if (z >= (uint32_t)nbins) return;
  const int lg = MN2::G::g();
  const uint32_t pk = L.pick[v], right = pk & kSubBuiltRight;
  const int64_t FB = (int64_t)nfeat * nbins, col = f * nbins + z;
  const int64_t ob = (2 * v + right) * FB + col, os = (2 * v + 1 - right) * FB + col;
  const uint32_t* rp = n2dev<MN2>(key).Rpow;
  const uint32_t* tw = sss_total<PW>(L, v);
  MN2 Mo;
  Mo.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L], x[MN2::L];
  Mo.load_words(b, sinv + (size_t)g * PW, PW);
  Mo.mul(b, ARowPacked<MN2::W, PW>{tw});             // Q^-1 T / R
  Mo.mul(b, ARow{rp + (size_t)2 * MN2::S4});         // times R^2 / R
  Mo.reduce_once(b);
  Mo.load_words(x, sinv + (size_t)(L.G + v) * PW, PW);
  Mo.mul(x, ARowPacked<MN2::W, PW>{L.qw + (size_t)g * PW});                    // T^-1 Q / R
  Mo.mul(x, ARowPacked<MN2::W, PW>{parent + (size_t)(v * FB + col) * PW});     // T^-1 Q parent / R^2
  Mo.mul(x, ARow{rp + (size_t)3 * MN2::S4});                                   // times R^3 / R
  Mo.reduce_once(x);
  if (pk & kSubEmpty) {
#pragma unroll
    for (int j = 0; j < MN2::L; ++j) b[j] = x[j] = (lg == 0 && j == 0) ? 1u : 0u;
  }
  Mo.store_words(b, out + (size_t)ob * PW, PW);
  Mo.store_words(x, out + (size_t)os * PW, PW);
  if (cnt && lg == 0) {
    const int32_t bc = node_cnt[2 * v + right] - nzsum[g];
    cnt[ob] = (pk & kSubEmpty) ? 0 : bc;
    cnt[os] = (pk & kSubEmpty) ? 0 : parent_cnt[v * FB + col] - bc;
  }
}

}  // namespace xhe
