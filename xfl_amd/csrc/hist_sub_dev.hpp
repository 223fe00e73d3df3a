// Histogram subtraction for the level-wise histogram (xhe_hist_level_sub):
// of the two children 2v, 2v + 1 of parent slot v only the one with fewer rows
// is multiplied from its rows; its sibling is parent / built mod n^2 per
// (feature, bin).
//
//   pick    k_sub_pick, one launch, no host read: from k_level_count's counts
//           of the level's slots every thread decides its row's pair again
//           (two loads) and writes the remapped node id - the pair id v for a
//           row of the built child, 0xFFFF for every other row; the first
//           npairs threads also write pick[v]: bit 0 = the built child is the
//           right one (fewer rows; a tie builds the left), bit 1 = the pair
//           holds no row at all. The level's order, tile and fold stages then
//           run unchanged on the remapped ids with npairs nodes and leave the
//           M = npairs * nfeat * nbins built rows as words in a workspace, in
//           xhe_hist_level's layout.
//   sibling Montgomery's batch inversion fused with the parent product. Lane
//           group k of nchunks walks the rows k, k + nchunks, ... (at most C =
//           paths::sib_chunk of them, interleaved as the sum's chunks are, so
//           that a wave's groups touch neighbouring rows at every step).
//           The built words are the operand of every product, unpacked where
//           they are used (any value the words hold); the powers of R that
//           leaves behind are carried in the chain and cancelled by one row
//           of Rpow per chunk, as the cumulative sum's raw level does:
//     k_sib_fwd  s_0 = R, s_(u+1) = s_u c_u / R: s_u = P_u R^(1-u), P_u = c_0
//                .. c_(u-1) the exclusive prefix, parked in column i of pre
//                ([S4][M], limb-major). The chunk total s_L R^L / R = P_L
//                leaves as words for invert_impl (the product tree and the one
//                host inverse of its root).
//     k_sib_bwd  t_L = P_L^-1 R^(L+1) / R = P_L^-1 R^L, and for u = L-1 .. 0
//                  x = t_(u+1) s_u / R         = c_u^-1 R          (the row's inverse)
//                  x = x parent_u / R          = parent_u / c_u    (stored, < n^2)
//                  t_u = t_(u+1) c_u / R       = P_u^-1 R^u
//                One product forward and three backward per row; the parent
//                row is read once and every output row written once: the
//                sibling's words, the built child's (copied from the
//                workspace) and both counts. An empty pair stores 1 and 0.
//           The chain states are not reduced: they stay below 2 n^2, which a
//           product accepts on either side (R is at least 2^8 times 2^(32 n2w)
//           in every n^2 shape).
#pragma once
#include "hist_level_dev.hpp"

namespace xhe {

static_assert(paths::kSibChunkMax + 1 < kRpowRows, "a chunk's exit rows: R^L and R^(L+1) for L <= kSibChunkMax");

constexpr uint32_t kSubBuiltRight = 1, kSubEmpty = 2;

// node_cnt: rows per level slot (k_level_count). remap[r] and pick[v] as above.
__global__ void __launch_bounds__(256) k_sub_pick(const uint16_t* __restrict__ node, int64_t n_rows, int nnodes,
                                                  const int32_t* __restrict__ node_cnt, uint16_t* __restrict__ remap,
                                                  uint32_t* __restrict__ pick) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nnodes / 2) {
    const int32_t l = node_cnt[2 * i], r = node_cnt[2 * i + 1];
    pick[i] = (r < l ? kSubBuiltRight : 0u) | (l + r == 0 ? kSubEmpty : 0u);
  }
  if (i >= n_rows) return;
  const uint32_t v = node[i];
  uint16_t to = 0xFFFF;
  if (v < (uint32_t)nnodes) {
    const uint32_t right = node_cnt[v | 1u] < node_cnt[v & ~1u] ? 1u : 0u;
    if ((v & 1u) == right) to = (uint16_t)(v >> 1);
  }
  remap[i] = to;
}

// Blocks per CU the sibling kernels are compiled for. The backward walk keeps
// two residues live (t and the row's x) next to the product's accumulators: at
// 2 blocks it spilled 80 VGPRs with 38 limbs a lane (2048 bits) and 97 with 40
// (8192 bits), the forward walk 14 with 40; at 1 block nothing spills.
template <class MN2>
constexpr int sib_fwd_waves() {
  return MN2::L > 38 ? 1 : 2;
}
template <class MN2>
constexpr int sib_bwd_waves() {
  return MN2::L > 32 ? 1 : 2;
}

// Rows of chunk k: k, k + nchunks, ... below M
XHE_DEV int sib_len(int64_t k, int64_t nchunks, int64_t M) { return (int)((M - k + nchunks - 1) / nchunks); }

// Lane group k: the chunk's exclusive prefixes into pre ([S4][M]), its total
// as words into tot[k].
template <class MN2, int PW>
__global__ void __launch_bounds__(256, sib_fwd_waves<MN2>())
    k_sib_fwd(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ built, int64_t M,
              int64_t nchunks, uint32_t* __restrict__ pre, uint32_t* __restrict__ tot) {
  const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  if (k >= nchunks) return;
  const int len = sib_len(k, nchunks, M);
  MN2 Mo;
  Mo.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t b[MN2::L];
  const uint32_t* rp = n2dev<MN2>(key).Rpow;
  Mo.load_row(b, rp + (size_t)MN2::S4);
#pragma unroll 1
  for (int u = 0; u < len; ++u) {
    const int64_t i = k + (int64_t)u * nchunks;
    Mo.store_strided(b, pre + i, (int)M);
    Mo.mul(b, ARowPacked<MN2::W, PW>{built + (size_t)i * PW});
    __builtin_amdgcn_sched_barrier(0);
  }
  Mo.mul(b, ARow{rp + (size_t)len * MN2::S4});
  Mo.reduce_once(b);
  Mo.store_words(b, tot + (size_t)k * PW, PW);
}

// Lane group k, backwards over its chunk with inv[k] = the inverse of its
// total (words): out and cnt of both children of every row's pair. FB = nfeat
// * nbins; built_cnt, parent_cnt, cnt: null together.
template <class MN2, int PW>
__global__ void __launch_bounds__(256, sib_bwd_waves<MN2>())
    k_sib_bwd(KeyDev key, const uint32_t* __restrict__ Nn2, const uint32_t* __restrict__ built,
              const int32_t* __restrict__ built_cnt, const uint32_t* __restrict__ parent,
              const int32_t* __restrict__ parent_cnt, const uint32_t* __restrict__ pick, int64_t M, int64_t FB,
              int64_t nchunks, const uint32_t* pre, const uint32_t* __restrict__ inv, uint32_t* __restrict__ out,
              int32_t* __restrict__ cnt) {
  const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MN2::TPI;
  if (k >= nchunks) return;
  const int len = sib_len(k, nchunks, M);
  const int g = MN2::G::g();
  MN2 Mo;
  Mo.init(Nn2, n2dev<MN2>(key).n0inv);
  uint32_t t[MN2::L], x[MN2::L];
  Mo.load_words(t, inv + (size_t)k * PW, PW);
  Mo.mul(t, ARow{n2dev<MN2>(key).Rpow + (size_t)(len + 1) * MN2::S4});
#pragma unroll 1
  for (int u = len - 1; u >= 0; --u) {
    const int64_t i = k + (int64_t)u * nchunks;
    const int64_t v = i / FB, col = i - v * FB;
    const uint32_t pk = pick[v];
    const int64_t ob = ((2 * v + (pk & kSubBuiltRight)) * FB + col), os = ((2 * v + 1 - (pk & kSubBuiltRight)) * FB + col);
    const uint32_t* bw = built + (size_t)i * PW;
#pragma unroll
    for (int j = 0; j < MN2::L; ++j) x[j] = t[j];
    Mo.mul(x, AStrided{pre + i, (int)M});
    __builtin_amdgcn_sched_barrier(0);
    Mo.mul(x, ARowPacked<MN2::W, PW>{parent + (size_t)i * PW});
    Mo.reduce_once(x);
    if (pk & kSubEmpty) {
#pragma unroll
      for (int j = 0; j < MN2::L; ++j) x[j] = (g == 0 && j == 0) ? 1u : 0u;
    }
    Mo.store_words(x, out + (size_t)os * PW, PW);
    // (the built rows are k_level_fold's: below n^2, and 1 for an empty pair)
    for (int w = g; w < PW; w += MN2::TPI) out[(size_t)ob * PW + w] = bw[w];
    if (cnt && g == 0) {
      const int32_t bc = built_cnt[i];
      cnt[ob] = bc;
      cnt[os] = (pk & kSubEmpty) ? 0 : parent_cnt[i] - bc;
    }
    __builtin_amdgcn_sched_barrier(0);
    if (u > 0) Mo.mul(t, ARowPacked<MN2::W, PW>{bw});
  }
}

}  // namespace xhe
