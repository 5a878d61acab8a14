// K5 on the 16-bit matrix cores at f32 accuracy: the per-expert variance term.
//
// Reference: the same contraction as trigemm.hip's K5 -- for every expert k,
// fvar[k][n] += sum_m' (L_k^T A)[m'][n]^2 with L_k = band_part(q_sqrt[k], -1, 0)
// (GPflow base_conditional, reached from MixtureGPs/models.py:141-143).
//
// Images (frag_image.hpp; the products and the main loops: x6_mainloop.hpp).  Read: Lfr,
// the A-operand image of L_k^T per expert (images.hip), and Afr, the B-operand image of
// A (K4, trsm_stats.hip); split-bf16 (x6, or its first 2 / 1 planes), split-f16 scaled by
// the bounds in the image trailers, or split-f16 with the e4m3 cross-term plane (f16x8).
// Written: part[k][row tile][n], the sums of C_k^2 over a row tile's 128 rows (folded
// with K4's stats by mgp_launch_cond_finalize); training (f16c) also C_k = L_k^T A per
// expert as a split-f16 B-layout image.
//
// K5x6 kernel: one 256-thread workgroup per item (expert k, row tile t of 128
// rows m', column tile of 256 n).  Wave w owns all 128 rows x 64 columns
// (4 x 2 accumulators of 32x32).  Per k-step (16 rows of m): the workgroup
// stages the 12 KiB of L fragments of its 4 row sub-tiles in LDS (double
// buffered, one barrier per k-step); each wave loads its 6 A fragments (6 KiB)
// straight from global into registers one k-step ahead; 48 MFMAs per wave.
// The triangle is exploited at row-tile granularity (k-steps start at 128 t);
// the zero blocks inside the diagonal tile come from Lfr's zero fill.
// The split-f16 kernels (expert_cond16_*) run the same items on 16x16x32 MFMAs, below.
#include "mgp_common.hpp"
#include "frag_image.hpp"
#include "x6_mainloop.hpp"

namespace mgp {

// Item b -> (row tile t heavy-first, column tile tn, expert k); the K experts of
// a column tile are 8 block ids apart (one XCD) when nTn % 8 == 0.
// TN_OUTER: per XCD, one column tile at a time with all its row tiles (heavy first)
// and experts, so A's column slab is fetched about once instead of once per row tile
// (the 32x32x16 C-writing K5 of round 2: 1.60 -> 1.51 ms; without the C writes the
// row-tile-outer order was faster, 1.33 vs 1.36 ms).  The 16x16x32 kernels use the
// row-tile-outer order for both (MGP_K5C_TN_OUTER).
template <bool TN_OUTER = false>
__device__ __forceinline__ void x6_item(int b, int nTn, int K, int& t, int& tn, int& k, int grid = -1) {
  if (TN_OUTER && nTn % 8 == 0) {
    const int nT = (grid < 0 ? (int)gridDim.x : grid) / (nTn * K);
    const int x = b & 7, j = b >> 3;
    const int per_g = nT * K;
    t = (j % per_g) / K;
    tn = (j / per_g) * 8 + x;
    k = j % K;
    return;
  }
#ifndef MGP_K5_GROUP
#define MGP_K5_GROUP 4
#endif
  // MGP_K5_GROUP = G > 0 (the default, 4): per XCD, groups of G column tiles, row tiles in
  // the middle (group outer, then t, then the group's tiles x experts), so that a group's A
  // slabs are re-read per row tile from L2 / MALL instead of re-streamed from HBM: K5 pair
  // 4.31 -> 3.71 GB fetched per launch, ELBO step 3.347-3.353 -> 3.322-3.332 ms, training
  // 14.52-14.58 -> 14.49-14.51 ms (profiles/r06zc_*, r06zd_*; G = 2 slower, 8 between).
  // Items are unchanged, so the results are bit-identical; at c4's per-rank N (one group per
  // XCD) the order is the row-tile-outer one.
  if (MGP_K5_GROUP > 0 && nTn % 8 == 0 && (nTn / 8) % MGP_K5_GROUP == 0) {
    constexpr int G = MGP_K5_GROUP > 0 ? MGP_K5_GROUP : 1;
    const int nT = (grid < 0 ? (int)gridDim.x : grid) / (nTn * K);
    const int x = b & 7, j = b >> 3;
    const int g = j / (nT * G * K);
    t = (j / (G * K)) % nT;
    const int i = (j / K) % G;
    k = j % K;
    tn = (g * G + i) * 8 + x;
    return;
  }
  if (nTn % 8 == 0) {
    const int x = b & 7, j = b >> 3;
    const int per_t = (nTn / 8) * K;
    t = j / per_t;
    const int rem = j % per_t;
    tn = (rem / K) * 8 + x;
    k = rem % K;
  } else {
    const int per_t = nTn * K;
    t = b / per_t;
    tn = (b % per_t) / K;
    k = b % K;
  }
}

// ------------------------------------------------------------------ K5 (x6)
// F16: split-f16 images (NPL = 2) scaled by 2^img_exp(*a_bound), 2^img_exp(*l_bound).
// X8: their hi planes on f16 MFMA and cross terms on e4m3 MFMA (mfma_f8x).
template <int NPL, bool F16 = false, bool X8 = false>
__global__ __launch_bounds__(256, 2) void expert_cond_x6_kernel(const bf16x8* __restrict__ Afr,
                                                                const bf16x8* __restrict__ Lfr,
                                                                uint32_t afr_bytes, uint32_t lfr_bytes,
                                                                int nmk, int nmb, int nTn, int K,
                                                                int64_t N, float* __restrict__ part,
                                                                int64_t ldp, const float* __restrict__ a_bound,
                                                                const float* __restrict__ l_bound) {
  __shared__ bf16x8 sL[2][4 * 3 * 64];  // 2 x 12 KiB: [row sub-tile][plane][lane]
  int t, tn, k;
  x6_item(blockIdx.x, nTn, K, t, tn, k);
  const int nTp = nmb / 4;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  floatx16 acc[4][2];
  x6_mainloop<1, 2, NPL, F16, X8>(acc, sL, img_rsrc(Lfr, lfr_bytes), (uint32_t)(((int64_t)k * nmb + 4 * t) * nmk) * 3u * kFragBytes,
              img_rsrc(Afr, afr_bytes), (uint32_t)((8 * tn + 2 * w) * nmk) * 3u * kFragBytes, 8 * t, nmk, nmk);

  // sum over the 128 rows of C^2 per column: 4 sub-tiles x 16 registers, then the lane halves
  const int64_t nbase = (int64_t)tn * kX6BN + 64 * w + (lane & 31);
  float* dst = part + ((int64_t)k * nTp + t) * ldp;
  float unscale = 1.f;
  if constexpr (F16) unscale = ldexpf(1.f, -2 * (img_exp(*a_bound) + img_exp(*l_bound)));
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) s = fmaf(acc[i][c][e], acc[i][c][e], s);
    s += __shfl_xor(s, 32, 64);
    if constexpr (F16) s *= unscale;
    const int64_t n = nbase + 32 * c;
    if (lane < 32 && n < N) dst[n] = s;
  }
}

// ------------------------------------------------------------------ K5 (split-f16) on 16x16x32 MFMAs
// The same contraction, items and split-f16 images as expert_cond_x6_kernel<2, true>,
// on v_mfma_f32_16x16x32_f16 (16 cycles per 16x16x32 block: the same cycles per flop
// as 32x32x16; the chip can hold a different clock per shape under load,
// MI355X_MICROARCH.md, DVFS give-back item 7).  No new image format: one k-step PAIR
// (32 deep) of the existing fragments is one MFMA k-step; lane l (i = l % 16,
// q = l / 16) takes the 16 bytes of fragment k-step 2 ks + q / 2 at lane position
// 16 (row block % 2) + i + 32 (q % 2) -- its 8 elements are 8 of the 32 m of the pair,
// the same 8 for the A operand (L_k^T, rows m') and the B operand (A, columns n), so
// the contraction is unchanged (x6_mainloop16).  Wave w: 128 rows x 64 columns =
// 8 x 4 blocks of 16 x 16; 96 MFMAs per wave and pair.
// COUT (training): C_k = L_k^T A is also written as a split-f16 B-layout image per expert,
// (the B-layout of the images K4 writes); a fragment's lane position takes
// 8 rows from two lanes of the 16x16 accumulator layout (one exchange across the lane halves).
// One item (workgroup index b of a launch of `grid` items) of the split-f16 K5.
// C_k images (training) with non-temporal stores (MGP_C_NT)
#ifndef MGP_C_NT
#define MGP_C_NT 1
#endif
constexpr bool kCntStores = MGP_C_NT;
// C-writing K5 (training) in the column-tile-outer item order (x6_item TN_OUTER): measured
// against the forward's row-tile-outer order on the 16x16x32 kernel, training step 14.18-14.22
// vs 14.11-14.18 ms (profiles/r06o_train_ab.log) -- so the row-tile-outer order (0) is kept
#ifndef MGP_K5C_TN_OUTER
#define MGP_K5C_TN_OUTER 0
#endif
constexpr bool kK5cTnOuter = MGP_K5C_TN_OUTER;
#ifndef MGP_K5_TN_OUTER
#define MGP_K5_TN_OUTER 0   // the forward K5's item order (0: row tile outer)
#endif
constexpr bool kK5TnOuter = MGP_K5_TN_OUTER;
template <bool COUT>
__device__ __forceinline__ void expert_cond16_item(bf16x8 (*sL)[4 * 2 * 3 * 64], int b, int grid,
                                                   const bf16x8* __restrict__ Afr, const bf16x8* __restrict__ Lfr,
                                                   uint32_t afr_bytes, uint32_t lfr_bytes, int nmk, int nmb, int nTn,
                                                   int K, int64_t N, float* __restrict__ part, int64_t ldp,
                                                   const float* __restrict__ a_bound,
                                                   const float* __restrict__ l_bound, bf16x8* __restrict__ Cfr,
                                                   int64_t cexp, const float* __restrict__ colmax) {
  int t, tn, k;
  x6_item<COUT ? kK5cTnOuter : kK5TnOuter>(b, nTn, K, t, tn, k, grid);
  const int nTp = nmb / 4;
  const int lane = threadIdx.x & 63, li = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  floatx4v acc[8][4];
  x6_mainloop16<1, 2, true>(acc, sL, img_rsrc(Lfr, lfr_bytes), (uint32_t)(((int64_t)k * nmb + 4 * t) * nmk) * 3u * kFragBytes,
                            img_rsrc(Afr, afr_bytes), (uint32_t)((8 * tn + 2 * w) * nmk) * 3u * kFragBytes, 4 * t,
                            nmk / 2, nmk);
  if constexpr (COUT) {
    const float cmul = ldexpf(1.f, img_exp(*colmax * *a_bound * 1.0009765625f) -
                                       (img_exp(*a_bound) + img_exp(*l_bound)));
    bf16x8* Ck = Cfr + (int64_t)k * cexp;
    const bool lo_half = lane < 32;
    const int pos = lo_half ? li + 32 * q : 16 + li + 32 * (q - 2);
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float v[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // lanes 0-31: (own 2c, lane + 32's 2c); 32-63: (lane - 32's 2c + 1, own)
          float x0 = acc[ib][2 * c][r], x1 = acc[ib][2 * c + 1][r];
          lane_half_swap(x0, x1);
          v[r] = x0 * cmul;
          v[4 + r] = x1 * cmul;
        }
        bf16x8* dst = Ck + ((((int64_t)8 * tn + 2 * w + c) * nmk + 8 * t + ib) * 3) * 64 + pos;
        if constexpr (kCntStores) {  // read back only by the backward, long after: past L2
          halfx8 h, l;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const _Float16 hi = (_Float16)v[j];
            h[j] = hi;
            l[j] = (_Float16)(v[j] - (float)hi);
          }
          __builtin_nontemporal_store(__builtin_bit_cast(bf16x8, h), dst);
          __builtin_nontemporal_store(__builtin_bit_cast(bf16x8, l), dst + 64);
        } else {
          store_split_f16(dst, v, 1.f);
        }
      }
  }
  // sum over the 128 rows of C^2 per column: 8 blocks x 4 registers, then the 4 lane groups
  const float unscale = ldexpf(1.f, -2 * (img_exp(*a_bound) + img_exp(*l_bound)));
  float* dst = part + ((int64_t)k * nTp + t) * ldp;
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    float s = 0.f;
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
      for (int r = 0; r < 4; ++r) s = fmaf(acc[ib][cb][r], acc[ib][cb][r], s);
    s += lane_xor16(s);
    s += lane_xor32(s);
    const int64_t n = (int64_t)tn * kX6BN + 64 * w + 16 * cb + li;
    if (lane < 16 && n < N) dst[n] = s * unscale;
  }
}

template <bool COUT = false>
__global__ __launch_bounds__(256, 2) void expert_cond16_kernel(const bf16x8* __restrict__ Afr,
                                                               const bf16x8* __restrict__ Lfr, uint32_t afr_bytes,
                                                               uint32_t lfr_bytes, int nmk, int nmb, int nTn, int K,
                                                               int64_t N, float* __restrict__ part, int64_t ldp,
                                                               const float* __restrict__ a_bound,
                                                               const float* __restrict__ l_bound,
                                                               bf16x8* __restrict__ Cfr = nullptr, int64_t cexp = 0,
                                                               const float* __restrict__ colmax = nullptr) {
  __shared__ bf16x8 sL[2][4 * 2 * 3 * 64];  // [row sub-tile][k-step of pair][plane][lane position] (2 planes used)
  expert_cond16_item<COUT>(sL, blockIdx.x, gridDim.x, Afr, Lfr, afr_bytes, lfr_bytes, nmk, nmb, nTn, K, N, part, ldp,
                           a_bound, l_bound, Cfr, cexp, colmax);
}

// One layer's operands of the batched K5.
struct K5Layer {
  const bf16x8* Afr;
  const bf16x8* Lfr;
  float* part;
  const float* a_bound;
  const float* l_bound;
  bf16x8* Cfr;
  const float* colmax;
};

// expert_cond16_kernel over two layers in one launch: workgroups [0, per) run layer 0's
// items, [per, 2 per) layer 1's (same items, same arithmetic: bit-identical partials
// and C_k images); one kernel tail fewer between the layers.
template <bool COUT>
__global__ __launch_bounds__(256, 2) void expert_cond16_pair_kernel(K5Layer l0, K5Layer l1, int per,
                                                                    uint32_t afr_bytes, uint32_t lfr_bytes, int nmk,
                                                                    int nmb, int nTn, int K, int64_t N, int64_t ldp,
                                                                    int64_t cexp) {
  __shared__ bf16x8 sL[2][4 * 2 * 3 * 64];
  const bool second = (int)blockIdx.x >= per;
  const K5Layer& l = second ? l1 : l0;
  expert_cond16_item<COUT>(sL, (int)blockIdx.x - (second ? per : 0), per, l.Afr, l.Lfr, afr_bytes, lfr_bytes, nmk,
                           nmb, nTn, K, N, l.part, ldp, l.a_bound, l.l_bound, l.Cfr, cexp, l.colmax);
}

}  // namespace mgp

using namespace mgp;

extern "C" size_t mgp_expert_x6_workspace_bytes(int64_t M, int64_t N, int32_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 16;
  return (size_t)K * (size_t)(x6_mp(M) / kX6BM) * (size_t)((N + 3) / 4 * 4) * sizeof(float);
}

// Argument checks report the index in mgp_expert_conditional_x6's signature.
static int expert_cond_planes(const void* Afr, size_t afr_bytes, const void* Lfr, size_t lfr_bytes,
                              const float* stats, int64_t lds, const float* variance, int64_t M, int64_t N,
                              int32_t K, int planes, float* fmean, float* fvar, int64_t ldf, void* workspace,
                              size_t workspace_bytes, mgp_stream_t stream, bool f16 = false,
                              bool x8 = false, void* Cfr = nullptr, size_t cfr_bytes = 0,
                              const float* colmax = nullptr) {
  if (!Afr) return -1;
  if (afr_bytes < mgp_x6_cols_bytes(M, N)) return -2;
  if (!Lfr) return -3;
  if (lfr_bytes < mgp_x6_lower_bytes(M, K)) return -4;
  if (!stats) return -5;
  if (lds < N) return -6;
  if (!variance) return -7;
  if (M < 0) return -8;
  if (N < 0) return -9;
  if (K < 1) return -10;
  if (!fmean) return -11;
  if (!fvar) return -12;
  if (ldf < N) return -13;
  if (!aligned16(Afr) || !aligned16(Lfr)) return MGP_ERR_ALIGN;
  if (afr_bytes >= ((size_t)1 << 32) || lfr_bytes >= ((size_t)1 << 32)) return MGP_ERR_UNSUPPORTED;
  if (M == 0 || N == 0) return MGP_OK;
  if (!workspace || workspace_bytes < mgp_expert_x6_workspace_bytes(M, N, K)) return MGP_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t Mp = x6_mp(M);
  const int nmk = (int)(Mp / 16), nmb = (int)(Mp / 32), nTp = (int)(Mp / kX6BM);
  const int nTn = (int)(x6_np(N) / kX6BN);
  const int64_t ldp = (N + 3) / 4 * 4;
  float* part = (float*)workspace;
  const dim3 grid((unsigned)(K * nTp * nTn));
  const float* a_bound = trailer(const_cast<void*>(Afr), cols_planes(M, N));
  const float* l_bound = trailer(const_cast<void*>(Lfr), lower_planes(M, K));
#define MGP_K5_CASE(NP, F16, X8)                                                                        \
  if (planes == NP && f16 == F16 && x8 == X8)                                                           \
    hipLaunchKernelGGL((expert_cond_x6_kernel<NP, F16, X8>), grid, dim3(256), 0, s, (const bf16x8*)Afr, \
                       (const bf16x8*)Lfr, (uint32_t)mgp_x6_cols_bytes(M, N),                           \
                       (uint32_t)mgp_x6_lower_bytes(M, K), nmk, nmb, nTn, K, N, part, ldp, a_bound,     \
                       l_bound);
  if (Cfr) {  // training: + the C_k images (mgp_expert_conditional_f16c)
    if (!f16 || x8 || planes != 2) return MGP_ERR_UNSUPPORTED;
    if (!colmax) return -18;
    const size_t cexp = cols_planes(M, N);
    if (cfr_bytes < (size_t)K * cexp) return -17;
    if (!aligned16(Cfr)) return MGP_ERR_ALIGN;
    hipLaunchKernelGGL((expert_cond16_kernel<true>), grid, dim3(256), 0, s, (const bf16x8*)Afr, (const bf16x8*)Lfr,
                       (uint32_t)mgp_x6_cols_bytes(M, N), (uint32_t)mgp_x6_lower_bytes(M, K), nmk, nmb, nTn, K, N,
                       part, ldp, a_bound, l_bound, (bf16x8*)Cfr, (int64_t)(cexp / 16), colmax);
  } else if (planes == 2 && f16 && !x8) {  // the split-f16 forward K5 (16x16x32 MFMA)
    hipLaunchKernelGGL((expert_cond16_kernel<false>), grid, dim3(256), 0, s, (const bf16x8*)Afr, (const bf16x8*)Lfr,
                       (uint32_t)mgp_x6_cols_bytes(M, N), (uint32_t)mgp_x6_lower_bytes(M, K), nmk, nmb, nTn, K, N,
                       part, ldp, a_bound, l_bound);
  } else {
  MGP_K5_CASE(3, false, false)
  MGP_K5_CASE(2, false, false)
  MGP_K5_CASE(1, false, false)
  MGP_K5_CASE(2, true, true)
  }
#undef MGP_K5_CASE
  int st = launch_status();
  if (st) return st;
  return mgp_launch_cond_finalize(stats, lds, mgp_stats_tiles(M), part, ldp, nTp, variance, N, K, fmean, fvar,
                                  ldf, s);
}

extern "C" int mgp_expert_conditional_x6(const void* Afr, size_t afr_bytes, const void* Lfr, size_t lfr_bytes,
                                         const float* stats, int64_t lds, const float* variance, int64_t M,
                                         int64_t N, int32_t K, float* fmean, float* fvar, int64_t ldf,
                                         void* workspace, size_t workspace_bytes, mgp_stream_t stream) {
  return expert_cond_planes(Afr, afr_bytes, Lfr, lfr_bytes, stats, lds, variance, M, N, K, 3, fmean, fvar, ldf,
                            workspace, workspace_bytes, stream);
}

extern "C" int mgp_expert_conditional_planes(const void* Afr, size_t afr_bytes, const void* Lfr, size_t lfr_bytes,
                                             const float* stats, int64_t lds, const float* variance, int64_t M,
                                             int64_t N, int32_t K, int32_t planes, float* fmean, float* fvar,
                                             int64_t ldf, void* workspace, size_t workspace_bytes,
                                             mgp_stream_t stream) {
  if (planes < 1 || planes > 3) return -11;
  const int st = expert_cond_planes(Afr, afr_bytes, Lfr, lfr_bytes, stats, lds, variance, M, N, K, planes, fmean,
                                    fvar, ldf, workspace, workspace_bytes, stream);
  return (st <= -11 && st >= -13) ? st - 1 : st;  // fmean, fvar, ldf follow `planes` here
}

extern "C" int mgp_expert_conditional_f16(const void* Afr, size_t afr_bytes, const void* Lfr, size_t lfr_bytes,
                                          const float* stats, int64_t lds, const float* variance, int64_t M,
                                          int64_t N, int32_t K, float* fmean, float* fvar, int64_t ldf,
                                          void* workspace, size_t workspace_bytes, mgp_stream_t stream) {
  return expert_cond_planes(Afr, afr_bytes, Lfr, lfr_bytes, stats, lds, variance, M, N, K, 2, fmean, fvar, ldf,
                            workspace, workspace_bytes, stream, true);
}

// Training: mgp_expert_conditional_f16 that also writes C_k = L_k^T A per expert as a
// split-f16 B-layout image (Cfr, mgp_c_images_bytes; colmax from mgp_colnorm_max
// of q_sqrt), consumed by mgp_conditional_backward_f16c.
extern "C" int mgp_expert_conditional_f16c(const void* Afr, size_t afr_bytes, const void* Lfr, size_t lfr_bytes,
                                           const float* stats, int64_t lds, const float* variance, int64_t M,
                                           int64_t N, int32_t K, float* fmean, float* fvar, int64_t ldf,
                                           void* workspace, size_t workspace_bytes, void* Cfr, size_t cfr_bytes,
                                           const float* colmax, mgp_stream_t stream) {
  if (!Cfr) return -16;
  return expert_cond_planes(Afr, afr_bytes, Lfr, lfr_bytes, stats, lds, variance, M, N, K, 2, fmean, fvar, ldf,
                            workspace, workspace_bytes, stream, true, false, Cfr, cfr_bytes, colmax);
}

// mgp_expert_conditional_f16 (Cfr == NULL) or mgp_expert_conditional_f16c (Cfr, colmax:
// host arrays of device pointers) for `batch` (1 or 2) layers of equal M, N, K: one K5
// launch over both layers, then each layer's finalize.  Per-layer operands are host arrays
// of device pointers, one workspace per layer.  Bit-identical to one call per layer.
// Errors: the single call's codes for the first bad layer; -20 for a batch outside [1, 2].
extern "C" int mgp_expert_conditional_f16_batch(int32_t batch, const void* const* Afr, size_t afr_bytes,
                                                const void* const* Lfr, size_t lfr_bytes, const float* const* stats,
                                                int64_t lds, const float* const* variance, int64_t M, int64_t N,
                                                int32_t K, float* const* fmean, float* const* fvar, int64_t ldf,
                                                void* const* workspace, size_t workspace_bytes,
                                                void* const* Cfr, size_t cfr_bytes, const float* const* colmax,
                                                mgp_stream_t stream) {
  if (batch < 1 || batch > 2) return -20;
  if (!Afr || !Lfr || !stats || !variance || !fmean || !fvar || !workspace) return -1;
  const size_t cexp = cols_planes(M, N);
  for (int b = 0; b < batch; ++b) {
    if (!Afr[b]) return -1;
    if (afr_bytes < mgp_x6_cols_bytes(M, N)) return -2;
    if (!Lfr[b]) return -3;
    if (lfr_bytes < mgp_x6_lower_bytes(M, K)) return -4;
    if (!stats[b]) return -5;
    if (lds < N) return -6;
    if (!variance[b]) return -7;
    if (M < 0) return -8;
    if (N < 0) return -9;
    if (K < 1) return -10;
    if (!fmean[b]) return -11;
    if (!fvar[b]) return -12;
    if (ldf < N) return -13;
    if (!aligned16(Afr[b]) || !aligned16(Lfr[b])) return MGP_ERR_ALIGN;
    if (M > 0 && N > 0 && (!workspace[b] || workspace_bytes < mgp_expert_x6_workspace_bytes(M, N, K)))
      return MGP_ERR_WORKSPACE;
    if (Cfr) {
      if (!Cfr[b]) return -16;
      if (cfr_bytes < (size_t)K * cexp) return -17;
      if (!colmax || !colmax[b]) return -18;
      if (!aligned16(Cfr[b])) return MGP_ERR_ALIGN;
    }
  }
  if (afr_bytes >= ((size_t)1 << 32) || lfr_bytes >= ((size_t)1 << 32)) return MGP_ERR_UNSUPPORTED;
  if (M == 0 || N == 0) return MGP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t Mp = x6_mp(M);
  const int nmk = (int)(Mp / 16), nmb = (int)(Mp / 32), nTp = (int)(Mp / kX6BM);
  const int nTn = (int)(x6_np(N) / kX6BN);
  const int64_t ldp = (N + 3) / 4 * 4;
  const int per = K * nTp * nTn;
  K5Layer l[2];
  for (int b = 0; b < 2; ++b) {
    const int q = b < batch ? b : 0;
    l[b] = K5Layer{(const bf16x8*)Afr[q], (const bf16x8*)Lfr[q], (float*)workspace[q],
                   trailer(const_cast<void*>(Afr[q]), cols_planes(M, N)),
                   trailer(const_cast<void*>(Lfr[q]), lower_planes(M, K)), Cfr ? (bf16x8*)Cfr[q] : nullptr,
                   Cfr ? colmax[q] : nullptr};
  }
  const dim3 grid((unsigned)(per * batch));
  const uint32_t ab = (uint32_t)mgp_x6_cols_bytes(M, N), lb = (uint32_t)mgp_x6_lower_bytes(M, K);
  if (Cfr)
    hipLaunchKernelGGL(expert_cond16_pair_kernel<true>, grid, dim3(256), 0, s, l[0], l[1], per, ab, lb, nmk, nmb, nTn,
                       (int)K, N, ldp, (int64_t)(cexp / 16));
  else
    hipLaunchKernelGGL(expert_cond16_pair_kernel<false>, grid, dim3(256), 0, s, l[0], l[1], per, ab, lb, nmk, nmb,
                       nTn, (int)K, N, ldp, (int64_t)0);
  int st = launch_status();
  if (st) return st;
  if (batch == 2)   // both layers' finalize in one launch too
    return mgp_launch_cond_finalize2(CondFinLayer{stats[0], (const float*)workspace[0], variance[0], fmean[0], fvar[0]},
                                     CondFinLayer{stats[1], (const float*)workspace[1], variance[1], fmean[1], fvar[1]},
                                     lds, mgp_stats_tiles(M), ldp, nTp, N, K, ldf, s);
  return mgp_launch_cond_finalize(stats[0], lds, mgp_stats_tiles(M), (const float*)workspace[0], ldp, nTp,
                                  variance[0], N, K, fmean[0], fvar[0], ldf, s);
}

// Split-f16 images with the X8 plane (mgp_split_lower_f16, mgp_split_cols_f16,
// mgp_trsm_stats_f16x8): hi products on f16, cross terms on e4m3 (mfma_f8x).
extern "C" int mgp_expert_conditional_f16x8(const void* Afr, size_t afr_bytes, const void* Lfr, size_t lfr_bytes,
                                            const float* stats, int64_t lds, const float* variance, int64_t M,
                                            int64_t N, int32_t K, float* fmean, float* fvar, int64_t ldf,
                                            void* workspace, size_t workspace_bytes, mgp_stream_t stream) {
  return expert_cond_planes(Afr, afr_bytes, Lfr, lfr_bytes, stats, lds, variance, M, N, K, 2, fmean, fvar, ldf,
                            workspace, workspace_bytes, stream, true, true);
}
