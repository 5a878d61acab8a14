// K4 on the 16-bit matrix cores at f32 accuracy: A = Lm^-1 Kuf with its column statistics.
//
// Reference: the same product as trigemm.hip's K4 -- GPflow base_conditional, reached
// from MixtureGPs/models.py:141-143:
//     A = triangular_solve(Lm, Kmn);  fvar = Knn - sum_m A^2;  fmean = A^T q_mu
// as the lower triangular GEMM A = LinvT^T Kuf, with the per-row-tile column sums of
// A^2 and A q_mu (the stats partials) in the epilogue.
//
// Images (frag_image.hpp; the products and the main loops: x6_mainloop.hpp).  Read: Tfr,
// the image of LinvT (upper; images.hip), and Kfr, the image of Kuf (K1), both split-bf16
// (x6) or split-f16 with their bounds in the image trailers.  Written: Afr, the B-operand
// image of A that K5 (expert_cond.hip) and the conditional backward read -- x6, or
// split-f16 scaled by 2^img_exp(sqrt(variance)) with that bound in its trailer, optionally
// with the e4m3 cross-term plane (f16x8); stats[64-row tile][1 + K][n]; training: A in f32.
//
// Work: one 256-thread workgroup per (pair of 128-row tiles t, nT - 1 - t; column tile of
// 256 n), so every workgroup has the same number of k-steps; wave w owns all 128 rows x 64
// columns of an item.  x6 and f16x8: trsm_stats_x6_kernel on 32x32x16 MFMAs; split-f16 in
// and out (the default): trsm_stats16_kernel on 16x16x32 MFMAs, trsm_stats16_pair_kernel
// for both SMGP layers in one launch.
#include "mgp_common.hpp"
#include "frag_image.hpp"
#include "x6_mainloop.hpp"

#ifndef MGP_K4_STORE_NT
#define MGP_K4_STORE_NT 1   // K4's A-image stores non-temporal (0: plain, for A/B builds)
#endif

namespace mgp {

// Debug builds only (-DMGP_DBG_STAMPS, tools/k4_stamps.py): K4 phase times per
// workgroup on the 100 MHz reference clock (one time base for every CU).
#ifdef MGP_DBG_STAMPS
__device__ unsigned long long g_k4_stamps[4096 * 8];
#define K4STAMP(i, k) do { if (threadIdx.x == 0 && (i) >= 0 && (i) < 4096) g_k4_stamps[(i) * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define K4STAMP(i, k) do {} while (0)
#endif

typedef _Float16 halfx2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------ K4 (x6)
// A = LinvT^T Kuf from the images Tfr (LinvT, upper) and Kfr (Kuf): item =
// (row tile t of 128 rows, heavy = large t first; column tile tn of 256), the
// 16 k-steps... 8 t + 8 k-steps of the lower triangle.  Epilogue: the A image
// (registers 8 s .. 8 s + 7 of each 32x32 tile are one B fragment of K5) and
// the stats of the two 64-row stats tiles 2 t, 2 t + 1 (same layout as the
// f32 K4: stats[st][0][n] = sum A^2, stats[st][1 + kk][n] = sum A q_mu[., kk]).
// a_var != nullptr: A's image is split-f16, scaled by 2^img_exp(sqrt(*a_var))
// (|A[m][n]| <= ||A[:, n]|| <= sqrt(k(x_n, x_n)) = sqrt(variance): the Nystrom
// bound; the image trailer a_bound receives sqrt(*a_var) for the consumer).
// F16IN: Tfr and Kfr are split-f16 images (scales 2^img_exp(*t_bound),
// 2^img_exp(*k_bound)): three f16 products per block instead of six bf16 ones;
// the accumulators are unscaled (exact power of two) before the epilogue.
// X8OUT (with F16OUT): the A image also gets its e4m3 cross-term plane (K5 f16x8);
// its f16 lo plane only when the f32 A is written too (training: the backward
// reads planes 0-1), so a forward-only image moves 4 B per element, not 6.
template <int KMAX, bool F16OUT = false, bool F16IN = false, bool X8OUT = false>
__device__ __forceinline__ void trsm_stats_x6_item(
    bf16x8 (*sL)[4 * 3 * 64], float* __restrict__ sQ, int t, int tn, const bf16x8* __restrict__ Tfr,
    uint32_t tfr_bytes, const bf16x8* __restrict__ Kfr, uint32_t kfr_bytes, int nmk, int64_t M, int64_t N,
    const float* __restrict__ q_mu, int64_t ldq, int K, bf16x8* __restrict__ Afr, float* __restrict__ stats,
    int64_t lds_, float* __restrict__ Af32, int64_t lda, const float* __restrict__ a_var,
    const float* __restrict__ t_bound = nullptr, const float* __restrict__ k_bound = nullptr) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t i0 = 128 * (int64_t)t;
  float a_scale = 1.f;
  if constexpr (F16OUT) a_scale = ldexpf(1.f, img_exp(sqrtf(*a_var)));
  // q_mu rows of this row tile -> LDS [128][KMAX] before the main loop (whose
  // barriers publish it), so the epilogue never waits on a global load.  F16OUT:
  // also max |q_mu| of the tile (sQ[128 KMAX], as float bits; the caller zeroes
  // it), the power-of-two scale of the split q_mu operand of the stats MFMAs
  if (stats) {
    float qmax = 0.f;
    for (int idx = threadIdx.x; idx < 128 * KMAX; idx += 256) {
      const int r = idx / KMAX, kk = idx % KMAX;
      const float q = (i0 + r < M && kk < K) ? q_mu[(i0 + r) * ldq + kk] : 0.f;
      sQ[idx] = q;
      qmax = fmaxf(qmax, fabsf(q));
    }
    if constexpr (F16OUT) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) qmax = fmaxf(qmax, __shfl_xor(qmax, off, 64));
      if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned int*>(sQ + 128 * KMAX), __float_as_uint(qmax));
    }
  }
  floatx16 acc[4][2];
  x6_mainloop<2, 2, F16IN ? 2 : 3, F16IN>(acc, sL, img_rsrc(Tfr, tfr_bytes), (uint32_t)(4 * t * nmk) * 3u * kFragBytes,
                                          img_rsrc(Kfr, kfr_bytes),
                                          (uint32_t)((8 * tn + 2 * w) * nmk) * 3u * kFragBytes, 0, 8 * t + 8, nmk);
  if constexpr (F16IN) {
    const float unscale = ldexpf(1.f, -(img_exp(*t_bound) + img_exp(*k_bound)));
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][c][e] *= unscale;
  }
  if (Af32) store_acc_f32(acc, Af32, lda, i0, (int64_t)tn * kX6BN, M, N, nullptr);
  // ---- epilogue by 32-row sub-tile i: the A image fragments of acc[i] and its
  // contribution to the stats of 64-row stats tile i / 2 (stats[st][0][n] = sum A^2,
  // stats[st][1 + kk][n] = sum A q_mu[., kk]); acc[i] dies after its sub-tile, which
  // keeps the live set to the remaining accumulators + 2 (1 + KMAX) sums (no spills)
  if constexpr (F16OUT) {
    // ---- split-f16: the A image, and the stats q_mu^T A on the matrix cores --
    // per 16-row k-step, the image fragments of acc[i][c] (B operand, k = rows)
    // times the split q_mu fragment (A operand: rows kk < K, k = the same 16
    // rows, from sQ) into sq[c] (32 x 32, rows kk); sum A^2 stays VALU.  Stats
    // tile st = 2 t + i / 2 (64 rows) as the VALU path.
    const int qe = img_exp(__uint_as_float(reinterpret_cast<const unsigned int*>(sQ)[128 * KMAX]));
    const float q_scale = ldexpf(1.f, qe), s_unscale = ldexpf(1.f, -(qe + img_exp(sqrtf(*a_var))));
    const int r = lane & 31, h = lane >> 5;
    floatx16 sq[2];
    float a2[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if ((i & 1) == 0) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          a2[c] = 0.f;
#pragma unroll
          for (int e = 0; e < 16; ++e) sq[c][e] = 0.f;
        }
      }
      const int64_t mk = 8 * (int64_t)t + 2 * i;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        bf16x8 qf[3];
        if (stats) {
          halfx8 qh, ql;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float x = (r < K ? sQ[(32 * i + 16 * s2 + kperm(h, j)) * KMAX + (r < KMAX ? r : 0)] : 0.f) * q_scale;
            const _Float16 xh = (_Float16)x;
            qh[j] = xh;
            ql[j] = (_Float16)(x - (float)xh);
          }
          qf[0] = __builtin_bit_cast(bf16x8, qh);
          qf[1] = __builtin_bit_cast(bf16x8, ql);
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int64_t nb = 8 * (int64_t)tn + 2 * w + c;
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = acc[i][c][8 * s2 + j];
          store_split_f16<X8OUT>(Afr + ((nb * nmk + mk + s2) * 3) * 64 + lane, v, a_scale, Af32 != nullptr);
          if (stats) {
            halfx8 vh, vl;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float x = v[j] * a_scale;
              const _Float16 xh = (_Float16)x;
              vh[j] = xh;
              vl[j] = (_Float16)(x - (float)xh);
              a2[c] = fmaf(v[j], v[j], a2[c]);
            }
            const bf16x8 bf[3] = {__builtin_bit_cast(bf16x8, vh), __builtin_bit_cast(bf16x8, vl), bf16x8{}};
            sq[c] = mfma_fmt<2, true>(qf, bf, sq[c]);
          }
        }
      }
      if (stats && (i & 1)) {
        const int64_t st = 2 * (int64_t)t + (i >> 1);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int64_t n = (int64_t)tn * kX6BN + 64 * w + 32 * c + (lane & 31);
          const float s_a2 = a2[c] + __shfl_xor(a2[c], 32, 64);
          if (n < N && 64 * st < M) {
            float* dst = stats + st * (K + 1) * lds_ + n;
            if (lane < 32) dst[0] = s_a2;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int kk = acc_row(e, lane);
              if (kk < K) dst[(int64_t)(1 + kk) * lds_] = sq[c][e] * s_unscale;
            }
          }
        }
      }
    }
    return;
  }
  float a2[2], qm[2][KMAX];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int64_t nb = 8 * (int64_t)tn + 2 * w + c;
      const int64_t mk = 8 * (int64_t)t + 2 * i;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = acc[i][c][8 * s2 + j];
        store_split(Afr + ((nb * nmk + mk + s2) * 3) * 64 + lane, v);
      }
    }
    if (!stats) continue;
    if ((i & 1) == 0) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        a2[c] = 0.f;
#pragma unroll
        for (int kk = 0; kk < KMAX; ++kk) qm[c][kk] = 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int lr = 32 * i + acc_row(e, lane);
      const float v0 = acc[i][0][e], v1 = acc[i][1][e];
      a2[0] = fmaf(v0, v0, a2[0]);
      a2[1] = fmaf(v1, v1, a2[1]);
#pragma unroll
      for (int kk = 0; kk < KMAX; ++kk) {
        const float q = sQ[lr * KMAX + kk];
        qm[0][kk] = fmaf(v0, q, qm[0][kk]);
        qm[1][kk] = fmaf(v1, q, qm[1][kk]);
      }
    }
    if (i & 1) {
      const int64_t st = 2 * (int64_t)t + (i >> 1);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int64_t n = (int64_t)tn * kX6BN + 64 * w + 32 * c + (lane & 31);
        const float s_a2 = a2[c] + __shfl_xor(a2[c], 32, 64);
        float s_qm[KMAX];
#pragma unroll
        for (int kk = 0; kk < KMAX; ++kk) s_qm[kk] = qm[c][kk] + __shfl_xor(qm[c][kk], 32, 64);
        if (lane < 32 && n < N && 64 * st < M) {
          float* dst = stats + st * (K + 1) * lds_ + n;
          dst[0] = s_a2;
#pragma unroll
          for (int kk = 0; kk < KMAX; ++kk)
            if (kk < K) dst[(int64_t)(1 + kk) * lds_] = s_qm[kk];
        }
      }
    }
  }
}

// One workgroup per (pair of row tiles t, nT - 1 - t; column tile tn): the
// pair holds 8 t + 8 + 8 (nT - t) = 8 nT + 16 k-steps whatever t, so every
// workgroup has the same work; both items read the same Kuf column slab.  Odd
// nT: the middle row tile is an item alone.  (c3: 385 us vs 439 us for one item
// per workgroup, whose register count stays below 256 without spills.)
template <int KMAX, bool F16OUT = false, bool F16IN = false, bool X8OUT = false>
__global__ __launch_bounds__(256, 2) void trsm_stats_x6_kernel(
    const bf16x8* __restrict__ Tfr, uint32_t tfr_bytes, const bf16x8* __restrict__ Kfr, uint32_t kfr_bytes,
    int nmk, int nTn, int64_t M, int64_t N, const float* __restrict__ q_mu, int64_t ldq, int K,
    bf16x8* __restrict__ Afr, float* __restrict__ stats, int64_t lds_, float* __restrict__ Af32, int64_t lda,
    const float* __restrict__ a_var, float* __restrict__ a_bound, const float* __restrict__ t_bound = nullptr,
    const float* __restrict__ k_bound = nullptr) {
  __shared__ bf16x8 sL[2][4 * 3 * 64];
  __shared__ float sQ[128 * KMAX + 1];  // + the tile's max |q_mu| (F16OUT)
  const int nT = nmk / 8, nP = (nT + 1) / 2;
  int p, tn;
  if constexpr (F16OUT)
    if (blockIdx.x == 0 && threadIdx.x == 0) *a_bound = sqrtf(*a_var);
  col_major_item(blockIdx.x, nP, nTn, p, tn);
  if (threadIdx.x == 0) sQ[128 * KMAX] = 0.f;
  __syncthreads();
  trsm_stats_x6_item<KMAX, F16OUT, F16IN, X8OUT>(sL, sQ, nT - 1 - p, tn, Tfr, tfr_bytes, Kfr, kfr_bytes, nmk, M, N, q_mu,
                                          ldq, K, Afr, stats, lds_, Af32, lda, a_var, t_bound, k_bound);
  if (nT - 1 - p == p) return;
  __syncthreads();  // the epilogue's sQ reads before the next item's sQ stores
  if (threadIdx.x == 0) sQ[128 * KMAX] = 0.f;
  __syncthreads();
  trsm_stats_x6_item<KMAX, F16OUT, F16IN, X8OUT>(sL, sQ, p, tn, Tfr, tfr_bytes, Kfr, kfr_bytes, nmk, M, N, q_mu, ldq, K,
                                          Afr, stats, lds_, Af32, lda, a_var, t_bound, k_bound);
}

// ------------------------------------------------------------------ K4 (split-f16) on 16x16x32 MFMAs
// trsm_stats_x6_item<KMAX, true, true> on x6_mainloop16 (as expert_cond16_kernel is K5 on
// it): the same items, images, outputs and bounds.  Epilogue per 16-row block ib (k-step
// 8 t + ib of A's image): the image fragment of each 32-column block from two lanes of the
// 16x16 accumulator layout (one exchange across the lane halves, as K5's C_k images);
// sum A^2 straight from the accumulators; the q_mu^T A stats of each 64-row stats tile on
// 16x16x32 f16 MFMAs whose B operand is the accumulators themselves: lane (i, q) slot j
// holds row 4q + j (j < 4) of block ib and row 4q + j - 4 of block ib + 1 -- any k order
// shared by both operands is the same sum, so the split q_mu operand (from LDS) is built
// in that order and no exchange is needed.  Rows kk of the 16 x 16 stats block are q_mu's
// columns (KMAX <= 16).
__device__ __forceinline__ void store_acc16_f32(const floatx4v (&acc)[8][4], float* __restrict__ out, int64_t ld,
                                                int64_t i0, int64_t n0, int64_t M, int64_t N) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, q = lane >> 4;
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc((void*)out, (short)0, (int)(uint32_t)(M * ld * 4), 0x00020000);
  const uint32_t soff = (uint32_t)((i0 * ld + n0) * 4);
  const uint32_t ld32 = (uint32_t)ld;
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    const int nl = 64 * w + 16 * cb + li;
    if (n0 + nl < N) {
#pragma unroll
      for (int ib = 0; ib < 8; ++ib)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t rl = (uint32_t)(16 * ib + 4 * q + e);
          // (through a float: __builtin_bit_cast of the vector element lvalue itself
          // reads element 0 with this compiler)
          const float x = acc[ib][cb][e];
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, x), r, (rl * ld32 + (uint32_t)nl) * 4u,
                                                soff, 0);
        }
    }
  }
}

template <int KMAX>
__device__ __forceinline__ void trsm_stats16_item(
    bf16x8 (*sL)[4 * 2 * 3 * 64], float* __restrict__ sQ, int t, int tn, const bf16x8* __restrict__ Tfr,
    uint32_t tfr_bytes, const bf16x8* __restrict__ Kfr, uint32_t kfr_bytes, int nmk, int64_t M, int64_t N,
    const float* __restrict__ q_mu, int64_t ldq, int K, bf16x8* __restrict__ Afr, float* __restrict__ stats,
    int64_t lds_, float* __restrict__ Af32, int64_t lda, const float* __restrict__ a_var,
    const float* __restrict__ t_bound, const float* __restrict__ k_bound, int sidx = -1, int sbase = 0) {
  static_assert(KMAX <= 16, "the stats block has 16 rows");
  const int lane = threadIdx.x & 63, li = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t i0 = 128 * (int64_t)t;
  const float a_scale = ldexpf(1.f, img_exp(sqrtf(*a_var)));
  // q_mu rows of the tile -> LDS [128][KMAX] and max |q_mu| (published by the main loop's barriers)
  if (stats) {
    float qmax = 0.f;
    for (int idx = threadIdx.x; idx < 128 * KMAX; idx += 256) {
      const int r = idx / KMAX, kk = idx % KMAX;
      const float qv = (i0 + r < M && kk < K) ? q_mu[(i0 + r) * ldq + kk] : 0.f;
      sQ[idx] = qv;
      qmax = fmaxf(qmax, fabsf(qv));
    }
    qmax = wave_max_f32(qmax);
    if (lane == 0) atomicMax(reinterpret_cast<unsigned int*>(sQ + 128 * KMAX), __float_as_uint(qmax));
  }
  floatx4v acc[8][4];
  x6_mainloop16<2, 2, true>(acc, sL, img_rsrc(Tfr, tfr_bytes), (uint32_t)(4 * t * nmk) * 3u * kFragBytes,
                            img_rsrc(Kfr, kfr_bytes), (uint32_t)((8 * tn + 2 * w) * nmk) * 3u * kFragBytes, 0,
                            4 * t + 4, nmk);
  K4STAMP(sidx, sbase);
  {
    const float unscale = ldexpf(1.f, -(img_exp(*t_bound) + img_exp(*k_bound)));
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[ib][cb][e] *= unscale;
  }
  if (Af32) store_acc16_f32(acc, Af32, lda, i0, (int64_t)tn * kX6BN, M, N);
  // A's image: fragment (column block 8 tn + 2 w + c, k-step 8 t + ib), lane position pos
  const bool lo_half = lane < 32;
  const int pos = lo_half ? li + 32 * q : 16 + li + 32 * (q - 2);
  if (!stats) {  // no stats: the image alone
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float v[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = acc[ib][2 * c][r];
          v[4 + r] = acc[ib][2 * c + 1][r];
          lane_half_swap(v[r], v[4 + r]);
        }
        store_split_f16(Afr + ((((int64_t)8 * tn + 2 * w + c) * nmk + 8 * t + ib) * 3) * 64 + pos, v, a_scale);
      }
    return;
  }
  // With the stats: every accumulator value is split once (x = a 2^e -> f16 hi, f16 lo,
  // packed two per dword) and both the image fragments and the stats products' B
  // operand are assembled from the packed halves (the image's lane-half exchange moves
  // packed halves); row-block pairs (ib0, ib0 + 1) = 64-row stats tile ib0 / 4.
  const int qe = img_exp(__uint_as_float(reinterpret_cast<const unsigned int*>(sQ)[128 * KMAX]));
  const float q_scale = ldexpf(1.f, qe), s_unscale = ldexpf(1.f, -(qe + img_exp(sqrtf(*a_var))));
  floatx4v sq[4];
  float a2[4];
#pragma unroll
  for (int pr4 = 0; pr4 < 4; ++pr4) {  // row blocks ib0 = 2 pr4, ib0 + 1
    const int ib0 = 2 * pr4, st2 = pr4 >> 1;
    if ((pr4 & 1) == 0) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        sq[cb] = floatx4v{0.f, 0.f, 0.f, 0.f};
        a2[cb] = 0.f;
      }
    }
    uint32_t hp[2][4][2], lp[2][4][2];  // [row block of the pair][column block][dword]
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          const float a0 = acc[ib0 + d][cb][2 * h2], a1 = acc[ib0 + d][cb][2 * h2 + 1];
          a2[cb] = fmaf(a1, a1, fmaf(a0, a0, a2[cb]));
          const float x0 = a0 * a_scale, x1 = a1 * a_scale;
          const _Float16 h0 = (_Float16)x0, h1 = (_Float16)x1;
          const halfx2 hh = {h0, h1}, ll = {(_Float16)(x0 - (float)h0), (_Float16)(x1 - (float)h1)};
          hp[d][cb][h2] = __builtin_bit_cast(uint32_t, hh);
          lp[d][cb][h2] = __builtin_bit_cast(uint32_t, ll);
        }
    // the image fragments of row blocks ib0, ib0 + 1
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        // lanes 0-31: (own block 2c, lane + 32's 2c); 32-63: (lane - 32's 2c + 1, own 2c + 1)
        uint32_t h0[2], h1[2], l0[2], l1[2];
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          h0[h2] = hp[d][2 * c][h2];
          h1[h2] = hp[d][2 * c + 1][h2];
          l0[h2] = lp[d][2 * c][h2];
          l1[h2] = lp[d][2 * c + 1][h2];
          lane_half_swap(h0[h2], h1[h2]);
          lane_half_swap(l0[h2], l1[h2]);
        }
        const u32x4v fh = u32x4v{h0[0], h0[1], h1[0], h1[1]};
        const u32x4v fl = u32x4v{l0[0], l0[1], l1[0], l1[1]};
        bf16x8* dst = Afr + ((((int64_t)8 * tn + 2 * w + c) * nmk + 8 * t + ib0 + d) * 3) * 64 + pos;
#if MGP_K4_STORE_NT   // streaming stores: fewer dirty L2 lines for the kernel boundary
        __builtin_nontemporal_store(__builtin_bit_cast(bf16x8, fh), dst);
        __builtin_nontemporal_store(__builtin_bit_cast(bf16x8, fl), dst + 64);
#else
        dst[0] = __builtin_bit_cast(bf16x8, fh);
        dst[64] = __builtin_bit_cast(bf16x8, fl);
#endif
      }
    // q_mu^T A of this row-block pair: B operand slot j = row 4q + j of block ib0 (j < 4),
    // row 4q + j - 4 of block ib0 + 1
    bf16x8 qf[3];
    {
      halfx8 qh, ql;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = 16 * ib0 + (j < 4 ? 4 * q + j : 16 + 4 * q + j - 4);
        const float x = (li < K ? sQ[row * KMAX + (li < KMAX ? li : 0)] : 0.f) * q_scale;
        const _Float16 xh = (_Float16)x;
        qh[j] = xh;
        ql[j] = (_Float16)(x - (float)xh);
      }
      qf[0] = __builtin_bit_cast(bf16x8, qh);
      qf[1] = __builtin_bit_cast(bf16x8, ql);
    }
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const bf16x8 bf[3] = {__builtin_bit_cast(bf16x8, u32x4v{hp[0][cb][0], hp[0][cb][1], hp[1][cb][0], hp[1][cb][1]}),
                            __builtin_bit_cast(bf16x8, u32x4v{lp[0][cb][0], lp[0][cb][1], lp[1][cb][0], lp[1][cb][1]}),
                            bf16x8{}};
      sq[cb] = mfma16_fmt<2, true>(qf, bf, sq[cb]);
    }
    if ((pr4 & 1) == 1) {  // 64-row stats tile 2 t + st2 done
      const int64_t st = 2 * (int64_t)t + st2;
      if (64 * st < M) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
          const int64_t n = (int64_t)tn * kX6BN + 64 * w + 16 * cb + li;
          float s_a2 = a2[cb] + lane_xor16(a2[cb]);
          s_a2 += lane_xor32(s_a2);
          if (n < N) {
            float* dst = stats + st * (K + 1) * lds_ + n;
            if (lane < 16) dst[0] = s_a2;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int kk = 4 * q + e;
              if (kk < K) dst[(int64_t)(1 + kk) * lds_] = sq[cb][e] * s_unscale;
            }
          }
        }
      }
    }
  }
}

// Row-tile pairs as trsm_stats_x6_kernel (equal work per workgroup).
template <int KMAX>
__global__ __launch_bounds__(256, 2) void trsm_stats16_kernel(
    const bf16x8* __restrict__ Tfr, uint32_t tfr_bytes, const bf16x8* __restrict__ Kfr, uint32_t kfr_bytes,
    int nmk, int nTn, int64_t M, int64_t N, const float* __restrict__ q_mu, int64_t ldq, int K,
    bf16x8* __restrict__ Afr, float* __restrict__ stats, int64_t lds_, float* __restrict__ Af32, int64_t lda,
    const float* __restrict__ a_var, float* __restrict__ a_bound, const float* __restrict__ t_bound,
    const float* __restrict__ k_bound) {
  __shared__ bf16x8 sL[2][4 * 2 * 3 * 64];
  __shared__ float sQ[128 * KMAX + 1];
  const int nT = nmk / 8, nP = (nT + 1) / 2;
  int p, tn;
  if (blockIdx.x == 0 && threadIdx.x == 0) *a_bound = sqrtf(*a_var);
  col_major_item(blockIdx.x, nP, nTn, p, tn);
  const int it = blockIdx.x;  // debug stamps only
  K4STAMP(it, 0);
  if (threadIdx.x == 0) sQ[128 * KMAX] = 0.f;
  __syncthreads();
  trsm_stats16_item<KMAX>(sL, sQ, nT - 1 - p, tn, Tfr, tfr_bytes, Kfr, kfr_bytes, nmk, M, N, q_mu, ldq, K, Afr, stats,
                          lds_, Af32, lda, a_var, t_bound, k_bound, it, 1);
  K4STAMP(it, 2);
  if (nT - 1 - p == p) return;
  __syncthreads();
  if (threadIdx.x == 0) sQ[128 * KMAX] = 0.f;
  __syncthreads();
  trsm_stats16_item<KMAX>(sL, sQ, p, tn, Tfr, tfr_bytes, Kfr, kfr_bytes, nmk, M, N, q_mu, ldq, K, Afr, stats, lds_,
                          Af32, lda, a_var, t_bound, k_bound, it, 3);
  K4STAMP(it, 4);
}

// One layer's operands of the batched K4 (both SMGP layers share M, N and K).
struct K4Layer {
  const bf16x8* Tfr;
  const bf16x8* Kfr;
  const float* q_mu;
  bf16x8* Afr;
  float* stats;
  float* Af32;
  const float* a_var;
  float* a_bound;
  const float* t_bound;
  const float* k_bound;
  int64_t ldq, lds, lda;
};

// trsm_stats16_kernel over two layers in one launch: workgroups [0, per) run layer 0's
// items, [per, 2 per) layer 1's, each exactly as the one-layer kernel does (same items,
// same arithmetic: bit-identical images and statistics).  One launch instead of two
// drops a dispatch round boundary and a kernel tail between the layers.
template <int KMAX>
__global__ __launch_bounds__(256, 2) void trsm_stats16_pair_kernel(K4Layer l0, K4Layer l1, int per,
                                                                  uint32_t tfr_bytes, uint32_t kfr_bytes, int nmk,
                                                                  int nTn, int64_t M, int64_t N, int K) {
  __shared__ bf16x8 sL[2][4 * 2 * 3 * 64];
  __shared__ float sQ[128 * KMAX + 1];
  const bool second = (int)blockIdx.x >= per;
  const K4Layer& l = second ? l1 : l0;
  const int bid = (int)blockIdx.x - (second ? per : 0);
  const int nT = nmk / 8, nP = (nT + 1) / 2;
  int p, tn;
  if (bid == 0 && threadIdx.x == 0) *l.a_bound = sqrtf(*l.a_var);
  col_major_item(bid, nP, nTn, p, tn);
  if (threadIdx.x == 0) sQ[128 * KMAX] = 0.f;
  __syncthreads();
  trsm_stats16_item<KMAX>(sL, sQ, nT - 1 - p, tn, l.Tfr, tfr_bytes, l.Kfr, kfr_bytes, nmk, M, N, l.q_mu, l.ldq, K,
                          l.Afr, l.stats, l.lds, l.Af32, l.lda, l.a_var, l.t_bound, l.k_bound);
  if (nT - 1 - p == p) return;
  __syncthreads();
  if (threadIdx.x == 0) sQ[128 * KMAX] = 0.f;
  __syncthreads();
  trsm_stats16_item<KMAX>(sL, sQ, p, tn, l.Tfr, tfr_bytes, l.Kfr, kfr_bytes, nmk, M, N, l.q_mu, l.ldq, K, l.Afr,
                          l.stats, l.lds, l.Af32, l.lda, l.a_var, l.t_bound, l.k_bound);
}

}  // namespace mgp

using namespace mgp;

template <int KMAX>
static int launch_trsm_x6(const void* Tfr, size_t tb, const void* Kfr, size_t kb, int64_t M, int64_t N,
                          const float* q_mu, int64_t ldq, int K, void* Afr, float* stats, int64_t lds,
                          float* A, int64_t lda, hipStream_t s, const float* a_var = nullptr,
                          bool f16in = false, bool x8 = false) {
  const int64_t Mp = x6_mp(M);
  const int nmk = (int)(Mp / 16), nT = (int)(Mp / kX6BM), nTn = (int)(x6_np(N) / kX6BN);
  const dim3 grid((unsigned)((nT + 1) / 2 * nTn));
  float* a_bound = trailer(Afr, cols_planes(M, N));
  if (f16in) {
    const float* t_bound = trailer(const_cast<void*>(Tfr), lower_planes(M, 1));
    const float* k_bound = trailer(const_cast<void*>(Kfr), cols_planes(M, N));
    if (x8)
      hipLaunchKernelGGL((trsm_stats_x6_kernel<KMAX, true, true, true>), grid, dim3(256), 0, s, (const bf16x8*)Tfr,
                         (uint32_t)tb, (const bf16x8*)Kfr, (uint32_t)kb, nmk, nTn, M, N, q_mu, ldq, K,
                         (bf16x8*)Afr, stats, lds, A, lda, a_var, a_bound, t_bound, k_bound);
    else
      hipLaunchKernelGGL((trsm_stats16_kernel<KMAX>), grid, dim3(256), 0, s, (const bf16x8*)Tfr, (uint32_t)tb,
                         (const bf16x8*)Kfr, (uint32_t)kb, nmk, nTn, M, N, q_mu, ldq, K, (bf16x8*)Afr, stats, lds, A,
                         lda, a_var, a_bound, t_bound, k_bound);
  } else if (a_var)
    hipLaunchKernelGGL((trsm_stats_x6_kernel<KMAX, true>), grid, dim3(256), 0, s, (const bf16x8*)Tfr,
                       (uint32_t)tb, (const bf16x8*)Kfr, (uint32_t)kb, nmk, nTn, M, N, q_mu, ldq, K,
                       (bf16x8*)Afr, stats, lds, A, lda, a_var, a_bound);
  else
    hipLaunchKernelGGL((trsm_stats_x6_kernel<KMAX, false>), grid, dim3(256), 0, s, (const bf16x8*)Tfr,
                       (uint32_t)tb, (const bf16x8*)Kfr, (uint32_t)kb, nmk, nTn, M, N, q_mu, ldq, K,
                       (bf16x8*)Afr, stats, lds, A, lda, a_var, a_bound);
  return launch_status();
}

extern "C" int mgp_trsm_stats_x6(const void* Tfr, size_t tfr_bytes, const void* Kfr, size_t kfr_bytes,
                                 int64_t M, int64_t N, const float* q_mu, int64_t ldq, int32_t K,
                                 void* Afr, size_t afr_bytes, float* stats, int64_t lds, float* A,
                                 int64_t lda, mgp_stream_t stream) {
  if (!Tfr) return -1;
  if (tfr_bytes < mgp_x6_lower_bytes(M, 1)) return -2;
  if (!Kfr) return -3;
  if (kfr_bytes < mgp_x6_cols_bytes(M, N)) return -4;
  if (M < 0) return -5;
  if (N < 0) return -6;
  if (!q_mu) return -7;
  if (ldq < K) return -8;
  if (K < 1) return -9;
  if (K > 16) return MGP_ERR_UNSUPPORTED;
  if (!Afr) return -10;
  if (afr_bytes < mgp_x6_cols_bytes(M, N)) return -11;
  if (stats && lds < N) return -13;
  if (A && lda < N) return -15;
  if (!aligned16(Tfr) || !aligned16(Kfr) || !aligned16(Afr)) return MGP_ERR_ALIGN;
  if (mgp_x6_cols_bytes(M, N) >= ((size_t)1 << 32) || mgp_x6_lower_bytes(M, 1) >= ((size_t)1 << 32))
    return MGP_ERR_UNSUPPORTED;
  if (M == 0 || N == 0) return MGP_OK;
  hipStream_t s = (hipStream_t)stream;
  const size_t tb = mgp_x6_lower_bytes(M, 1), kb = mgp_x6_cols_bytes(M, N);
  if (K <= 4) return launch_trsm_x6<4>(Tfr, tb, Kfr, kb, M, N, q_mu, ldq, K, Afr, stats, lds, A, lda, s);
  if (K <= 8) return launch_trsm_x6<8>(Tfr, tb, Kfr, kb, M, N, q_mu, ldq, K, Afr, stats, lds, A, lda, s);
  return launch_trsm_x6<16>(Tfr, tb, Kfr, kb, M, N, q_mu, ldq, K, Afr, stats, lds, A, lda, s);
}

// ------------------------------------------------------------------ split-f16 ("f16x3") K5 path
static int trsm_stats_f16_out(const void* Tfr, size_t tfr_bytes, const void* Kfr, size_t kfr_bytes, int64_t M,
                              int64_t N, const float* q_mu, int64_t ldq, int32_t K, const float* variance, void* Afr,
                              size_t afr_bytes, float* stats, int64_t lds, mgp_stream_t stream, bool f16in,
                              float* A = nullptr, int64_t lda = 0, bool x8 = false) {
  if (!Tfr) return -1;
  if (tfr_bytes < mgp_x6_lower_bytes(M, 1)) return -2;
  if (!Kfr) return -3;
  if (kfr_bytes < mgp_x6_cols_bytes(M, N)) return -4;
  if (M < 0) return -5;
  if (N < 0) return -6;
  if (!q_mu) return -7;
  if (ldq < K) return -8;
  if (K < 1) return -9;
  if (K > 16) return MGP_ERR_UNSUPPORTED;
  if (!variance) return -10;
  if (!Afr) return -11;
  if (afr_bytes < mgp_x6_cols_bytes(M, N)) return -12;
  if (stats && lds < N) return -14;  // stats may be NULL (A image only)
  
  if (!aligned16(Tfr) || !aligned16(Kfr) || !aligned16(Afr)) return MGP_ERR_ALIGN;
  if (mgp_x6_cols_bytes(M, N) >= ((size_t)1 << 32) || mgp_x6_lower_bytes(M, 1) >= ((size_t)1 << 32))
    return MGP_ERR_UNSUPPORTED;
  if (M == 0 || N == 0) return MGP_OK;
  hipStream_t s = (hipStream_t)stream;
  const size_t tb = mgp_x6_lower_bytes(M, 1), kb = mgp_x6_cols_bytes(M, N);
  if (K <= 4)
    return launch_trsm_x6<4>(Tfr, tb, Kfr, kb, M, N, q_mu, ldq, K, Afr, stats, lds, A, lda, s, variance, f16in, x8);
  if (K <= 8)
    return launch_trsm_x6<8>(Tfr, tb, Kfr, kb, M, N, q_mu, ldq, K, Afr, stats, lds, A, lda, s, variance, f16in, x8);
  return launch_trsm_x6<16>(Tfr, tb, Kfr, kb, M, N, q_mu, ldq, K, Afr, stats, lds, A, lda, s, variance, f16in, x8);
}

// x6 images in (Tfr, Kfr), split-f16 A image out (K5's operand).
extern "C" int mgp_trsm_stats_x6_f16(const void* Tfr, size_t tfr_bytes, const void* Kfr, size_t kfr_bytes,
                                     int64_t M, int64_t N, const float* q_mu, int64_t ldq, int32_t K,
                                     const float* variance, void* Afr, size_t afr_bytes, float* stats,
                                     int64_t lds, mgp_stream_t stream) {
  return trsm_stats_f16_out(Tfr, tfr_bytes, Kfr, kfr_bytes, M, N, q_mu, ldq, K, variance, Afr, afr_bytes, stats, lds,
                            stream, false);
}

// split-f16 images in (mgp_split_upper_f16, mgp_rbf_kuf_f16) and out: three f16
// products per block instead of six bf16 ones.
extern "C" int mgp_trsm_stats_f16(const void* Tfr, size_t tfr_bytes, const void* Kfr, size_t kfr_bytes, int64_t M,
                                  int64_t N, const float* q_mu, int64_t ldq, int32_t K, const float* variance,
                                  void* Afr, size_t afr_bytes, float* stats, int64_t lds, float* A, int64_t lda,
                                  mgp_stream_t stream) {
  if (A && lda < N) return -16;
  return trsm_stats_f16_out(Tfr, tfr_bytes, Kfr, kfr_bytes, M, N, q_mu, ldq, K, variance, Afr, afr_bytes, stats, lds,
                            stream, true, A, lda);
}

// mgp_trsm_stats_f16 for `batch` (1 or 2) layers of equal M, N, K in one launch (the two
// SMGP layers' K4); the per-layer operands are host arrays of device pointers (A[b] may be
// NULL; A itself may be NULL: no f32 A for any layer).  Results are bit-identical to one
// mgp_trsm_stats_f16 call per layer.  Errors: the single call's codes for the first bad
// layer; -17 for a batch outside [1, 2].
extern "C" int mgp_trsm_stats_f16_batch(int32_t batch, const void* const* Tfr, size_t tfr_bytes,
                                        const void* const* Kfr, size_t kfr_bytes, int64_t M, int64_t N,
                                        const float* const* q_mu, int64_t ldq, int32_t K,
                                        const float* const* variance, void* const* Afr, size_t afr_bytes,
                                        float* const* stats, int64_t lds, float* const* A, int64_t lda,
                                        mgp_stream_t stream) {
  if (batch < 1 || batch > 2) return -17;
  if (!Tfr || !Kfr || !q_mu || !variance || !Afr || !stats) return -1;
  if (A && lda < N) return -16;
  for (int b = 0; b < batch; ++b) {
    if (!Tfr[b]) return -1;
    if (tfr_bytes < mgp_x6_lower_bytes(M, 1)) return -2;
    if (!Kfr[b]) return -3;
    if (kfr_bytes < mgp_x6_cols_bytes(M, N)) return -4;
    if (M < 0) return -5;
    if (N < 0) return -6;
    if (!q_mu[b]) return -7;
    if (ldq < K) return -8;
    if (K < 1) return -9;
    if (K > 16) return MGP_ERR_UNSUPPORTED;
    if (!variance[b]) return -10;
    if (!Afr[b]) return -11;
    if (afr_bytes < mgp_x6_cols_bytes(M, N)) return -12;
    if (!stats[b]) return -13;
    if (lds < N) return -14;
    if (!aligned16(Tfr[b]) || !aligned16(Kfr[b]) || !aligned16(Afr[b])) return MGP_ERR_ALIGN;
  }
  if (mgp_x6_cols_bytes(M, N) >= ((size_t)1 << 32) || mgp_x6_lower_bytes(M, 1) >= ((size_t)1 << 32))
    return MGP_ERR_UNSUPPORTED;
  if (M == 0 || N == 0) return MGP_OK;
  const size_t tb = mgp_x6_lower_bytes(M, 1), kb = mgp_x6_cols_bytes(M, N);
  const int64_t Mp = x6_mp(M);
  const int nmk = (int)(Mp / 16), nT = (int)(Mp / kX6BM), nTn = (int)(x6_np(N) / kX6BN);
  const int per = (nT + 1) / 2 * nTn;
  K4Layer l[2];
  for (int b = 0; b < 2; ++b) {
    const int s = b < batch ? b : 0;
    l[b] = K4Layer{(const bf16x8*)Tfr[s], (const bf16x8*)Kfr[s], q_mu[s], (bf16x8*)Afr[s], stats[s],
                   A ? A[s] : nullptr, variance[s], trailer(Afr[s], cols_planes(M, N)),
                   trailer(const_cast<void*>(Tfr[s]), lower_planes(M, 1)),
                   trailer(const_cast<void*>(Kfr[s]), cols_planes(M, N)), ldq, lds, lda};
  }
  const dim3 grid((unsigned)(per * batch));
  hipStream_t s = (hipStream_t)stream;
  if (K <= 4)
    hipLaunchKernelGGL(trsm_stats16_pair_kernel<4>, grid, dim3(256), 0, s, l[0], l[1], per, (uint32_t)tb,
                       (uint32_t)kb, nmk, nTn, M, N, (int)K);
  else if (K <= 8)
    hipLaunchKernelGGL(trsm_stats16_pair_kernel<8>, grid, dim3(256), 0, s, l[0], l[1], per, (uint32_t)tb,
                       (uint32_t)kb, nmk, nTn, M, N, (int)K);
  else
    hipLaunchKernelGGL(trsm_stats16_pair_kernel<16>, grid, dim3(256), 0, s, l[0], l[1], per, (uint32_t)tb,
                       (uint32_t)kb, nmk, nTn, M, N, (int)K);
  return launch_status();
}

// mgp_trsm_stats_f16 that also writes the A image's e4m3 cross-term plane (the
// operand of mgp_expert_conditional_f16x8).  With A == NULL the f16 lo plane is
// not written (only the f16x8 K5 reads that image).
extern "C" int mgp_trsm_stats_f16x8(const void* Tfr, size_t tfr_bytes, const void* Kfr, size_t kfr_bytes, int64_t M,
                                    int64_t N, const float* q_mu, int64_t ldq, int32_t K, const float* variance,
                                    void* Afr, size_t afr_bytes, float* stats, int64_t lds, float* A, int64_t lda,
                                    mgp_stream_t stream) {
  if (A && lda < N) return -16;
  return trsm_stats_f16_out(Tfr, tfr_bytes, Kfr, kfr_bytes, M, N, q_mu, ldq, K, variance, Afr, afr_bytes, stats, lds,
                            stream, true, A, lda, true);
}

#ifdef MGP_DBG_STAMPS
extern "C" int mgp_dbg_k4_stamps(unsigned long long* host) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(mgp::g_k4_stamps), sizeof(mgp::g_k4_stamps));
}
#endif
