// The conditional backward: reverse mode of K4 and K5 on the 16-bit matrix cores.
//
// Reference: reverse mode of GPflow base_conditional's A = triangular_solve(Lm, Kmn),
// fmean = A^T q_mu, fvar = Knn - sum_m A^2 + sum_m' (L_k^T A)^2 with
// L_k = band_part(q_sqrt[k], -1, 0) (MixtureGPs/models.py:141-143).  For the cotangents
// G_mu = dELBO/dfmean and Gv = dELBO/dfvar ([K][N] each), in the order of
// conditional_backward's steps:
//     gA       = q_mu G_mu - 2 A sum_k Gv_k + 2 sum_k (S_k A) diag(Gv_k),  S_k = L_k L_k^T
//                (with the forward's C_k = L_k^T A images: 2 sum_k L_k (C_k diag(Gv_k)))
//     g_Kuf    = L^-T gA = Linv^T gA
//     g_q_sqrt[k] = 2 tril(P_k L_k),  P_k = A diag(Gv_k) A^T
//     g_Lm     = -tril(g_Kuf A^T),  g_q_mu = A G_mu^T,  g_var = sum Gv
//
// Images (frag_image.hpp; the products and the main loops: x6_mainloop.hpp).  Read: Afr,
// A's image from K4 (trsm_stats.hip), with the f32 A; the images of S_k or of L_k and of
// Linv, built here through images.hip's launchers; with the C path the C_k images of the
// training K5 (expert_cond.hip).  Written: gA as an image (x6, or split-f16 with one
// exponent per (128-row tile, column)), A's row image for the P_k gram, and the f32
// gradients.  The grams (P_k, g_q_sqrt, g_Lm, g_q_mu) are gram.hip's.
//
// Work: the MFMA kernels take one 256-thread workgroup per item of 128 rows x 128 or 256
// columns in col_major_item's order (grad_a_c*: per row-tile pair, as K4); the kernels
// that only read A or fold partials are described where they stand.
#include <algorithm>

#include "mgp_common.hpp"
#include "frag_image.hpp"
#include "x6_mainloop.hpp"

namespace mgp {

// ------------------------------------------------------------------ backward (x6)
// gA0[m][n] = sum_k q_mu[m][k] G_mu[k][n] - 2 A[m][n] sum_k Gv[k][n]: the part
// of the A gradient that needs no GEMM (one thread per column n, looping rows).
template <int KMAX>
__global__ __launch_bounds__(256) void grad_a_base_kernel(const float* __restrict__ A, int64_t lda,
                                                          const float* __restrict__ q_mu, int64_t ldq,
                                                          const float* __restrict__ Gmu,
                                                          const float* __restrict__ Gv, int64_t ldg, int64_t M,
                                                          int64_t N, int K, int rows_per_block,
                                                          float* __restrict__ out, int64_t ldo) {
  __shared__ float sq[64][KMAX];
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  float gmu[KMAX], gvs = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    gmu[k] = (k < K && n < N) ? Gmu[(int64_t)k * ldg + n] : 0.f;
    if (k < K && n < N) gvs += Gv[(int64_t)k * ldg + n];
  }
  for (int64_t rb = r0; rb < r0 + rows_per_block && rb < M; rb += 64) {
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * KMAX; i += 256) {
      const int rr = i / KMAX, k = i % KMAX;
      sq[rr][k] = (rb + rr < M && k < K) ? q_mu[(rb + rr) * ldq + k] : 0.f;
    }
    __syncthreads();
    if (n < N) {
      const int rows = (int)((M - rb) < 64 ? (M - rb) : 64);
      for (int rr = 0; rr < rows; ++rr) {
        float v = -2.f * A[(rb + rr) * lda + n] * gvs;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) v = fmaf(sq[rr][k], gmu[k], v);
        out[(rb + rr) * ldo + n] = v;
      }
    }
  }
}

// Steps 2, 5 (A's row image) and 6 (g_q_mu) of the split-f16 conditional backward
// in ONE pass over A (three kernels read A before: grad_a_base, split_rows_f16,
// gram_narrow).  Workgroup: one slab of 8 k-steps (128 n) x kPrepRB 32-row blocks;
// G_mu and sum_k Gv over the slab's columns are staged in LDS once.  Per row block:
//   (1) coalesced: thread t takes rows t / 32 + 8 i (i < 4), columns 4 (t % 32) + e
//       of A (16-B loads, two 512-B rows per wave instruction) and writes
//       gA0[m][n] = sum_k q_mu[m][k] G_mu[k][n] - 2 A[m][n] sum_k Gv[k][n] the same
//       way, and puts the tile into LDS (pitch 132 floats: conflict-free reads below);
//   (2) fragments: lane (r, h) of wave w takes row r, k-steps w and w + 4
//       (n = 16 ns + 8 h + j), stores split_rows_f16(A)'s image (same layout and
//       scale 2^img_exp(*bound)) and sums A[m][n] G_mu[k][n] for g_q_mu:
//       part[slab][m][k] (f32 per slab; folded in float64 by prep_fold_kernel).
// The tile and the row sums are double-buffered: one barrier per row block.
// c3 (MI355X, rocprofv3): 205 us per layer against 126 + 90 + 111 + 12 us for
// grad_a_base, split_rows_f16, gram_narrow and its fold (profiles/r03_grad_a_prep_probe.log).
// Measured, not kept: the next row block's A loads issued before (2) (287 vs 248 us),
// 4 instead of 8 row blocks per workgroup (same).
constexpr int kPrepRB = 8, kPrepPitch = 132;
template <int KMAX>
__global__ __launch_bounds__(256) void grad_a_prep_kernel(const float* __restrict__ A, int64_t lda,
                                                          const float* __restrict__ q_mu, int64_t ldq,
                                                          const float* __restrict__ Gmu,
                                                          const float* __restrict__ Gv, int64_t ldg, int64_t M,
                                                          int64_t N, int K, int nns, const float* __restrict__ bound,
                                                          float* __restrict__ gA0, int64_t ldo,
                                                          bf16x8* __restrict__ img, float* __restrict__ part, int rbs, int qvec,
                                                          float* __restrict__ amax = nullptr) {
  __shared__ __attribute__((aligned(16))) float sg[KMAX + 1][128];  // G_mu rows, then sum_k Gv
  __shared__ __attribute__((aligned(16))) float sA[2][32][kPrepPitch];
  __shared__ float sp[2][4][32][KMAX];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t nsb = 8 * (int64_t)blockIdx.x, n0 = 16 * nsb;
  const int64_t rb0 = (int64_t)blockIdx.y * rbs;
  const int nblk = (int)((M + 31) / 32);
  const int nit = nblk - rb0 < rbs ? (int)(nblk - rb0) : rbs;
  for (int i = tid; i < (KMAX + 1) * 32; i += 256) {  // 4 columns per item
    const int k = i >> 5, c = 4 * (i & 31);
    const int64_t n = n0 + c;
    floatx4 v = {0.f, 0.f, 0.f, 0.f};
    if (k < KMAX) {
      if (k < K) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = n + e < N ? Gmu[(int64_t)k * ldg + n + e] : 0.f;
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < KMAX; ++kk)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += (kk < K && n + e < N) ? Gv[(int64_t)kk * ldg + n + e] : 0.f;
    }
    *reinterpret_cast<floatx4*>(&sg[k][c]) = v;
  }
  __syncthreads();
  const float scale = ldexpf(1.f, img_exp(*bound));
  const int ct_r = tid >> 5, ct_c = 4 * (tid & 31);
  const int64_t nc = n0 + ct_c;
  const bool colvec = nc + 3 < N;
  floatx4 gmu4[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) gmu4[k] = *reinterpret_cast<const floatx4*>(&sg[k][ct_c]);
  const floatx4 gvs4 = *reinterpret_cast<const floatx4*>(&sg[KMAX][ct_c]);
  auto flush = [&](int it, int b) {
    for (int i = tid; i < 32 * KMAX; i += 256) {
      const int rr = i / KMAX, k = i % KMAX;
      const int64_t m = 32 * (rb0 + it) + rr;
      if (m < M && k < K)
        part[((int64_t)blockIdx.x * M + m) * K + k] = (sp[b][0][rr][k] + sp[b][1][rr][k]) + (sp[b][2][rr][k] + sp[b][3][rr][k]);
    }
  };
  auto load_rows = [&](floatx4 (&a)[4], int64_t rb) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = 32 * rb + ct_r + 8 * i;
      a[i] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (row < M) {
        if (colvec) {
          a[i] = *reinterpret_cast<const floatx4*>(A + row * lda + nc);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) a[i][e] = nc + e < N ? A[row * lda + nc + e] : 0.f;
        }
      }
    }
  };
  floatx4 a[4];
  for (int it = 0; it < nit; ++it) {
    const int64_t rb = rb0 + it;
    const int b = it & 1;
    load_rows(a, rb);
    if (amax) {  // max |A[m][.]| over this slab per row -> amax[slab][m] (rowmax_fold_kernel)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float m =
            half_max_f32(fmaxf(fmaxf(fabsf(a[i][0]), fabsf(a[i][1])), fmaxf(fabsf(a[i][2]), fabsf(a[i][3]))));
        const int64_t row = 32 * rb + ct_r + 8 * i;
        if ((tid & 31) == 0 && row < M) amax[(int64_t)blockIdx.x * M + row] = m;
      }
    }
    // (1) coalesced rows: gA0, the LDS tile
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = 32 * rb + ct_r + 8 * i;
      if (row < M) {
        floatx4 g = -2.f * a[i] * gvs4;
        if (qvec) {  // q_mu's row in 16-B loads (ldq % 4 == 0, K a multiple of 4)
#pragma unroll
          for (int k4 = 0; k4 < KMAX / 4; ++k4) {
            if (4 * k4 < K) {
              const floatx4 q = *reinterpret_cast<const floatx4*>(q_mu + row * ldq + 4 * k4);
#pragma unroll
              for (int e = 0; e < 4; ++e) g += q[e] * gmu4[4 * k4 + e];
            }
          }
        } else {
#pragma unroll
          for (int k = 0; k < KMAX; ++k)
            if (k < K) g += q_mu[row * ldq + k] * gmu4[k];
        }
        float* dst = gA0 + row * ldo + nc;
        if (colvec) {
          *reinterpret_cast<floatx4*>(dst) = g;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (nc + e < N) dst[e] = g[e];
        }
      }
      *reinterpret_cast<floatx4*>(&sA[b][ct_r + 8 * i][ct_c]) = a[i];
    }
    __syncthreads();
    if (it > 0) flush(it - 1, b ^ 1);
    // (2) fragments: the image and the g_q_mu row sums
    float pf[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) pf[k] = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int st = w + 4 * s2;
      const int64_t ns = nsb + st;
      if (ns >= nns) continue;
      const int c = 16 * st + 8 * h;
      const floatx4 lo = *reinterpret_cast<const floatx4*>(&sA[b][r][c]);
      const floatx4 hi = *reinterpret_cast<const floatx4*>(&sA[b][r][c + 4]);
      float v[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = lo[j];
        v[4 + j] = hi[j];
      }
      store_split_f16(img + (rb * nns + ns) * 128 + lane, v, scale);
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[k] = fmaf(v[j], sg[k][c + j], pf[k]);
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) pf[k] += __shfl_xor(pf[k], 32, 64);
    if (h == 0) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k) sp[b][w][r][k] = pf[k];
    }
  }
  __syncthreads();
  if (nit > 0) flush(nit - 1, (nit - 1) & 1);
}

// out[m][k] = sum over the slabs of part[slab][m][k] in float64, fixed order:
// 16 outputs per workgroup, thread (o, g) sums slabs g, g + 16, ... (four running
// sums, slab c into sum (c / 16) % 4), then the 16 groups in order.
__global__ __launch_bounds__(256) void prep_fold_kernel(const float* __restrict__ part, int slabs, int64_t M, int K,
                                                        float* __restrict__ out, int64_t ldo) {
  __shared__ double sred[16][17];
  const int o = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int64_t MK = M * K, idx = (int64_t)blockIdx.x * 16 + o;
  double v = 0.0;
  if (idx < MK) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int c = g;
    for (; c + 48 < slabs; c += 64) {
      a0 += (double)part[(int64_t)c * MK + idx];
      a1 += (double)part[(int64_t)(c + 16) * MK + idx];
      a2 += (double)part[(int64_t)(c + 32) * MK + idx];
      a3 += (double)part[(int64_t)(c + 48) * MK + idx];
    }
    for (int u = 0; c < slabs; c += 16, ++u) {
      const double x = (double)part[(int64_t)c * MK + idx];
      if (u == 0) a0 += x; else if (u == 1) a1 += x; else a2 += x;
    }
    v = (a0 + a1) + (a2 + a3);
  }
  sred[g][o] = v;
  __syncthreads();
  if (threadIdx.x < 16 && idx < MK) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) t += sred[q][o];
    out[(idx / K) * ldo + idx % K] = (float)t;
  }
}

// B-b: gA (image) = 2 sum_k (S_k A) diag(Gv_k) + gA0 with S_k = L_k L_k^T
// (full split images): item = (row tile t of 128 rows, column tile tn of
// 128), wave w owns the 32 columns of B block 4 tn + w.  Each expert's
// product runs through the K5 main loop (full T, one column sub-tile per
// wave) and is folded into the output registers with its column weights, so
// no per-expert intermediate is written.
// F16: Sfr and Afr are split-f16 images (scales 2^img_exp(*s_bound), 2^img_exp(*a_bound)):
// three f16 products per block; the unscale folds into the column weights.
// X8 (with F16): the S_k A products on f16 hi products + e4m3 cross terms
// (mfma_f8x; both images carry the e4m3 plane in the f16x8 training step).
template <bool F16 = false, bool X8 = false>
__global__ __launch_bounds__(256, 2) void grad_a_s_kernel(const bf16x8* __restrict__ Sfr, uint32_t s_bytes,
                                                          const bf16x8* __restrict__ Afr, uint32_t afr_bytes,
                                                          int nmk, int nTn, int K, int64_t M, int64_t N,
                                                          const float* __restrict__ Gv, int64_t ldg,
                                                          const float* __restrict__ gA0, int64_t ld0,
                                                          bf16x8* __restrict__ gAfr,
                                                          const float* __restrict__ s_bound = nullptr,
                                                          const float* __restrict__ a_bound = nullptr) {
  __shared__ bf16x8 sL[2][4 * 3 * 64];
  const int nT = nmk / 8, nmb = nmk / 2;
  int t, tn;
  col_major_item(blockIdx.x, nT, nTn, t, tn);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nb = 4 * (int64_t)tn + w;
  const int64_t n = 32 * nb + (lane & 31);
  floatx16 acc[4][1], out[4][1];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) out[i][0][e] = 0.f;
  const int64_t s_elems = (int64_t)nmb * nmk * 3 * 64;  // one expert's S image (bf16x8 units)
  float unscale = 1.f;
  if constexpr (F16) unscale = ldexpf(1.f, -(img_exp(*s_bound) + img_exp(*a_bound)));
  for (int k = 0; k < K; ++k) {
    x6_mainloop<0, 1, F16 ? 2 : 3, F16, X8>(acc, sL, img_rsrc(Sfr + k * s_elems, s_bytes),
                                        (uint32_t)(4 * t * nmk) * 3u * kFragBytes, img_rsrc(Afr, afr_bytes),
                                        (uint32_t)(nb * nmk) * 3u * kFragBytes, 0, nmk, nmk);
    const float g = n < N ? Gv[(int64_t)k * ldg + n] * unscale : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) out[i][0][e] = fmaf(g, acc[i][0][e], out[i][0][e]);
  }
  const int64_t i0 = 128 * (int64_t)t;
  const __amdgpu_buffer_rsrc_t r0 =
      __builtin_amdgcn_make_buffer_rsrc((void*)gA0, (short)0, (int)(uint32_t)(M * ld0 * 4), 0x00020000);
  const uint32_t soff = (uint32_t)((i0 * ld0 + 128 * (int64_t)tn) * 4), ld32 = (uint32_t)ld0;
  const int nl = 32 * w + (lane & 31);
  const bool ok = n < N;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const uint32_t rl = (uint32_t)(32 * i + acc_row(e, lane));
      const float b0 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r0, (rl * ld32 + (uint32_t)nl) * 4u, soff, 0));
      v[e] = ok ? fmaf(2.f, out[i][0][e], b0) : 0.f;   // rows >= M read 0 (outside the resource)
    }
    const int64_t mk = 8 * (int64_t)t + 2 * i;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      float u[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) u[j] = v[8 * s2 + j];
      store_split(gAfr + ((nb * nmk + mk + s2) * 3) * 64 + lane, u);
    }
  }
}

// B-b on split-f16 images (grad_a_s_kernel<true> restated for LDS economy):
// gA = 2 sum_k (S_k A) diag(Gv_k) + gA0.  Item = (row tile t of 128, column tile
// tn of 128) as grad_a_s_kernel, but each wave owns a 64 x 64 quarter (row half
// wr = w / 2, column half wc = w % 2: 2 sub-tiles x 2 column blocks), so a T
// fragment read from LDS feeds two column blocks, and two experts run per pass
// of the main loop, sharing every B fragment (A's image).  Per wave and k-step:
// 8 LDS reads, 4 B loads, 24 MFMAs (grad_a_s_kernel: 8 LDS reads and 2 B loads
// per 12) -- half the LDS bytes per MFMA, which bound that kernel.  Odd K: the
// last pass pairs the last expert with itself at weight 0.
__global__ __launch_bounds__(256, 2) void grad_a_s_f16_kernel(const bf16x8* __restrict__ Sfr, uint32_t s_bytes,
                                                             const bf16x8* __restrict__ Afr, uint32_t afr_bytes,
                                                             int nmk, int nTn, int K, int64_t M, int64_t N,
                                                             const float* __restrict__ Gv, int64_t ldg,
                                                             const float* __restrict__ gA0, int64_t ld0,
                                                             bf16x8* __restrict__ gAfr,
                                                             const float* __restrict__ s_bound,
                                                             const float* __restrict__ a_bound) {
  __shared__ bf16x8 sL[2][2][4 * 3 * 64];  // [stage][expert of the pair][sub-tile][plane][lane]
  const int nT = nmk / 8, nmb = nmk / 2;
  int t, tn;
  col_major_item(blockIdx.x, nT, nTn, t, tn);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 1, wc = w & 1;
  const int64_t nbw = 4 * (int64_t)tn + 2 * wc;  // the wave's first column block
  int64_t ncol[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) ncol[c] = 32 * (nbw + c) + (lane & 31);
  const float unscale = ldexpf(1.f, -(img_exp(*s_bound) + img_exp(*a_bound)));
  const __amdgpu_buffer_rsrc_t rT = img_rsrc(Sfr, s_bytes), rB = img_rsrc(Afr, afr_bytes);
  const uint32_t sexp = (uint32_t)nmb * (uint32_t)nmk * 3u * kFragBytes;  // one expert's S image
  const uint32_t tb = (uint32_t)(4 * t * nmk) * 3u * kFragBytes;
  const uint32_t sB0 = (uint32_t)(nbw * nmk) * 3u * kFragBytes, sBc = (uint32_t)nmk * 3u * kFragBytes;
  const uint32_t vB = 16u * lane;
  // T stage units (both experts): e = tid + 256 s -> sub-tile e / 128, plane (e / 64) % 2
  uint32_t vT[2];
  int dT[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const int e = tid + 256 * s2, i = e / 128, p = (e / 64) % 2;
    vT[s2] = (uint32_t)((i * nmk * 192 + p * 64 + (e & 63)) * 16);
    dT[s2] = (3 * i + p) * 64 + (e & 63);
  }
  floatx16 out[2][2];
#pragma unroll
  for (int il = 0; il < 2; ++il)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) out[il][c][e] = 0.f;

  for (int k = 0; k < K; k += 2) {
    const int k1 = k + 1 < K ? k + 1 : k;
    const uint32_t tb0 = (uint32_t)k * sexp + tb, tb1 = (uint32_t)k1 * sexp + tb;
    floatx16 acc0[2][2], acc1[2][2];
#pragma unroll
    for (int il = 0; il < 2; ++il)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          acc0[il][c][e] = 0.f;
          acc1[il][c][e] = 0.f;
        }
    auto load_b = [&](bf16x8 (&b)[2][3], int mk) {
      const uint32_t o = (uint32_t)mk * 3u * kFragBytes;
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int p = 0; p < 2; ++p) b[c][p] = ld_frag(rB, vB, sB0 + c * sBc + o + p * kFragBytes);
    };
    auto load_t = [&](u32x4v (&st)[4], int mk) {
      const uint32_t o = (uint32_t)mk * 192u * 16u;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        st[s2] = __builtin_amdgcn_raw_buffer_load_b128(rT, vT[s2], tb0 + o, 0);
        st[2 + s2] = __builtin_amdgcn_raw_buffer_load_b128(rT, vT[s2], tb1 + o, 0);
      }
    };
    auto store_t = [&](int buf, const u32x4v (&st)[4]) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        reinterpret_cast<u32x4v*>(sL[buf][0])[dT[s2]] = st[s2];
        reinterpret_cast<u32x4v*>(sL[buf][1])[dT[s2]] = st[2 + s2];
      }
    };
    auto compute = [&](int buf, const bf16x8 (&b)[2][3]) {
#pragma unroll
      for (int il = 0; il < 2; ++il) {
        const int i = 2 * wr + il;
        bf16x8 a0[3], a1[3];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          a0[p] = sL[buf][0][(i * 3 + p) * 64 + lane];
          a1[p] = sL[buf][1][(i * 3 + p) * 64 + lane];
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          acc0[il][c] = mfma_fmt<2, true>(a0, b[c], acc0[il][c]);
          acc1[il][c] = mfma_fmt<2, true>(a1, b[c], acc1[il][c]);
        }
      }
    };
    bf16x8 b0[2][3], b1[2][3];
    u32x4v st[4];
    load_t(st, 0);
    load_b(b0, 0);
    store_t(0, st);
    __syncthreads();
#pragma nounroll
    for (int mk = 0; mk < nmk; mk += 2) {
      load_t(st, mk + 1);
      load_b(b1, mk + 1);
      __builtin_amdgcn_sched_barrier(0);
      compute(0, b0);
      __builtin_amdgcn_sched_barrier(0);
      store_t(1, st);
      __syncthreads();
      const int m2 = mk + 2 < nmk ? mk + 2 : nmk - 1;  // after the last pair: harmless reload
      load_t(st, m2);
      load_b(b0, m2);
      __builtin_amdgcn_sched_barrier(0);
      compute(1, b1);
      __builtin_amdgcn_sched_barrier(0);
      store_t(0, st);
      __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float g0 = ncol[c] < N ? Gv[(int64_t)k * ldg + ncol[c]] * unscale : 0.f;
      const float g1 = (k + 1 < K && ncol[c] < N) ? Gv[(int64_t)(k + 1) * ldg + ncol[c]] * unscale : 0.f;
#pragma unroll
      for (int il = 0; il < 2; ++il)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          out[il][c][e] = fmaf(g1, acc1[il][c][e], fmaf(g0, acc0[il][c][e], out[il][c][e]));
    }
  }

  // gA = 2 out + gA0, stored as the split image (bf16 x6, for B-d)
  const int64_t i0 = 128 * (int64_t)t;
  const __amdgpu_buffer_rsrc_t r0 =
      __builtin_amdgcn_make_buffer_rsrc((void*)gA0, (short)0, (int)(uint32_t)(M * ld0 * 4), 0x00020000);
  const uint32_t soff = (uint32_t)((i0 * ld0 + 128 * (int64_t)tn) * 4), ld32 = (uint32_t)ld0;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int nl = 32 * (2 * wc + c) + (lane & 31);
    const bool ok = ncol[c] < N;
#pragma unroll
    for (int il = 0; il < 2; ++il) {
      const int i = 2 * wr + il;
      float v[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const uint32_t rl = (uint32_t)(32 * i + acc_row(e, lane));
        const float a0 = __builtin_bit_cast(
            float, __builtin_amdgcn_raw_buffer_load_b32(r0, (rl * ld32 + (uint32_t)nl) * 4u, soff, 0));
        v[e] = ok ? fmaf(2.f, out[il][c][e], a0) : 0.f;  // rows >= M read 0 (outside the resource)
      }
      const int64_t mk = 8 * (int64_t)t + 2 * i;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float u[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) u[j] = v[8 * s2 + j];
        store_split(gAfr + (((nbw + c) * nmk + mk + s2) * 3) * 64 + lane, u);
      }
    }
  }
}

// B-b from the forward's C images (split-f16 training, mgp_conditional_backward_f16c):
// gA = 2 sum_k L_k (C_k diag(Gv_k)) + gA0 -- the triangular L_k instead of the full
// S_k = L_k L_k^T, so half of grad_a_s's products, and no S_k build.  T = L_k's
// image with rows m, k-steps over m' <= m (DIAG 2, mk < 8 t + 8), B = C_k's image
// (one column sub-tile per wave).  A workgroup takes the row-tile pair (nT - 1 - p,
// p) of a column tile for every expert in turn (K4's balancing): the pairs of a
// column tile then do equal work per expert and stay in step on one XCD, so each
// C_k column strip is read from HBM about once and served to the other pairs
// from L2 (one row tile per workgroup: the light tiles ran ahead through the
// experts and every strip came from HBM/MALL ~4.5 times).
// cexp != nullptr (MGP_TRSM_BWD16): the image is split-f16 instead of x6, each
// column of the 128-row tile t scaled by 2^e, e = img_exp(max over the tile's rows of
// |gA[., n]|) -- exact per (tile, column), so no bound can be loose -- and e goes to
// cexp[t][n] (kCexpZero for an all-zero tile) for trsm_bwd16_kernel.
constexpr float kCexpZero = 1000.f;
template <int NC>
__device__ __forceinline__ void grad_a_c_store(const floatx16 (&out)[4][NC], int c, int t, int tn, int w, int lane,
                                               int nmk, int64_t M, int64_t N, const float* __restrict__ gA0,
                                               int64_t ld0, bf16x8* __restrict__ gAfr, float* __restrict__ cexp,
                                               int64_t ldc) {
  const int64_t nb = 4 * (int64_t)tn + w;
  const int64_t n = 32 * nb + (lane & 31);
  const int64_t i0 = 128 * (int64_t)t;
  const __amdgpu_buffer_rsrc_t r0 =
      __builtin_amdgcn_make_buffer_rsrc((void*)gA0, (short)0, (int)(uint32_t)(M * ld0 * 4), 0x00020000);
  const uint32_t soff = (uint32_t)((i0 * ld0 + 128 * (int64_t)tn) * 4), ld32 = (uint32_t)ld0;
  const int nl = 32 * w + (lane & 31);
  const bool ok = n < N;
  if (cexp) {
    float v[4][16];
    float mx = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const uint32_t rl = (uint32_t)(32 * i + acc_row(e, lane));
        const float b0 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r0, (rl * ld32 + (uint32_t)nl) * 4u, soff, 0));
        v[i][e] = ok ? fmaf(2.f, out[i][c][e], b0) : 0.f;
        mx = fmaxf(mx, fabsf(v[i][e]));
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // the column's other 16 rows of each 32-row block
    // 2^ex as two factors: a tile of tiny values (|gA| < 2^-114) needs ex > 127
    const int ex = img_exp(mx), ex1 = ex / 2;
    const float sc1 = ldexpf(1.f, ex1), scale = ldexpf(1.f, ex - ex1);
    if (lane < 32 && ok) cexp[t * ldc + n] = mx > 0.f ? (float)ex : kCexpZero;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t mk = 8 * (int64_t)t + 2 * i;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float u[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) u[j] = v[i][8 * s2 + j] * sc1;
        store_split_f16(gAfr + ((nb * nmk + mk + s2) * 3) * 64 + lane, u, scale);
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const uint32_t rl = (uint32_t)(32 * i + acc_row(e, lane));
      const float b0 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r0, (rl * ld32 + (uint32_t)nl) * 4u, soff, 0));
      v[e] = ok ? fmaf(2.f, out[i][c][e], b0) : 0.f;  // rows >= M read 0 (outside the resource)
    }
    const int64_t mk = 8 * (int64_t)t + 2 * i;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      float u[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) u[j] = v[8 * s2 + j];
      store_split(gAfr + ((nb * nmk + mk + s2) * 3) * 64 + lane, u);
    }
  }
}

template <int I, int N, typename F>
__device__ __forceinline__ void static_for_from(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for_from<I + 1, N>(f);
  }
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_from<0, N>(f);
}

// One continuous pipeline over the K L k-steps of a row tile (L = 8 t + 8 per
// expert), in blocks of 8 k-steps: for each 8-row-step block of m' (outer), for
// each expert k, its 8 k-steps.  T (L_k's row slab, via registers into the LDS
// double buffer), B (C_k's fragments, straight to registers) and g = Gv_k[n] are
// loaded PD k-steps ahead into a register ring of PD + 1 sets, across expert and
// block boundaries; every load of a k-step is issued before any of a later one
// (vector loads complete in order), so the wait for k-step s + 1's T slab never
// forces a younger prefetch.  Block order keeps the workgroups of a column tile in
// step: all start the first pass (row tile nT - 1 - p, nT - p blocks) at block 0 and
// advance one block per unit time, and the second pass (row tile p) runs its blocks
// downwards, which puts every workgroup at block nT - time in it -- so each C_k
// strip is fetched about twice per column tile, not once per workgroup.
// The per-column expert weights need no second accumulator set: acc holds the
// running sum in units of the current expert's g, sum (g_j / g_k) P_j, rescaled by
// g_k / g_k' at each expert switch (every 8 k-steps) and by the last g at the end
// -- each rescale is one f32 rounding relative to the running total, as for
// out += g acc.  |g| is clamped from below to 2^-40 max_k |g_k[n]| (the clamp moves
// the result by < 2^-40 of the largest contribution; the quotient stays < 2^82 of
// it).  DIAG masks are not applied: the zero blocks of the diagonal tile are
// zero-filled in the image (8 % more MFMAs, no branch in the pipeline).
// NC: 32-column sub-tiles per wave (workgroup = 128 rows x 128 NC columns).
// grad_a_c_kernel's prefetch distance and column sub-tiles per wave (c3, MI355X:
// PD 3 / NC 1 1.72 ms; PD 1 / NC 2 1.77 ms, 264 B of spill in its epilogue)
#ifndef MGP_GAC_PD
#define MGP_GAC_PD 3
#define MGP_GAC_NC 1
#endif
constexpr int kGacPD = MGP_GAC_PD, kGacNC = MGP_GAC_NC;
// the split-f16 C-images backward on grad_a_c16_kernel (0: grad_a_c_kernel; A/B)
#ifndef MGP_GAC16
#define MGP_GAC16 1
#endif
constexpr bool kGac16 = MGP_GAC16;
// grad_a_c16_kernel's row-tile groups per workgroup (1; 2: two row tiles at once, measured
// slower -- 3.0 vs 1.78 ms per launch for 3.2 vs 8.1 GB fetched, r06k_gac16_train_ab.log)
#ifndef MGP_GAC16_G
#define MGP_GAC16_G 1
#endif
constexpr int kGac16G = MGP_GAC16_G;

template <int PD, int NC>
__global__ __launch_bounds__(256, 2) void grad_a_c_kernel(const bf16x8* __restrict__ Ltfr, uint32_t lt_bytes,
                                                         const bf16x8* __restrict__ Cfr, int64_t cexp,
                                                         uint32_t c_bytes, int nmk, int nTn, int K, int64_t M,
                                                         int64_t N, const float* __restrict__ Gv, int64_t ldg,
                                                         const float* __restrict__ gA0, int64_t ld0,
                                                         bf16x8* __restrict__ gAfr,
                                                         const float* __restrict__ l_bound,
                                                         const float* __restrict__ a_bound,
                                                         const float* __restrict__ colmax,
                                                         float* __restrict__ gexp, int64_t ldc) {
  constexpr int U = PD + 1;
  static_assert(8 % U == 0, "the ring cycles within an expert's 8 k-steps (and the LDS double buffer)");
  __shared__ bf16x8 sL[2][4 * 3 * 64];
  const int nT = nmk / 8, nmb = nmk / 2, nP = (nT + 1) / 2;
  int p, tn;
  col_major_item(blockIdx.x, nP, nTn, p, tn);
  const int t1 = nT - 1 - p, t2 = p;  // t1 == t2: the middle tile of an odd nT, alone
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t nb = 4 * NC * (int64_t)tn + NC * w;  // column blocks nb .. nb + NC - 1 (32 wide)
  const float unscale =
      ldexpf(1.f, -(img_exp(*l_bound) + img_exp(*colmax * *a_bound * 1.0009765625f)));
  const __amdgpu_buffer_rsrc_t rT = img_rsrc(Ltfr, lt_bytes);
  const __amdgpu_buffer_rsrc_t rG =
      __builtin_amdgcn_make_buffer_rsrc((void*)Gv, (short)0, (int)(uint32_t)(K * ldg * 4), 0x00020000);
  uint32_t vG[NC];
  float gmin[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int64_t n = 32 * (nb + c) + (lane & 31);
    vG[c] = (uint32_t)(n < N ? n : 0) * 4u;
    float gmax = 0.f;
    for (int k = 0; k < K; ++k)
      gmax = fmaxf(gmax, fabsf(__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                             rG, vG[c], (uint32_t)(k * ldg * 4), 0))));
    gmin[c] = fmaxf(gmax * 0x1p-40f, 0x1p-126f);
  }
  // T stage: thread tid moves units e = tid + 256 s (s = 0, 1): row sub-tile e / 128,
  // plane (e / 64) % 2, lane e % 64
  uint32_t vT[2];
  int dT[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int e = tid + 256 * s, i = e / 128, pl = (e / 64) % 2;
    vT[s] = (uint32_t)((i * nmk * 192 + pl * 64 + (e & 63)) * 16);
    dT[s] = (3 * i + pl) * 64 + (e & 63);
  }
  const uint32_t vB = 16u * lane;
  for (int pass = 0; pass < (t2 != t1 ? 2 : 1); ++pass) {
    const int t = pass ? t2 : t1;
    const int L = 8 * t + 8, S = K * L;
    u32x4v st[U][2];
    bf16x8 bb[U][NC][3];
    // the load stream's k-step: 8-step block lmb (outer; the second pass runs it
    // downwards), expert lk, mk = 8 lmb + lj; index ls
    const int dmb = pass ? -1 : 1;
    int lk = 0, lmb = pass ? t : 0, lj = 0, ls = 0;
    auto issue = [&](auto jc) {
      constexpr int J = decltype(jc)::value;
      const int lmk = 8 * lmb + lj;
      const uint32_t ot = (uint32_t)(((int64_t)lk * nmb + 4 * t) * nmk + lmk) * 192u * 16u;
#pragma unroll
      for (int s = 0; s < 2; ++s) st[J][s] = __builtin_amdgcn_raw_buffer_load_b128(rT, vT[s], ot, 0);
      const __amdgpu_buffer_rsrc_t rB = img_rsrc(Cfr + (int64_t)lk * cexp, c_bytes);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const uint32_t ob = (uint32_t)((nb + c) * nmk + lmk) * 3u * kFragBytes;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) bb[J][c][pl] = ld_frag(rB, vB, ob + pl * kFragBytes);
      }
      if (ls < S - 1) {  // advance (the stream stays on the last k-step once it is reached)
        ++ls;
        if (++lj == 8) {
          lj = 0;
          if (++lk == K) {
            lk = 0;
            lmb += dmb;
          }
        }
      }
    };
    auto loadg = [&](int k, float (&g)[NC]) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const float x =
            __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rG, vG[c], (uint32_t)(k * ldg * 4), 0));
        g[c] = __builtin_copysignf(fmaxf(fabsf(x), gmin[c]), x);
      }
    };
    floatx16 acc[4][NC];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][c][e] = 0.f;
    // compute stream: expert ck; acc in units of gcur (= expert ck's g)
    int ck = 0;
    float gcur[NC], gnext[NC];
    loadg(0, gcur);
    static_for<PD>([&](auto jc) { issue(jc); });
#pragma unroll
    for (int s = 0; s < 2; ++s) reinterpret_cast<u32x4v*>(sL[0])[dT[s]] = st[0][s];
    __syncthreads();
    // the 8 k-steps of one (block, expert)
#pragma nounroll
    for (int s0 = 0; s0 < S; s0 += 8) {
      static_for<8>([&](auto jc) {
        constexpr int JJ = decltype(jc)::value, J = JJ % U;
        issue(std::integral_constant<int, (J + PD) % U>{});
        if constexpr (JJ == 0) loadg(ck + 1 < K ? ck + 1 : 0, gnext);  // needed at JJ = 7
        __builtin_amdgcn_sched_barrier(0);
        // NC = 1: all 8 LDS reads in flight before the first MFMA (3 MFMAs per
        // fragment pair would wait on each read); NC = 2: two sub-tiles at a time
        constexpr int RB = NC == 1 ? 4 : 2;
#pragma unroll
        for (int i0 = 0; i0 < 4; i0 += RB) {
          bf16x8 a[RB][3];
#pragma unroll
          for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) a[i][pl] = sL[J % 2][((i0 + i) * 3 + pl) * 64 + lane];
          if constexpr (RB == 4) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[i0 + i][c] = mfma_fmt<2, true>(a[i], bb[J][c], acc[i0 + i][c]);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (JJ == 7) {  // end of the expert's 8 k-steps: to units of the next one's g
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            const float r = gcur[c] / gnext[c];
            gcur[c] = gnext[c];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int e = 0; e < 16; ++e) acc[i][c][e] *= r;
          }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) reinterpret_cast<u32x4v*>(sL[(J + 1) % 2])[dT[s]] = st[(J + 1) % U][s];
        __syncthreads();
      });
      if (++ck == K) ck = 0;
    }
    // acc is in units of gcur (the wrapped-around expert 0's g after the last block)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float gl = gcur[c] * unscale;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][c][e] *= gl;
      // column block nb + c as (128-column tile, wave) of the one-block store
      grad_a_c_store(acc, c, t, (int)((nb + c) / 4), (int)((nb + c) % 4), lane, nmk, M, N, gA0, ld0, gAfr, gexp,
                     ldc);
    }
  }
}

// B-b from the C images on 16x16x32 MFMAs (round 6; replaces grad_a_c_kernel in the
// split-f16 training step): the same sum gA = 2 sum_k L_k (C_k diag(Gv_k)) + gA0 and the
// same per-(tile, column) exponent image, but with K5's main-loop shape instead of
// grad_a_c's 32x32x16 one -- wave tile 128 rows x 64 columns (8 x 4 blocks of 16 x 16),
// one LDS barrier per 32-deep k-step PAIR (96 MFMAs per wave) instead of per 16-deep
// k-step (12 MFMAs), and half the LDS bytes per MFMA (each staged L_k fragment feeds
// four column blocks instead of one).  grad_a_c measured 54-57 % MFMA busy with an
// LDS read per 1.5 MFMAs; K5's shape runs at ~80 %.
// Item = (row-tile pair (nT - 1 - p, p), 256-column tile tn), both passes as grad_a_c.
// The pair stream of a pass (row tile t): blocks of 4 pairs (8 k-steps) outer (the
// second pass runs them downwards, as grad_a_c, so the workgroups of a column tile
// stay in step on one XCD), experts inner; after an expert's 4 pairs the accumulator
// goes to units of the next expert's column weight (grad_a_c's rescale: one f32
// rounding per switch relative to the running sum, |g| clamped below at 2^-40 of the
// column's largest).  The column weights (K x 256) and their clamps sit in LDS.
// Zero blocks of the diagonal tile are zero-filled in the L_k image (no masks).
constexpr int kGac16KMax = 16;
// G = 1 (the default): two passes per 256-thread workgroup, as above.  G = 2 (measured,
// not kept): a 512-thread workgroup takes the row tiles (2j + 1, 2j) of a column tile AT
// ONCE, one per 4-wave group, over one stream of blocks ascending, so that both groups
// read the same C_k fragments between the same barriers.  With G = 1 the row-tile
// workgroups of a column tile share the C_k strips only through L2 when they happen to
// be in step (8.1 GB fetched per launch for 2.1 GB of images, profiles/
// r06i_pmc_cond_bwd_f16c.json); G = 2 fetches 3.2 GB but runs 3.0 ms instead of 1.78
// (one 8-wave workgroup per CU, a barrier over both groups, the short tile's group idle
// through the long tile's extra blocks) -- the fetched bytes are not what bounds it.
template <int G>
__global__ __launch_bounds__(256 * G, 2 / G) void grad_a_c16_kernel(const bf16x8* __restrict__ Ltfr, uint32_t lt_bytes,
                                                            const bf16x8* __restrict__ Cfr, int64_t cexp,
                                                            uint32_t c_bytes, int nmk, int nTn, int K, int64_t M,
                                                            int64_t N, const float* __restrict__ Gv, int64_t ldg,
                                                            const float* __restrict__ gA0, int64_t ld0,
                                                            bf16x8* __restrict__ gAfr,
                                                            const float* __restrict__ l_bound,
                                                            const float* __restrict__ a_bound,
                                                            const float* __restrict__ colmax,
                                                            float* __restrict__ gexp, int64_t ldc) {
  __shared__ bf16x8 sL[G][2][4 * 2 * 2 * 64];
  __shared__ float sG[kGac16KMax * 256];
  const int nT = nmk / 8, nmb = nmk / 2;
  const int nI = G == 1 ? (nT + 1) / 2 : (nT + 1) / 2;   // items per column tile
  int p, tn;
  col_major_item(blockIdx.x, nI, nTn, p, tn);
  const int grp = G == 2 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8)) : 0;
  // G = 1: passes over row tiles t1 = nT - 1 - p, then t2 = p (t1 == t2: the middle tile of
  // an odd nT, alone).  G = 2: one pass over blocks 0 .. th, th = min(2p + 1, nT - 1);
  // group 0 owns row tile th, group 1 row tile 2p (none when th == 2p)
  const int th = G == 2 ? (2 * p + 1 < nT ? 2 * p + 1 : nT - 1) : 0;
  const int own2 = grp == 0 ? th : (2 * p < th ? 2 * p : -1);
  const int tid = threadIdx.x & 255, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float unscale =
      ldexpf(1.f, -(img_exp(*l_bound) + img_exp(*colmax * *a_bound * 1.0009765625f)));
  // column weights of the tile (column tid), clamped from below at 2^-40 of the column's largest
  if (grp == 0) {
    const int64_t n = 256 * (int64_t)tn + tid;
    float gmax = 0.f;
    for (int k = 0; k < K; ++k) {
      const float x = n < N ? Gv[(int64_t)k * ldg + n] : 0.f;
      sG[k * 256 + tid] = x;
      gmax = fmaxf(gmax, fabsf(x));
    }
    const float gmin = fmaxf(gmax * 0x1p-40f, 0x1p-126f);
    for (int k = 0; k < K; ++k) {
      const float x = sG[k * 256 + tid];
      sG[k * 256 + tid] = __builtin_copysignf(fmaxf(fabsf(x), gmin), x);
    }
  }
  // T staging (x6_mainloop16, NPL 2): unit e = tid + 256 s: sub-tile e / 256, k-step
  // (e / 128) % 2 of the pair, plane (e / 64) % 2
  uint32_t vT[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int e = tid + 256 * s, i = e / 256, kk = (e / 128) % 2, pl = (e / 64) % 2;
    vT[s] = (uint32_t)((((i * nmk + kk) * 3 + pl) * 64 + (e & 63)) * 16);
  }
  const uint32_t vB = (uint32_t)((((q >> 1) * 3) * 64 + li + 32 * (q & 1)) * 16);
  const uint32_t sB0 = (uint32_t)((8 * tn + 2 * w) * nmk) * 3u * kFragBytes;
  const int aoff = (q >> 1) * 64 * 2 + li + 32 * (q & 1);
  const int col0 = 64 * w + li;   // this lane's column of block cb: col0 + 16 cb (within the tile)
  bf16x8 (*sLg)[4 * 2 * 2 * 64] = sL[grp];
  __syncthreads();   // sG
  for (int pass = 0; pass < (G == 1 ? (nT - 1 - p != p ? 2 : 1) : 1); ++pass) {
    const int trun = G == 1 ? (pass ? p : nT - 1 - p) : th;   // the stream's blocks 0 .. trun
    const int t = G == 1 ? trun : own2;                      // this group's row tile (-1: none)
    const bool desc = G == 1 && pass;                        // G = 1, second pass: blocks downwards
    const int S = K * 4 * (trun + 1);                        // pairs of the stream (even)
    // pair s_ of the stream -> (expert k, pair ks, block b)
    auto at = [&](int s_, int& k, int& ks) {
      const int bi = s_ / (4 * K), r = s_ % (4 * K);
      k = r >> 2;
      ks = 4 * (desc ? trun - bi : bi) + (r & 3);
    };
    auto active = [&](int s_) {   // uniform per group: this group's tile needs the pair
      if (G == 1) return true;
      const int bi = s_ / (4 * K);
      return bi <= t;
    };
    auto load_t = [&](u32x4v (&st)[4], int s_) {
      if (!active(s_)) return;
      int k, ks;
      at(s_, k, ks);
      const uint32_t o = (uint32_t)(((int64_t)k * nmb + 4 * t) * nmk + 2 * ks) * 3u * kFragBytes;
#pragma unroll
      for (int u = 0; u < 4; ++u) st[u] = __builtin_amdgcn_raw_buffer_load_b128(img_rsrc(Ltfr, lt_bytes), vT[u], o, 0);
    };
    auto load_b = [&](bf16x8 (&b)[4][3], int s_) {
      if (!active(s_)) return;
      int k, ks;
      at(s_, k, ks);
      const __amdgpu_buffer_rsrc_t rB = img_rsrc(Cfr + (int64_t)k * cexp, c_bytes);
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
          b[cb][pl] = ld_frag(rB, vB, sB0 + (uint32_t)(cb >> 1) * (uint32_t)nmk * 3u * kFragBytes +
                                          (uint32_t)((2 * ks) * 3 + pl) * kFragBytes + (uint32_t)(16 * (cb & 1)) * 16u);
    };
    auto store_t = [&](int buf, const u32x4v (&st)[4], int s_) {
      if (!active(s_)) return;
#pragma unroll
      for (int u = 0; u < 4; ++u) reinterpret_cast<u32x4v*>(sLg[buf])[tid + 256 * u] = st[u];
    };
    floatx4v acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[i][c] = floatx4v{0.f, 0.f, 0.f, 0.f};
    auto compute = [&](int buf, const bf16x8 (&b)[4][3], int s_) {
      if (!active(s_)) return;
#pragma unroll
      for (int ib = 0; ib < 8; ++ib) {
        const int base = (ib >> 1) * 128 * 2 + 16 * (ib & 1) + aoff;
        bf16x8 a[3];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) a[pl] = sLg[buf][base + 64 * pl];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[ib][cb] = mfma16_fmt<2, true>(a, b[cb], acc[ib][cb]);
      }
    };
    // after expert k's 4 pairs of a block: to units of expert (k + 1) % K's weight
    auto rescale = [&](int s_) {
      if (!active(s_)) return;
      const int k = (s_ % (4 * K)) >> 2, kn = k + 1 < K ? k + 1 : 0;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const float r = sG[k * 256 + col0 + 16 * cb] / sG[kn * 256 + col0 + 16 * cb];
#pragma unroll
        for (int ib = 0; ib < 8; ++ib) acc[ib][cb] *= r;
      }
    };
    bf16x8 b0[4][3], b1[4][3];
    u32x4v st[4];
    load_t(st, 0);
    load_b(b0, 0);
    store_t(0, st, 0);
    __syncthreads();
#pragma nounroll
    for (int s_ = 0; s_ < S; s_ += 2) {
      load_t(st, s_ + 1);
      load_b(b1, s_ + 1);
      __builtin_amdgcn_sched_barrier(0);
      compute(0, b0, s_);
      __builtin_amdgcn_sched_barrier(0);
      store_t(1, st, s_ + 1);
      __syncthreads();
      const int s2 = s_ + 2 < S ? s_ + 2 : S - 1;  // after the last pair: harmless reload
      load_t(st, s2);
      load_b(b0, s2);
      __builtin_amdgcn_sched_barrier(0);
      compute(1, b1, s_ + 1);
      __builtin_amdgcn_sched_barrier(0);
      if ((s_ & 3) == 2) rescale(s_ + 1);   // pair s_ + 1 ended the expert's block
      store_t(0, st, s2);
      __syncthreads();
    }
    if (t < 0) continue;   // (G = 2: a group without a row tile; uniform per group, no barrier below)
    // acc is in units of expert 0's weight (the wrap after the last block)
    float gl[4], mx[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      gl[cb] = sG[col0 + 16 * cb] * unscale;
      mx[cb] = 0.f;
    }
    // gA = 2 out + gA0 (rows >= M read 0 outside the resource), column maxima over the tile
    const int64_t i0 = 128 * (int64_t)t;
    const __amdgpu_buffer_rsrc_t r0 =
        __builtin_amdgcn_make_buffer_rsrc((void*)gA0, (short)0, (int)(uint32_t)(M * ld0 * 4), 0x00020000);
    uint32_t ld32 = (uint32_t)ld0;
    // (opaque per pass: otherwise the 128 per-lane epilogue offsets are hoisted out of the
    // pass loop and spilled across the main loop)
    asm volatile("" : "+s"(ld32));
    const uint32_t soff = (uint32_t)((i0 * ld0 + 256 * (int64_t)tn) * 4);
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int nl = col0 + 16 * cb;
      const bool ok = 256 * (int64_t)tn + nl < N;
#pragma unroll
      for (int ib = 0; ib < 8; ++ib)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t rl = (uint32_t)(16 * ib + 4 * q + e);
          const float a0 =
              __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r0, (rl * ld32 + (uint32_t)nl) * 4u, soff, 0));
          const float v = ok ? fmaf(2.f, acc[ib][cb][e] * gl[cb], a0) : 0.f;
          acc[ib][cb][e] = v;
          mx[cb] = fmaxf(mx[cb], fabsf(v));
        }
      mx[cb] = fmaxf(mx[cb], lane_xor16(mx[cb]));
      mx[cb] = fmaxf(mx[cb], lane_xor32(mx[cb]));
      const int64_t n = 256 * (int64_t)tn + nl;
      if (q == 0 && ok) gexp[t * ldc + n] = mx[cb] > 0.f ? (float)img_exp(mx[cb]) : kCexpZero;
    }
    // the split-f16 image at 2^e per column (two factors: e can pass 127): fragment
    // (32-column block 8 tn + 2 w + c, k-step 8 t + ib) from the 16x16 blocks (ib, 2c)
    // and (ib, 2c + 1) through one lane-half exchange (K4's epilogue)
    const bool lo_half = lane < 32;
    const int pos = lo_half ? li + 32 * q : 16 + li + 32 * (q - 2);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int ex = img_exp(lo_half ? mx[2 * c] : mx[2 * c + 1]), ex1 = ex / 2;
      const float sc1 = ldexpf(1.f, ex1), scale = ldexpf(1.f, ex - ex1);
#pragma unroll
      for (int ib = 0; ib < 8; ++ib) {
        float v[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = acc[ib][2 * c][r];
          v[4 + r] = acc[ib][2 * c + 1][r];
          lane_half_swap(v[r], v[4 + r]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= sc1;
        store_split_f16(gAfr + ((((int64_t)8 * tn + 2 * w + c) * nmk + 8 * t + ib) * 3) * 64 + pos, v, scale);
      }
    }
  }
}

// B-d: gKuf = L^-T gA = Linv^T gA as f32 [M][ld]; T image = Linv (lower in
// (k, i)), B image = gA; items and main loop as K5 (one "expert").
__global__ __launch_bounds__(256, 2) void trsm_bwd_kernel(const bf16x8* __restrict__ gAfr,
                                                         const bf16x8* __restrict__ LIfr, uint32_t gafr_bytes,
                                                         uint32_t lifr_bytes, int nmk, int nmb, int nTn,
                                                         int64_t M, int64_t N, float* __restrict__ gKuf,
                                                         int64_t ldk) {
  __shared__ bf16x8 sL[2][4 * 3 * 64];
  int t, tn;
  col_major_item(blockIdx.x, nmk / 8, nTn, t, tn);
  t = nmk / 8 - 1 - t;  // lower T from the diagonal on: row tile 0 is the heaviest
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  floatx16 acc[4][2];
  x6_mainloop<1, 2, 3, false, false, true>(acc, sL, img_rsrc(LIfr, lifr_bytes), (uint32_t)((4 * t) * nmk) * 3u * kFragBytes,
                    img_rsrc(gAfr, gafr_bytes), (uint32_t)((8 * tn + 2 * w) * nmk) * 3u * kFragBytes, 8 * t, nmk, nmk);
  store_acc_f32(acc, gKuf, ldk, 128 * (int64_t)t, (int64_t)tn * kX6BN, M, N, nullptr);
}

// B-d on split-f16 images (MGP_TRSM_BWD16): three f16 products per block instead of
// six bf16 ones.  Linv's image at 2^img_exp(*li_bound); gA's image per (128-row tile
// t', column n) at 2^cexp[t'][n] (grad_a_c_store).  Each lane owns one column of each
// of its two sub-tiles: at the start it takes E = min over the tiles t' >= t it
// contracts of cexp[t'][n] (the largest tile), and every B fragment of tile t' is
// multiplied by 2^(E - cexp[t'][n]) <= 1 in f16 right before its MFMAs, so all
// tiles meet in the accumulator at the common scale 2^E (exact powers of two: the
// product is that of the exactly-scaled image; only parts below 2^-24 of the
// column's largest tile are lost to f16 underflow).  Output unscaled by 2^-(E + eL).
constexpr int kTrsmBwd16MaxT = 32;  // row tiles (M <= 4096); larger M: trsm_bwd_kernel
#ifndef MGP_TRSM_BWD16
#define MGP_TRSM_BWD16 1
#endif
constexpr bool kTrsmBwd16 = MGP_TRSM_BWD16;
#ifndef MGP_GLM_F16
#define MGP_GLM_F16 1
#endif
constexpr bool kGlmF16 = MGP_GLM_F16;
__global__ __launch_bounds__(256, 2) void trsm_bwd16_kernel(const bf16x8* __restrict__ gAfr,
                                                           const bf16x8* __restrict__ LIfr, uint32_t gafr_bytes,
                                                           uint32_t lifr_bytes, int nmk, int nmb, int nTn,
                                                           int64_t M, int64_t N, float* __restrict__ gKuf,
                                                           int64_t ldk, const float* __restrict__ cexp, int64_t ldc,
                                                           const float* __restrict__ li_bound,
                                                           float* __restrict__ gmax) {
  __shared__ bf16x8 sL[2][4 * 3 * 64];
  __shared__ float sF[kTrsmBwd16MaxT][kX6BN];  // per (tile t' - t, column): 2^(E - cexp)
  int t, tn;
  const int nT = nmk / 8;
  col_major_item(blockIdx.x, nT, nTn, t, tn);
  t = nT - 1 - t;  // lower T from the diagonal on: row tile 0 is the heaviest
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  {  // thread = one column of the item
    const int64_t n = (int64_t)tn * kX6BN + threadIdx.x;
    float E = kCexpZero;
    if (n < N)
      for (int tp = t; tp < nT; ++tp) E = fminf(E, cexp[tp * ldc + n]);
    for (int tp = t; tp < nT; ++tp) sF[tp - t][threadIdx.x] = n < N ? exp2f(E - cexp[tp * ldc + n]) : 0.f;
  }
  float E2[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {  // this lane's columns (the accumulators' and the B fragments')
    const int64_t n = (int64_t)tn * kX6BN + 64 * w + 32 * c + (lane & 31);
    float E = kCexpZero;
    if (n < N)
      for (int tp = t; tp < nT; ++tp) E = fminf(E, cexp[tp * ldc + n]);
    E2[c] = E;
  }
  int tcur = -1;
  _Float16 f[2] = {(_Float16)1.f, (_Float16)1.f};
  auto bh = [&](bf16x8 (&b)[2][3], int mk) {
    const int tp = mk >> 3;
    if (tp != tcur) {  // uniform: every 8 k-steps
      tcur = tp;
#pragma unroll
      for (int c = 0; c < 2; ++c) f[c] = (_Float16)sF[tp - t][64 * w + 32 * c + (lane & 31)];
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int p = 0; p < 2; ++p)
        b[c][p] = __builtin_bit_cast(bf16x8, __builtin_bit_cast(halfx8, b[c][p]) * f[c]);
  };
  floatx16 acc[4][2];
  x6_mainloop<1, 2, 2, true, false, true>(acc, sL, img_rsrc(LIfr, lifr_bytes), (uint32_t)((4 * t) * nmk) * 3u * kFragBytes,
                    img_rsrc(gAfr, gafr_bytes), (uint32_t)((8 * tn + 2 * w) * nmk) * 3u * kFragBytes, 8 * t, nmk, nmk,
                    true, bh);
  const int eL = img_exp(*li_bound);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    // 2^-(E + eL) as two factors (E reaches ~160 for a column of tiny values)
    const float x = E2[c] + (float)eL, x1 = floorf(0.5f * x);
    const float u1 = E2[c] >= kCexpZero ? 0.f : exp2f(-x1), u2 = exp2f(x1 - x);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][c][e] = acc[i][c][e] * u1 * u2;
  }
  if (gmax) {  // max |gKuf[m][.]| over this wave's 64 columns per row -> gmax[4 tn + w][m]
    float* dst = gmax + (int64_t)(4 * tn + w) * M;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float m = half_max_f32(fmaxf(fabsf(acc[i][0][e]), fabsf(acc[i][1][e])));
        const int64_t row = 128 * (int64_t)t + 32 * i + acc_row(e, lane);
        if ((lane & 31) == 0 && row < M) dst[row] = m;
      }
  }
  store_acc_f32(acc, gKuf, ldk, 128 * (int64_t)t, (int64_t)tn * kX6BN, M, N, nullptr);
}

// out[m] = max over p < np of part[p][m] (blockIdx.y = 0: A's slab partials into
// out[0 .. M), 1: g_Kuf's wave partials into out[M .. 2M)).  Workgroup: 16 rows x 16
// partial groups (a thread takes partials g, g + 64, ... eight loads in flight), LDS
// (16 rows x 16 groups: 21 us per launch at c3; 64 groups: the loads' latency shared).
__global__ __launch_bounds__(1024) void rowmax_fold_kernel(const float* __restrict__ pa, int npa,
                                                           const float* __restrict__ pg, int npg, int64_t M,
                                                           float* __restrict__ out) {
  __shared__ float sm[64][17];
  const int r = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int64_t m = (int64_t)blockIdx.x * 16 + r;
  const float* p = blockIdx.y ? pg : pa;
  const int np = blockIdx.y ? npg : npa;
  float v = 0.f;
  if (m < M) {
#pragma unroll 8
    for (int q = g; q < np; q += 64) v = fmaxf(v, p[(int64_t)q * M + m]);
  }
  sm[g][r] = v;
  __syncthreads();
  if (threadIdx.x < 16 && m < M) {
    float x = sm[0][r];
#pragma unroll
    for (int k = 1; k < 64; ++k) x = fmaxf(x, sm[k][r]);
    out[blockIdx.y * M + m] = x;
  }
}

}  // namespace mgp

using namespace mgp;

// ------------------------------------------------------------------ conditional backward (x6)

constexpr int kRowSumChunks = 32;  // column chunks of row_sums_kernel

namespace {
struct CondBwdWs {  // workspace carve-up (256-B aligned pieces)
  size_t sfr, ga0, rimg, qpart, gafr, lifr, P, LT, part, bnd, cexp, rmax, rpart, gram, total;
};
size_t al256(size_t x) { return (x + 255) / 256 * 256; }
CondBwdWs cond_bwd_layout(int64_t M, int64_t N, int32_t K) {
  CondBwdWs w;
  const int64_t ldn = (N + 3) / 4 * 4;
  size_t o = 0;
  const int64_t ldm = (M + 3) / 4 * 4;
  w.sfr = o;  o += al256(mgp_x6_lower_bytes(M, K));
  // gA0 (read last by step 3), then A's row image for the P_k gram (step 5)
  w.ga0 = o;  o += al256(std::max((size_t)M * ldn * 4, mgp_rows_f16_bytes(M, N)));
  // A's row image written beside gA0 by grad_a_prep_kernel (split-f16), its g_q_mu partials
  w.rimg = o; o += al256(mgp_rows_f16_bytes(M, N));
  w.qpart = o; o += al256((size_t)((mgp_rows_f16_ksteps(N) + 7) / 8) * M * K * 4);
  w.gafr = o; o += al256(mgp_x6_cols_bytes(M, N));
  w.lifr = o; o += al256(mgp_x6_lower_bytes(M, 1));
  w.P = o;    o += al256((size_t)K * M * ldm * 4);
  w.LT = o;   o += al256((size_t)K * M * ldm * 4);
  w.part = o; o += al256((size_t)K * kRowSumChunks * 8);  // row_sums partials
  w.bnd = o;  o += 256;  // split-f16 bounds: max |Gv|, max |LinvT| (MGP_TRSM_BWD16)
  w.cexp = o; o += al256((size_t)((M + 127) / 128) * ldn * 4);  // gA image scales per (row tile, column)
  w.rmax = o; o += al256((size_t)2 * M * 4);  // row maxima of A and g_Kuf (the f16 g_Lm gram)
  // their partials: per slab of 128 n (grad_a_prep), per 64 columns (trsm_bwd16)
  w.rpart = o; o += al256((size_t)(mgp_rows_f16_ksteps(N) / 8 + 1 + (N + 63) / 64 + 4) * M * 4);
  w.gram = o;
  size_t g = mgp_gram_x6_workspace_bytes(M, M, N, K, 2);
  g = g > mgp_gram_x6_workspace_bytes(M, M, M, K, 2) ? g : mgp_gram_x6_workspace_bytes(M, M, M, K, 2);
  const size_t sizes[3] = {mgp_gram_x6_workspace_bytes(M, M, M, K, 1), mgp_gram_x6_workspace_bytes(M, M, N, 1, 1),
                           mgp_gram_workspace_bytes(M, K, N, 0)};
  for (size_t v : sizes) g = v > g ? v : g;
  o += al256(g);
  w.total = o;
  return w;
}
}  // namespace

// part[k][c] = sum of x[k][n] over column chunk c (grid: rows x kRowSumChunks), then
// out = sum of all parts (fixed order).
__global__ __launch_bounds__(256) void row_sums_kernel(const float* __restrict__ x, int64_t cols, int64_t ld,
                                                       double* __restrict__ part) {
  __shared__ double scratch[16];
  const float* row = x + (int64_t)blockIdx.x * ld;
  const int64_t per = (cols + kRowSumChunks - 1) / kRowSumChunks;
  const int64_t nb = (int64_t)blockIdx.y * per, ne = nb + per < cols ? nb + per : cols;
  double v = 0.0;
  for (int64_t n = nb + threadIdx.x; n < ne; n += 256) v += (double)row[n];
  v = mgp::block_sum<double>(v, scratch);
  if (threadIdx.x == 0) part[blockIdx.x * kRowSumChunks + blockIdx.y] = v;
}

// out = sum of part[0 .. rows) in index order (one wave stages the partials in LDS,
// lane 0 adds them: the single-thread loop over global memory took 16 us)
constexpr int kSumPartsMax = 16 * kRowSumChunks;
__global__ __launch_bounds__(64) void sum_parts_kernel(const double* __restrict__ part, int rows,
                                                       double* __restrict__ out) {
  __shared__ double sp[kSumPartsMax];
  for (int i = threadIdx.x; i < rows; i += 64) sp[i] = part[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = 0.0;
#pragma unroll 8
    for (int k = 0; k < rows; ++k) v += sp[k];
    *out = v;
  }
}

// T[k][i][j] = L_k[i][j] for j <= i, else 0 (the lower triangle of q_sqrt).
__global__ __launch_bounds__(256) void tril_copy_kernel(const float* __restrict__ q, int64_t ldq, int64_t sq,
                                                        int64_t M, float* __restrict__ T, int64_t ldt, int64_t st) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * M) return;
  const int k = blockIdx.y;
  const int64_t i = idx / M, j = idx % M;
  T[k * st + i * ldt + j] = j <= i ? q[k * sq + i * ldq + j] : 0.f;
}

// LT[k][j][l] = L_k[l][j] for l >= j, else 0 (the transposed lower triangle of q_sqrt).
__global__ __launch_bounds__(256) void tril_transpose_kernel(const float* __restrict__ q, int64_t ldq, int64_t sq,
                                                             int64_t M, float* __restrict__ LT, int64_t ldt,
                                                             int64_t st) {
  __shared__ float tile[32][33];
  const int k = blockIdx.z;
  const int64_t r0 = (int64_t)blockIdx.y * 32, c0 = (int64_t)blockIdx.x * 32;  // source rows l, columns j
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int y = ty; y < 32; y += 8) {
    const int64_t l = r0 + y, j = c0 + tx;
    tile[y][tx] = (l < M && j < M && l >= j) ? q[k * sq + l * ldq + j] : 0.f;
  }
  __syncthreads();
  for (int y = ty; y < 32; y += 8) {
    const int64_t j = c0 + y, l = r0 + tx;
    if (j < M && l < M) LT[k * st + j * ldt + l] = tile[tx][y];
  }
}

extern "C" size_t mgp_conditional_backward_workspace_bytes(int64_t M, int64_t N, int32_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 256;
  return cond_bwd_layout(M, N, K).total;
}

static int conditional_backward(
    const void* Afr, size_t afr_bytes, const float* A, int64_t lda,
    const float* q_sqrt, int64_t ldqs, int64_t strideq, const float* q_mu, int64_t ldq, const float* LinvT,
    int64_t ldl, const float* Gmu, const float* Gv, int64_t ldg, int64_t M, int64_t N, int32_t K,
    float* g_q_mu, int64_t ldgq, float* g_q_sqrt, int64_t ldgs, int64_t strideg, float* g_Kuf, int64_t ldk,
    float* g_Lm, int64_t ldgl, double* g_var, void* workspace, size_t workspace_bytes, mgp_stream_t stream,
    bool f16, bool x8 = false, const void* Cfr = nullptr, size_t cfr_bytes = 0, const float* colmax = nullptr,
    const float* l_bound = nullptr, const void* qprep = nullptr, const float* t_bound = nullptr) {
  if (!Afr) return -1;
  if (afr_bytes < mgp_x6_cols_bytes(M, N)) return -2;
  if (!A) return -3;
  if (lda < N) return -4;
  if (!q_sqrt) return -7;
  if (ldqs < M) return -8;
  if (!q_mu) return -10;
  if (ldq < K) return -11;
  if (!LinvT) return -12;
  if (ldl < M) return -13;
  if (!Gmu) return -14;
  if (!Gv) return -15;
  if (ldg < N) return -16;
  if (M <= 0) return -17;
  if (N <= 0) return -18;
  if (K < 1) return -19;
  if (K > 16) return MGP_ERR_UNSUPPORTED;
  if (!g_q_mu) return -20;
  if (!g_q_sqrt) return -22;
  if (!g_Kuf) return -25;
  if (!g_Lm) return -27;
  if (!g_var) return -29;
  if (!workspace || workspace_bytes < mgp_conditional_backward_workspace_bytes(M, N, K)) return MGP_ERR_WORKSPACE;
  if (!aligned16(workspace) || !aligned16(Afr)) return MGP_ERR_ALIGN;
  // A and g_Kuf are operands of the grams over N (float4 rows) and Gv their weights, one
  // expert every ldg floats: refused here, before anything is launched, not by the grams
  // (with their own argument numbers, and g_Kuf already written)
  if (lda % 4 || ldk % 4 || (K > 1 && ldg % 4) || !aligned16(A) || !aligned16(Gv) || !aligned16(g_Kuf))
    return MGP_ERR_ALIGN;
  const size_t img = mgp_x6_cols_bytes(M, N);
  if (img >= ((size_t)1 << 32) || (size_t)M * ((N + 3) / 4 * 4) * 4 >= ((size_t)1 << 32)) return MGP_ERR_UNSUPPORTED;
  // the S_k / L_k image is addressed through one 32-bit buffer resource by the gA kernels
  if (lower_planes(M, K) >= ((size_t)1 << 32)) return MGP_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const CondBwdWs L = cond_bwd_layout(M, N, K);
  char* ws = (char*)workspace;
  const int64_t ldn = (N + 3) / 4 * 4;
  float* P = (float*)(ws + L.P);
  float* LT = qprep ? (float*)((char*)const_cast<void*>(qprep) + al256(mgp_x6_lower_bytes(M, K))) : (float*)(ws + L.LT);
  double* part = (double*)(ws + L.part);
  const int64_t ldm = (M + 3) / 4 * 4;
  // qprep (mgp_conditional_backward_prep_f16c, the C path only): L_k's image and the
  // transposed triangles already formed from q_sqrt, e.g. beside the forward's K3
  bf16x8* Sfr = qprep ? (bf16x8*)const_cast<void*>(qprep) : (bf16x8*)(ws + L.sfr);
  float* gA0 = (float*)(ws + L.ga0);
  bf16x8* gAfr = (bf16x8*)(ws + L.gafr);
  bf16x8* LIfr = (bf16x8*)(ws + L.lifr);
  void* gws = ws + L.gram;
  const size_t gwsb = L.total - L.gram;
  const int64_t Mp = x6_mp(M);
  const int nmk = (int)(Mp / 16), nmb = (int)(Mp / 32), nT = (int)(Mp / kX6BM);
  const int nTn = (int)(x6_np(N) / kX6BN);
  int st;
  const bool cpath = f16 && !x8 && Cfr;  // B-b from the forward's C_k images
  // B-d on split-f16 images (trsm_bwd16_kernel): the C path, M <= 4096
  const bool bwd16 = kTrsmBwd16 && cpath && nT <= kTrsmBwd16MaxT;
  // max |LinvT| given (t_bound: the forward's L^-T image bound from K3) or formed here
  float* li_bound = t_bound ? const_cast<float*>(t_bound) : (float*)(ws + L.bnd) + 1;
  float* cexp = (float*)(ws + L.cexp);
  if (cpath) {
    if (!colmax || !l_bound) return -32;
    if (cfr_bytes < mgp_c_images_bytes(M, N, K)) return -31;
    if ((int64_t)K * ldg * 4 >= ((int64_t)1 << 32)) return MGP_ERR_UNSUPPORTED;  // grad_a_c's Gv resource
    if (!aligned16(Cfr)) return MGP_ERR_ALIGN;
    // L_k's image (rows m, k-steps over m' <= m) into the S image's space; Linv's image
    const int64_t nfrag = (int64_t)K * nmb * nmk, nf1 = (int64_t)nmb * nmk;
    if (!qprep) launch_split_tri(TriImage::kUpperTrans, q_sqrt, ldqs, strideq, M, nmb, nmk, nfrag, Sfr, l_bound, s);
    if (bwd16 && !t_bound) {  // Linv's split-f16 image at max |LinvT| (its upper triangle)
      if ((st = hip_status(hipMemsetAsync(li_bound, 0, sizeof(float), s)))) return st;
      launch_absmax_tri(AbsTri::kUpper, LinvT, ldl, (int64_t)0, M, M, M, li_bound, s);
    }
    launch_split_tri(TriImage::kLowerTrans, LinvT, ldl, (int64_t)0, M, nmb, nmk, nf1, LIfr,
                     bwd16 ? (const float*)li_bound : nullptr, s);
    if ((st = launch_status())) return st;
  } else {
  // 1. S_k = L_k L_k^T (x6 gram over M of tril(q_sqrt), into the LT buffer) and its
  //    full split images; the image of Linv (T operand of B-d)
  hipLaunchKernelGGL(tril_copy_kernel, dim3((unsigned)((M * M + 255) / 256), (unsigned)K), dim3(256), 0, s, q_sqrt,
                     ldqs, strideq, M, P, ldm, M * ldm);
  if ((st = launch_status())) return st;
  st = mgp_gram_x6(P, ldm, M * ldm, M, P, ldm, M * ldm, M, nullptr, 0, M, K, 1.f, 2, LT, ldm, M * ldm, gws, gwsb,
                   stream);
  if (st) return st;
  {
    const int64_t nfrag = (int64_t)K * nmb * nmk;
    float* s_bound = trailer(Sfr, lower_planes(M, K));
    if (f16) {  // max |S_k| over the experts into the image trailer, then the scaled split
      if ((st = hip_status(hipMemsetAsync(s_bound, 0, sizeof(float), s)))) return st;
      launch_absmax_tri(AbsTri::kAll, LT, ldm, M * ldm, M, M, (int64_t)K * M, s_bound, s);
    }
    launch_split_tri(TriImage::kLowerFull, LT, ldm, M * ldm, M, nmb, nmk, nfrag, Sfr,
                     f16 ? (const float*)s_bound : nullptr, s);
    const int64_t nf1 = (int64_t)nmb * nmk;
    launch_split_tri(TriImage::kLowerTrans, LinvT, ldl, (int64_t)0, M, nmb, nmk, nf1, LIfr, nullptr, s);
    if ((st = launch_status())) return st;
  }
  }
  // 2. gA0 = q_mu G_mu - 2 A sum_k Gv_k; split-f16: with A's row image (step 5) and
  //    g_q_mu's partials (step 6) in the same pass over A
  const float* a_bound = trailer(const_cast<void*>(Afr), cols_planes(M, N));
  bf16x8* rimg = (bf16x8*)(ws + L.rimg);
  float* qpart = (float*)(ws + L.qpart);
  const int nns = (int)mgp_rows_f16_ksteps(N);
  const int slabs = (nns + 7) / 8;
  const bool prep = f16 && lda % 4 == 0 && aligned16(A);  // else grad_a_base, split_rows_f16, gram_narrow
  // g_Lm on f16 products with exact per-row scales (MGP_GLM_F16): the row maxima of A
  // (grad_a_prep) and of g_Kuf (trsm_bwd16) by atomics
  const bool glm16 = kGlmF16 && bwd16 && prep;
  float* rmaxA = (float*)(ws + L.rmax);
  float* rmaxG = rmaxA + M;
  float* rpartA = glm16 ? (float*)(ws + L.rpart) : nullptr;
  float* rpartG = glm16 ? rpartA + (int64_t)slabs * M : nullptr;
  if (prep) {
    const int rbs = kPrepRB;
    const dim3 grid((unsigned)slabs, (unsigned)((M + 32 * rbs - 1) / (32 * rbs)));
    const int qvec = (ldq % 4 == 0 && K % 4 == 0 && aligned16(q_mu)) ? 1 : 0;
    if (K <= 4)
      hipLaunchKernelGGL(grad_a_prep_kernel<4>, grid, dim3(256), 0, s, A, lda, q_mu, ldq, Gmu, Gv, ldg, M, N, K, nns,
                         a_bound, gA0, ldn, rimg, qpart, rbs, qvec, rpartA);
    else if (K <= 8)
      hipLaunchKernelGGL(grad_a_prep_kernel<8>, grid, dim3(256), 0, s, A, lda, q_mu, ldq, Gmu, Gv, ldg, M, N, K, nns,
                         a_bound, gA0, ldn, rimg, qpart, rbs, qvec, rpartA);
    else
      hipLaunchKernelGGL(grad_a_prep_kernel<16>, grid, dim3(256), 0, s, A, lda, q_mu, ldq, Gmu, Gv, ldg, M, N, K, nns,
                         a_bound, gA0, ldn, rimg, qpart, rbs, qvec, rpartA);
    if ((st = launch_status())) return st;
  } else {
    const int rows = 128;
    const dim3 grid((unsigned)((N + 255) / 256), (unsigned)((M + rows - 1) / rows));
    if (K <= 4)
      hipLaunchKernelGGL(grad_a_base_kernel<4>, grid, dim3(256), 0, s, A, lda, q_mu, ldq, Gmu, Gv, ldg, M, N, K, rows,
                         gA0, ldn);
    else if (K <= 8)
      hipLaunchKernelGGL(grad_a_base_kernel<8>, grid, dim3(256), 0, s, A, lda, q_mu, ldq, Gmu, Gv, ldg, M, N, K, rows,
                         gA0, ldn);
    else
      hipLaunchKernelGGL(grad_a_base_kernel<16>, grid, dim3(256), 0, s, A, lda, q_mu, ldq, Gmu, Gv, ldg, M, N, K,
                         rows, gA0, ldn);
    if ((st = launch_status())) return st;
  }
  // 3. gA (image) = 2 sum_k (S_k A) diag(Gv_k) + gA0  (C path: 2 sum_k L_k C_k diag(Gv_k) + gA0)
  if (cpath && kGac16 && bwd16 && K <= kGac16KMax)
    hipLaunchKernelGGL(grad_a_c16_kernel<kGac16G>, dim3((unsigned)((nT + 1) / 2 * nTn)), dim3(256 * kGac16G), 0, s,
                       (const bf16x8*)Sfr,
                       (uint32_t)lower_planes(M, K), (const bf16x8*)Cfr, (int64_t)(cols_planes(M, N) / 16),
                       (uint32_t)cols_planes(M, N), nmk, nTn, K, M, N, Gv, ldg, gA0, ldn, gAfr, l_bound,
                       (const float*)trailer(const_cast<void*>(Afr), cols_planes(M, N)), colmax, cexp, ldn);
  else if (cpath)
    hipLaunchKernelGGL((grad_a_c_kernel<kGacPD, kGacNC>), dim3((unsigned)((nT + 1) / 2 * (2 / kGacNC) * nTn)), dim3(256), 0, s,
                       (const bf16x8*)Sfr, (uint32_t)lower_planes(M, K), (const bf16x8*)Cfr,
                       (int64_t)(cols_planes(M, N) / 16), (uint32_t)cols_planes(M, N), nmk, (2 / kGacNC) * nTn, K, M, N, Gv, ldg, gA0, ldn, gAfr, l_bound,
                       (const float*)trailer(const_cast<void*>(Afr), cols_planes(M, N)), colmax,
                       bwd16 ? cexp : nullptr, ldn);
  else if (f16 && x8)
    hipLaunchKernelGGL((grad_a_s_kernel<true, true>), dim3((unsigned)(nT * 2 * nTn)), dim3(256), 0, s,
                       (const bf16x8*)Sfr, (uint32_t)mgp_x6_lower_bytes(M, 1), (const bf16x8*)Afr, (uint32_t)afr_bytes,
                       nmk, 2 * nTn, K, M, N, Gv, ldg, gA0, ldn, gAfr, (const float*)trailer(Sfr, lower_planes(M, K)),
                       (const float*)trailer(const_cast<void*>(Afr), cols_planes(M, N)));
  else if (f16)
    hipLaunchKernelGGL(grad_a_s_f16_kernel, dim3((unsigned)(nT * 2 * nTn)), dim3(256), 0, s, (const bf16x8*)Sfr,
                       (uint32_t)lower_planes(M, K), (const bf16x8*)Afr, (uint32_t)afr_bytes, nmk, 2 * nTn, K, M, N,
                       Gv, ldg, gA0, ldn, gAfr, (const float*)trailer(Sfr, lower_planes(M, K)),
                       (const float*)trailer(const_cast<void*>(Afr), cols_planes(M, N)));
  else
    hipLaunchKernelGGL(grad_a_s_kernel<false>, dim3((unsigned)(nT * 2 * nTn)), dim3(256), 0, s, (const bf16x8*)Sfr,
                       (uint32_t)mgp_x6_lower_bytes(M, 1), (const bf16x8*)Afr, (uint32_t)afr_bytes, nmk, 2 * nTn, K,
                       M, N, Gv, ldg, gA0, ldn, gAfr, nullptr, nullptr);
  if ((st = launch_status())) return st;
  // 4. gKuf = Linv^T gA
  if (bwd16)
    hipLaunchKernelGGL(trsm_bwd16_kernel, dim3((unsigned)(nT * nTn)), dim3(256), 0, s, (const bf16x8*)gAfr,
                       (const bf16x8*)LIfr, (uint32_t)img, (uint32_t)mgp_x6_lower_bytes(M, 1), nmk, nmb, nTn, M, N,
                       g_Kuf, ldk, (const float*)cexp, ldn, (const float*)li_bound, rpartG);
  else
  hipLaunchKernelGGL(trsm_bwd_kernel, dim3((unsigned)(nT * nTn)), dim3(256), 0, s, (const bf16x8*)gAfr,
                     (const bf16x8*)LIfr, (uint32_t)img, (uint32_t)mgp_x6_lower_bytes(M, 1), nmk, nmb, nTn, M, N, g_Kuf,
                     ldk);
  if ((st = launch_status())) return st;
  // 5. g_q_sqrt[k] = 2 tril(A diag(Gv_k) (L_k^T A)^T) = 2 tril(P_k L_k), P_k = A diag(Gv_k) A^T
  //    (x6 grams over N, then over M with the transposed triangle of L_k); f16: the
  //    grams over N on f16 products, bounds |A| <= sqrt(var) (Afr's trailer), max |Gv|
  float* bnd = (float*)(ws + L.bnd);
  if (f16) {
    if ((st = hip_status(hipMemsetAsync(bnd, 0, sizeof(float), s)))) return st;
    launch_absmax_tri(AbsTri::kAll, Gv, ldg, (int64_t)0, (int64_t)K, N, (int64_t)K, bnd, s);
    if ((st = launch_status())) return st;
    // A's row image (step 2) as the grams' unweighted side
    if (!prep && (st = mgp_split_rows_f16(A, lda, M, N, a_bound, rimg, mgp_rows_f16_bytes(M, N), stream))) return st;
    st = mgp_gram_f16_rows(rimg, mgp_rows_f16_bytes(M, N), M, A, lda, M, Gv, ldg, N, K, 1.f, 2, P, ldm, M * ldm,
                           a_bound, a_bound, bnd, gws, gwsb, stream);
  } else {
    st = mgp_gram_x6(A, lda, 0, M, A, lda, 0, M, Gv, ldg, N, K, 1.f, 2, P, ldm, M * ldm, gws, gwsb, stream);
  }
  if (st) return st;
  if (!(cpath && qprep)) {
    hipLaunchKernelGGL(tril_transpose_kernel, dim3((unsigned)((M + 31) / 32), (unsigned)((M + 31) / 32), (unsigned)K),
                       dim3(256), 0, s, q_sqrt, ldqs, strideq, M, LT, ldm, M * ldm);
    if ((st = launch_status())) return st;
  }
  st = mgp_gram_x6(P, ldm, M * ldm, M, LT, ldm, M * ldm, M, nullptr, 0, M, K, 2.f, 1, g_q_sqrt, ldgs, strideg, gws,
                   gwsb, stream);
  if (st) return st;
  // 6. g_Lm = -tril(g_Kuf A^T), g_q_mu = A G_mu^T, g_var = sum G_v.  g_Lm stays x6 in
  //    both modes: it feeds the near-cancelling Z / lengthscale / variance gradients
  //    through the Cholesky backward (split-f16 operands measured 3.6e-4 normwise on a
  //    lengthscale gradient where float32 autograd is 2.2e-4)
  //    (the C path with MGP_GLM_F16: f16 products, every row of g_Kuf and of A split at
  //    its own exact scale -- the global-bound split was what lost the accuracy)
  if (glm16) {
    hipLaunchKernelGGL(rowmax_fold_kernel, dim3((unsigned)((M + 15) / 16), 2), dim3(1024), 0, s, rpartA, slabs,
                       rpartG, 4 * nTn, M, rmaxA);
    if ((st = launch_status())) return st;
  }
  if (glm16)
    st = gram_f16_rowscaled(g_Kuf, ldk, M, A, lda, M, N, -1.f, 1, g_Lm, ldgl, (const float*)rmaxG,
                            (const float*)rmaxA, gws, gwsb, stream);
  else
    st = mgp_gram_x6(g_Kuf, ldk, 0, M, A, lda, 0, M, nullptr, 0, N, 1, -1.f, 1, g_Lm, ldgl, M * ldgl, gws, gwsb,
                     stream);
  if (st) return st;
  if (prep) {  // g_q_mu from step 2's partials
    hipLaunchKernelGGL(prep_fold_kernel, dim3((unsigned)((M * K + 15) / 16)), dim3(256), 0, s, qpart, slabs, M, K,
                       g_q_mu, ldgq);
  } else {
    st = mgp_gram(A, lda, M, Gmu, ldg, K, N, 1.f, 0, g_q_mu, ldgq, gws, gwsb, stream);
    if (st) return st;
  }
  hipLaunchKernelGGL(row_sums_kernel, dim3((unsigned)K, kRowSumChunks), dim3(256), 0, s, Gv, N, ldg, part);
  hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(64), 0, s, part, (int)K * kRowSumChunks, g_var);
  return launch_status();
}

extern "C" int mgp_conditional_backward_x6(
    const void* Afr, size_t afr_bytes, const float* A, int64_t lda,
    const float* q_sqrt, int64_t ldqs, int64_t strideq, const float* q_mu, int64_t ldq, const float* LinvT,
    int64_t ldl, const float* Gmu, const float* Gv, int64_t ldg, int64_t M, int64_t N, int32_t K,
    float* g_q_mu, int64_t ldgq, float* g_q_sqrt, int64_t ldgs, int64_t strideg, float* g_Kuf, int64_t ldk,
    float* g_Lm, int64_t ldgl, double* g_var, void* workspace, size_t workspace_bytes, mgp_stream_t stream) {
  return conditional_backward(Afr, afr_bytes, A, lda, q_sqrt, ldqs, strideq, q_mu, ldq, LinvT, ldl, Gmu, Gv, ldg, M,
                              N, K, g_q_mu, ldgq, g_q_sqrt, ldgs, strideg, g_Kuf, ldk, g_Lm, ldgl, g_var, workspace,
                              workspace_bytes, stream, false);
}

// Afr is A's split-f16 image (mgp_trsm_stats_f16); S_k = L_k L_k^T is split the same
// way, so the S_k A product (B-b) runs on three f16 products per block.
extern "C" int mgp_conditional_backward_f16(
    const void* Afr, size_t afr_bytes, const float* A, int64_t lda,
    const float* q_sqrt, int64_t ldqs, int64_t strideq, const float* q_mu, int64_t ldq, const float* LinvT,
    int64_t ldl, const float* Gmu, const float* Gv, int64_t ldg, int64_t M, int64_t N, int32_t K,
    float* g_q_mu, int64_t ldgq, float* g_q_sqrt, int64_t ldgs, int64_t strideg, float* g_Kuf, int64_t ldk,
    float* g_Lm, int64_t ldgl, double* g_var, void* workspace, size_t workspace_bytes, mgp_stream_t stream) {
  return conditional_backward(Afr, afr_bytes, A, lda, q_sqrt, ldqs, strideq, q_mu, ldq, LinvT, ldl, Gmu, Gv, ldg, M,
                              N, K, g_q_mu, ldgq, g_q_sqrt, ldgs, strideg, g_Kuf, ldk, g_Lm, ldgl, g_var, workspace,
                              workspace_bytes, stream, true);
}

// mgp_conditional_backward_f16 with the forward's C_k images (mgp_expert_conditional_f16c
// with the same Afr, q_sqrt and colmax; l_bound = the bound of its Lfr image):
// B-b as 2 sum_k L_k C_k diag(Gv_k), no S_k = L_k L_k^T.
extern "C" int mgp_conditional_backward_f16c(
    const void* Afr, size_t afr_bytes, const float* A, int64_t lda,
    const float* q_sqrt, int64_t ldqs, int64_t strideq, const float* q_mu, int64_t ldq, const float* LinvT,
    int64_t ldl, const float* Gmu, const float* Gv, int64_t ldg, int64_t M, int64_t N, int32_t K,
    float* g_q_mu, int64_t ldgq, float* g_q_sqrt, int64_t ldgs, int64_t strideg, float* g_Kuf, int64_t ldk,
    float* g_Lm, int64_t ldgl, double* g_var, void* workspace, size_t workspace_bytes, const void* Cfr,
    size_t cfr_bytes, const float* colmax, const float* l_bound, mgp_stream_t stream) {
  if (!Cfr) return -30;
  return conditional_backward(Afr, afr_bytes, A, lda, q_sqrt, ldqs, strideq, q_mu, ldq, LinvT, ldl, Gmu, Gv, ldg, M,
                              N, K, g_q_mu, ldgq, g_q_sqrt, ldgs, strideg, g_Kuf, ldk, g_Lm, ldgl, g_var, workspace,
                              workspace_bytes, stream, true, false, Cfr, cfr_bytes, colmax, l_bound);
}

// The q_sqrt-only part of mgp_conditional_backward_f16c -- L_k's image (the B-b operand,
// scale l_bound: the bound of the forward's Lfr image) and the transposed triangles
// L_k^T (B-d's operand) -- into prep, so that it can run off the backward's critical
// path (the Python host: on the side stream beside the forward's K3).
extern "C" size_t mgp_conditional_backward_prep_bytes(int64_t M, int32_t K) {
  if (M <= 0 || K <= 0) return 256;
  const int64_t ldm = (M + 3) / 4 * 4;
  return al256(mgp_x6_lower_bytes(M, K)) + al256((size_t)K * M * ldm * 4);
}

extern "C" int mgp_conditional_backward_prep_f16c(const float* q_sqrt, int64_t ldqs, int64_t strideq, int64_t M,
                                                  int32_t K, const float* l_bound, void* prep, size_t prep_bytes,
                                                  mgp_stream_t stream) {
  if (!q_sqrt) return -1;
  if (ldqs < M) return -2;
  if (K > 1 && strideq < ldqs * M) return -3;
  if (M <= 0) return -4;
  if (K < 1) return -5;
  if (K > 16) return MGP_ERR_UNSUPPORTED;
  if (!l_bound) return -6;
  if (!prep) return -7;
  if (prep_bytes < mgp_conditional_backward_prep_bytes(M, K)) return MGP_ERR_WORKSPACE;
  if (!aligned16(prep)) return MGP_ERR_ALIGN;
  if (lower_planes(M, K) >= ((size_t)1 << 32)) return MGP_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int64_t Mp = x6_mp(M), ldm = (M + 3) / 4 * 4;
  const int nmk = (int)(Mp / 16), nmb = (int)(Mp / 32);
  const int64_t nfrag = (int64_t)K * nmb * nmk;
  float* LT = (float*)((char*)prep + al256(mgp_x6_lower_bytes(M, K)));
  // (full grids: the capped grid-stride form of the ELBO's q_sqrt launches measured slower here,
  // training step 14.02-14.11 vs 13.98-14.01 ms, profiles/r06w_side_grid_ab.log)
  launch_split_tri(TriImage::kUpperTrans, q_sqrt, ldqs, strideq, M, nmb, nmk, nfrag, (bf16x8*)prep, l_bound, s);
  hipLaunchKernelGGL(tril_transpose_kernel, dim3((unsigned)((M + 31) / 32), (unsigned)((M + 31) / 32), (unsigned)K),
                     dim3(256), 0, s, q_sqrt, ldqs, strideq, M, LT, ldm, M * ldm);
  return launch_status();
}

// mgp_conditional_backward_f16c on a prep of the same q_sqrt and l_bound
// (mgp_conditional_backward_prep_f16c): two launches fewer, the same results.
extern "C" int mgp_conditional_backward_f16c_prepped(
    const void* Afr, size_t afr_bytes, const float* A, int64_t lda,
    const float* q_sqrt, int64_t ldqs, int64_t strideq, const float* q_mu, int64_t ldq, const float* LinvT,
    int64_t ldl, const float* Gmu, const float* Gv, int64_t ldg, int64_t M, int64_t N, int32_t K,
    float* g_q_mu, int64_t ldgq, float* g_q_sqrt, int64_t ldgs, int64_t strideg, float* g_Kuf, int64_t ldk,
    float* g_Lm, int64_t ldgl, double* g_var, void* workspace, size_t workspace_bytes, const void* Cfr,
    size_t cfr_bytes, const float* colmax, const float* l_bound, const void* prep, size_t prep_bytes,
    const float* t_bound, mgp_stream_t stream) {
  if (!Cfr) return -30;
  if (!prep) return -33;
  if (prep_bytes < mgp_conditional_backward_prep_bytes(M, K)) return -34;
  if (!aligned16(prep)) return MGP_ERR_ALIGN;
  return conditional_backward(Afr, afr_bytes, A, lda, q_sqrt, ldqs, strideq, q_mu, ldq, LinvT, ldl, Gmu, Gv, ldg, M,
                              N, K, g_q_mu, ldgq, g_q_sqrt, ldgs, strideg, g_Kuf, ldk, g_Lm, ldgl, g_var, workspace,
                              workspace_bytes, stream, true, false, Cfr, cfr_bytes, colmax, l_bound, prep, t_bound);
}

// Afr from mgp_trsm_stats_f16x8 with the f32 A (all three planes): S_k A on f16 hi
// products + e4m3 cross terms (grad_a_s_kernel<true, true>).
extern "C" int mgp_conditional_backward_f16x8(
    const void* Afr, size_t afr_bytes, const float* A, int64_t lda,
    const float* q_sqrt, int64_t ldqs, int64_t strideq, const float* q_mu, int64_t ldq, const float* LinvT,
    int64_t ldl, const float* Gmu, const float* Gv, int64_t ldg, int64_t M, int64_t N, int32_t K,
    float* g_q_mu, int64_t ldgq, float* g_q_sqrt, int64_t ldgs, int64_t strideg, float* g_Kuf, int64_t ldk,
    float* g_Lm, int64_t ldgl, double* g_var, void* workspace, size_t workspace_bytes, mgp_stream_t stream) {
  return conditional_backward(Afr, afr_bytes, A, lda, q_sqrt, ldqs, strideq, q_mu, ldq, LinvT, ldl, Gmu, Gv, ldg, M,
                              N, K, g_q_mu, ldgq, g_q_sqrt, ldgs, strideg, g_Kuf, ldk, g_Lm, ldgl, g_var, workspace,
                              workspace_bytes, stream, true, true);
}
