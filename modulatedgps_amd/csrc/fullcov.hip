// Full-covariance whitened SVGP conditional (full_cov=True predictions).
//
// Reference: GPflow 2.7 base_conditional(Kmn, Kmm, Knn, f, full_cov=True, q_sqrt,
// white=True), reached from MixtureGPs/models.py:133-143 with
// Knn = self.kernel(Xnew, full_cov=True):
//     A    = triangular_solve(Lm, Kmn)                       [M, N]
//     fvar = Knn - A^T A                                     [N, N]
//     LTA  = matmul(band_part(q_sqrt, -1, 0), A, transpose_a=True)   [K, M, N]
//     fvar = fvar + LTA^T LTA                                [K, N, N]
// A comes from K4 (mgp_trsm_stats / mgp_trsm_stats_x6 / mgp_trsm_stats_f16 with an A
// buffer); this file adds the two products that scale with N^2:
//   stage 1  C_k = L_k^T A into the workspace [K][M][ldw]: an upper-triangular GEMM per
//            expert (workgroup = expert k x 128 rows m' x 128 columns n; the k-range
//            m < m' tile start lies in L_k's zero triangle and is skipped);
//   stage 2  one workgroup per LOWER-triangle 128 x 128 output tile (ti >= tj): the
//            shared G = A^T A tile once, Knn from X in the epilogue (squared distance as
//            a sum of squared differences: exactly var on the diagonal), then per expert
//            H_k = C_k^T C_k and cov[k] = (Knn - G) + H_k written to the tile and its
//            mirror.  G is computed once for all K experts and only half the tiles are
//            computed: (K + 1) / 2 M N^2 MFMA flops instead of 2 K M N^2.  Tiles that do
//            not fill a round of the CUs are cut by expert over several workgroups
//            (fc_split), each forming G itself.
// Only elements i >= j are taken from the accumulators (the mirror is a copy, also
// inside diagonal tiles), so cov[k] is bitwise symmetric.
//
// gfx950 mapping: 256 threads = 4 waves as 2 x 2, wave tile 64 x 64 = 2 x 2 accumulators
// of v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation; 157 TFLOP/s peak).
// Both operands of every product are k-major ([k][column], the layout of A, C_k and
// q_sqrt), staged in 16-row chunks global -> registers -> LDS (double buffered, one
// barrier per chunk).  Every global access is guarded (any N, M).
#include <algorithm>

#include "mgp_common.hpp"

namespace mgp {

constexpr int kFcBT = 128;   // tile edge (rows and columns)
constexpr int kFcBK = 16;    // k rows per chunk
constexpr int kFcNT = 256;   // threads
constexpr int kFcMaxD = 32;
constexpr int kFcV4 = kFcBK * kFcBT / 4 / kFcNT;             // float4 per thread, operand and chunk
constexpr int kFcChunk = kFcBK * 2 * kFcBT;                  // floats of one chunk (P and Q)
constexpr int kFcXld = kFcMaxD + 1;                          // odd row stride of the X tiles in LDS
constexpr int kFcLds = 2 * kFcChunk > 2 * kFcBT * kFcXld ? 2 * kFcChunk : 2 * kFcBT * kFcXld;

static inline size_t fc_align256(size_t x) { return (x + 255) / 256 * 256; }
static inline int64_t fc_round4(int64_t x) { return (x + 3) / 4 * 4; }

// acc[r][c] (wave (wr, wc), 32 x 32 blocks) = sum_{k in [kbeg, kend)} P[k][p0 + i] Q[k][q0 + j]
// for P [krows][ldp] (pcols columns) and Q [krows][ldq] (qcols columns), zero outside.
// TRI: P is read as a lower triangle, P[k][i] kept for k >= i (L_k as the T operand of
// C_k = L_k^T A).  kbeg is a multiple of 16.
template <bool TRI>
struct FcGemm {
  __device__ static __forceinline__ void load_chunk(floatx4 (&rp)[kFcV4], floatx4 (&rq)[kFcV4],
                                                    const float* __restrict__ P, int64_t ldp, int64_t pcols,
                                                    int64_t p0, const float* __restrict__ Q, int64_t ldq,
                                                    int64_t qcols, int64_t q0, int64_t krows, int64_t k0) {
#pragma unroll
    for (int q = 0; q < kFcV4; ++q) {
      const int idx = threadIdx.x + kFcNT * q;
      const int r = idx / (kFcBT / 4), c = (idx % (kFcBT / 4)) * 4;
      rp[q] = load4_guarded(P, ldp, k0 + r, p0 + c, krows, pcols);
      if (TRI) {
        const int64_t rel = k0 + r - (p0 + c);   // k - i of element 0
#pragma unroll
        for (int e = 0; e < 4; ++e) rp[q][e] = rel >= e ? rp[q][e] : 0.f;
      }
      rq[q] = load4_guarded(Q, ldq, k0 + r, q0 + c, krows, qcols);
    }
  }

  __device__ static __forceinline__ void store_chunk(float* __restrict__ sP, const floatx4 (&rp)[kFcV4],
                                                     const floatx4 (&rq)[kFcV4]) {
    float* sQ = sP + kFcBK * kFcBT;
#pragma unroll
    for (int q = 0; q < kFcV4; ++q) {
      const int idx = threadIdx.x + kFcNT * q;
      *reinterpret_cast<floatx4*>(sP + idx * 4) = rp[q];
      *reinterpret_cast<floatx4*>(sQ + idx * 4) = rq[q];
    }
  }

  // Leaves the LDS free (a barrier follows the last chunk's reads).
  __device__ static __forceinline__ void run(floatx16 (&acc)[2][2], float* __restrict__ lds,
                                             const float* __restrict__ P, int64_t ldp, int64_t pcols, int64_t p0,
                                             const float* __restrict__ Q, int64_t ldq, int64_t qcols, int64_t q0,
                                             int64_t krows, int64_t kbeg, int64_t kend) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = w >> 1, wc = w & 1;
    const int h = lane >> 5, l32 = lane & 31;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[r][c][e] = 0.f;
    if (kend <= kbeg) return;
    const int nchunks = (int)((kend - kbeg + kFcBK - 1) / kFcBK);
    floatx4 rp[kFcV4], rq[kFcV4];
    load_chunk(rp, rq, P, ldp, pcols, p0, Q, ldq, qcols, q0, krows, kbeg);
    store_chunk(lds, rp, rq);
    __syncthreads();
#pragma nounroll
    for (int ch = 0; ch < nchunks; ++ch) {
      const float* sP = lds + (ch & 1) * kFcChunk;
      const float* sQ = sP + kFcBK * kFcBT;
      const bool more = ch + 1 < nchunks;
      if (more) load_chunk(rp, rq, P, ldp, pcols, p0, Q, ldq, qcols, q0, krows, kbeg + (int64_t)(ch + 1) * kFcBK);
      float fa[kFcBK / 2][2], fb[kFcBK / 2][2];
#pragma unroll
      for (int ks = 0; ks < kFcBK / 2; ++ks) {
        const int kl = 2 * ks + h;
#pragma unroll
        for (int r = 0; r < 2; ++r) fa[ks][r] = sP[kl * kFcBT + wr * 64 + 32 * r + l32];
#pragma unroll
        for (int c = 0; c < 2; ++c) fb[ks][c] = sQ[kl * kFcBT + wc * 64 + 32 * c + l32];
      }
#pragma unroll
      for (int ks = 0; ks < kFcBK / 2; ++ks)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int c = 0; c < 2; ++c) acc[r][c] = mfma32x32x2(fa[ks][r], fb[ks][c], acc[r][c]);
      if (more) store_chunk(lds + ((ch + 1) & 1) * kFcChunk, rp, rq);
      __syncthreads();
    }
  }
};

// ------------------------------------------------------------------ stage 1
// grid (n tiles, m' tiles, K): C[k][m'][n] = sum_{m >= m'} q_sqrt[k][m][m'] A[m][n].
__global__ __launch_bounds__(kFcNT) void fullcov_lta_kernel(const float* __restrict__ A, int64_t lda,
                                                            const float* __restrict__ q_sqrt, int64_t ldqs,
                                                            int64_t strideq, int64_t M, int64_t N,
                                                            float* __restrict__ C, int64_t ldw, int64_t stridew) {
  __shared__ __attribute__((aligned(16))) float lds[2 * kFcChunk];
  const int64_t n0 = (int64_t)blockIdx.x * kFcBT, m0 = (int64_t)blockIdx.y * kFcBT;
  const int64_t k = blockIdx.z;
  floatx16 acc[2][2];
  FcGemm<true>::run(acc, lds, q_sqrt + k * strideq, ldqs, M, m0, A, lda, N, n0, M, m0, M);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = w >> 1, wc = w & 1, l32 = lane & 31;
  float* Ck = C + k * stridew;
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int64_t col = n0 + wc * 64 + 32 * c + l32;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int64_t row = m0 + wr * 64 + 32 * r + acc_row(e, lane);
        if (row < M && col < N) Ck[row * ldw + col] = acc[r][c][e];
      }
    }
}

// ------------------------------------------------------------------ stage 2
// Work items over the nT (nT + 1) / 2 lower-triangle tiles (ti >= tj, row-major over the
// triangle): item < whole owns tile `item` with all K experts; the remaining tiles are cut
// into `pieces` items of kg experts each (FcSplit), every piece forming base itself.
__global__ __launch_bounds__(kFcNT) void fullcov_syrk_kernel(
    const float* __restrict__ X, int64_t ldx, int64_t N, int D, const float* __restrict__ variance,
    const float* __restrict__ lengthscales, int n_ls, const float* __restrict__ A, int64_t lda,
    const float* __restrict__ C, int64_t ldw, int64_t stridew, int64_t M, int K, float* __restrict__ cov,
    int64_t ldc, int64_t stridec, int64_t whole, int pieces, int kg) {
  __shared__ __attribute__((aligned(16))) float lds[kFcLds];
  const int64_t item = blockIdx.x;
  const int64_t t = item < whole ? item : whole + (item - whole) / pieces;
  const int kbeg = item < whole ? 0 : (int)((item - whole) % pieces) * kg;
  const int kend = item < whole ? K : (kbeg + kg < K ? kbeg + kg : K);
  // tile (ti, tj) of linear index t = ti (ti + 1) / 2 + tj
  int64_t ti = (int64_t)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  while (ti * (ti + 1) / 2 > t) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  const int64_t tj = t - ti * (ti + 1) / 2;
  const int64_t i0 = ti * kFcBT, j0 = tj * kFcBT;

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = w >> 1, wc = w & 1, l32 = lane & 31;

  // base = Knn - A^T A
  floatx16 base[2][2];
  FcGemm<false>::run(base, lds, A, lda, N, i0, A, lda, N, j0, M, 0, M);
  {
    // (x - X[0]) / lengthscale of the tile's rows (sXi) and columns (sXj), zero beyond N:
    // relative to the first point before the scaling, so Knn does not depend on where the
    // data sits (the rounding of a scaled coordinate grows with the spread about X[0])
    float* sXi = lds;
    float* sXj = lds + kFcBT * kFcXld;
    for (int idx = threadIdx.x; idx < 2 * kFcBT * D; idx += kFcNT) {
      const int side = idx / (kFcBT * D), rem = idx % (kFcBT * D);
      const int p = rem / D, d = rem % D;
      const int64_t g = (side ? j0 : i0) + p;
      const float ls = lengthscales[n_ls == 1 ? 0 : d];
      (side ? sXj : sXi)[p * kFcXld + d] = g < N ? (X[g * ldx + d] - X[d]) / ls : 0.f;
    }
    __syncthreads();
    const float var = variance[0];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float* xj = sXj + (wc * 64 + 32 * c + l32) * kFcXld;
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float* xi = sXi + (wr * 64 + 32 * r + acc_row(e, lane)) * kFcXld;
          float r2 = 0.f;
          for (int d = 0; d < D; ++d) {
            const float df = xi[d] - xj[d];
            r2 = fmaf(df, df, r2);
          }
          base[r][c][e] = var * expf(-0.5f * r2) - base[r][c][e];
        }
    }
    __syncthreads();
  }

  const bool diag_tile = ti == tj;
  for (int k = kbeg; k < kend; ++k) {
    const float* Ck = C + (int64_t)k * stridew;
    floatx16 acc[2][2];
    FcGemm<false>::run(acc, lds, Ck, ldw, N, i0, Ck, ldw, N, j0, M, 0, M);
    float* out = cov + (int64_t)k * stridec;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int64_t gj = j0 + wc * 64 + 32 * c + l32;
        if (gj >= N) continue;
        // a tile of a diagonal workgroup tile that lies wholly above the diagonal
        if (diag_tile && wr * 64 + 32 * r + 31 < wc * 64 + 32 * c) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          // registers 4q .. 4q + 3: four consecutive rows
          const int64_t gi = i0 + wr * 64 + 32 * r + acc_row(4 * q, lane);
          floatx4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = base[r][c][4 * q + e] + acc[r][c][4 * q + e];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (gi + e < N && gi + e >= gj) out[(gi + e) * ldc + gj] = v[e];
          // mirror: cov[gj][gi .. gi + 3] (gi % 4 == 0, ldc % 4 == 0: 16-B aligned)
          if (gi + 3 < N && gi >= gj) {
            *reinterpret_cast<floatx4*>(out + gj * ldc + gi) = v;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (gi + e < N && gi + e > gj) out[gj * ldc + gi + e] = v[e];
          }
        }
      }
  }
}

// Stage 2's items.  A workgroup holds a CU for (experts + 1) passes over M, and the launch
// lasts (workgroup rounds) x (passes per workgroup).  Tiles in whole rounds of the CUs keep
// all K experts (A^T A once per tile); the tiles left over, which would hold a round of
// their own at K + 1 passes, are cut into pieces of kg experts, the cut that costs the
// fewest passes.  Costed for the MI355X's 256 CUs whatever device is current; cov's bits do
// not depend on the cut (every piece forms the same base and adds its own experts).
constexpr int kFcCUs = 256;
struct FcSplit { int64_t whole, items; int pieces, kg; };
static FcSplit fc_split(int64_t tiles, int K) {
  FcSplit s;
  s.whole = tiles / kFcCUs * kFcCUs;
  s.pieces = 1;
  s.kg = K;
  const int64_t rest = tiles - s.whole;
  int64_t best = K + 1;   // uncut: one round of K + 1 passes
  for (int kg = K - 1; kg >= 1; --kg) {
    const int pieces = (K + kg - 1) / kg;
    const int64_t cost = (rest * pieces + kFcCUs - 1) / kFcCUs * (kg + 1);
    if (cost < best) { best = cost; s.pieces = pieces; s.kg = kg; }
  }
  s.items = s.whole + rest * s.pieces;
  return s;
}

}  // namespace mgp

using namespace mgp;

extern "C" size_t mgp_full_cov_workspace_bytes(int64_t M, int64_t N, int32_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return fc_align256((size_t)K * (size_t)M * (size_t)fc_round4(N) * sizeof(float));
}

extern "C" int mgp_full_cov_conditional(const float* X, int64_t ldx, int64_t N, int32_t D, const float* variance,
                                        const float* lengthscales, int32_t n_ls, const float* A, int64_t lda,
                                        const float* q_sqrt, int64_t ldqs, int64_t strideq, int64_t M, int32_t K,
                                        float* cov, int64_t ldc, int64_t stridec, void* workspace,
                                        size_t workspace_bytes, mgp_stream_t stream) {
  if (!X) return -1;
  if (D < 1) return -4;
  if (D > kFcMaxD) return MGP_ERR_UNSUPPORTED;
  if (!variance) return -5;
  if (!lengthscales) return -6;
  if (n_ls != 1 && n_ls != D) return -7;
  if (!A) return -8;
  if (!q_sqrt) return -10;
  if (K > 32) return MGP_ERR_UNSUPPORTED;
  if (!cov) return -15;
  if (N <= 0 || M <= 0 || K <= 0) return MGP_OK;
  if (ldx < D) return -2;
  if (lda < N) return -9;
  if (ldqs < M) return -11;
  if (K > 1 && strideq < ldqs * M) return -12;
  if (ldc < N) return -16;
  if (K > 1 && stridec < ldc * N) return -17;
  if (lda % 4 || ldqs % 4 || ldc % 4 || (K > 1 && (strideq % 4 || stridec % 4))) return MGP_ERR_ALIGN;
  if (!aligned16(A) || !aligned16(q_sqrt) || !aligned16(cov)) return MGP_ERR_ALIGN;
  if (!workspace || workspace_bytes < mgp_full_cov_workspace_bytes(M, N, K)) return MGP_ERR_WORKSPACE;
  if (!aligned16(workspace)) return MGP_ERR_ALIGN;
  const int64_t nT = (N + kFcBT - 1) / kFcBT, mT = (M + kFcBT - 1) / kFcBT;
  if (nT * (nT + 1) / 2 > 0x7fffffffLL / 32 || mT > 65535) return MGP_ERR_UNSUPPORTED;
  const FcSplit sp = fc_split(nT * (nT + 1) / 2, K);
  hipStream_t s = (hipStream_t)stream;
  float* C = (float*)workspace;
  const int64_t ldw = fc_round4(N), stridew = M * ldw;
  hipLaunchKernelGGL(fullcov_lta_kernel, dim3((unsigned)nT, (unsigned)mT, (unsigned)K), dim3(kFcNT), 0, s, A, lda,
                     q_sqrt, ldqs, strideq, M, N, C, ldw, stridew);
  int st = launch_status();
  if (st) return st;
  hipLaunchKernelGGL(fullcov_syrk_kernel, dim3((unsigned)sp.items), dim3(kFcNT), 0, s, X, ldx, N, (int)D, variance,
                     lengthscales, (int)n_ls, A, lda, C, ldw, stridew, M, (int)K, cov, ldc, stridec, sp.whole,
                     sp.pieces, sp.kg);
  return launch_status();
}
