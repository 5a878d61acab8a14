// Natural-gradient step on the variational parameters (q_mu, q_sqrt) of a whitened SVGP
// layer: gpflow.optimizers.NaturalGradient(gamma) with the XiSqrtMeanVar parameterisation,
// which the reference's users run beside Adam on the hyper-parameters.  The semantics are
// stated in mgp_hip.h and DESIGN "Natural gradient"; tests/natgrad_ref.py restates them in
// float64 by the direct route (explicit natural / expectation parameters and inverses).
//
// Per expert k, L = tril(q_sqrt[k]), mu = q_mu[:, k], g = grad_sign * (given gradients):
//   P  = Phi(L^T g_L)              Phi: lower triangle, diagonal halved
//   B  = I + step (P + P^T)        the step exists iff B is positive definite
//   B  = W^T W, W lower            J B J = C C^T (J the index flip), W = J C^T J
//   L' = L W^-1                    W^-1 = J C^-T J, lower
//   mu' = mu - step L' (L'^T g_mu)
// All in float64 on the float32 inputs; no inverse of L or S = L L^T is formed.  Launches:
//   natgrad_b      lower 64 x 64 tiles of L^T g_L on v_mfma_f64_16x16x4_f64, k from the
//                  tile's first non-zero row block; writes J B J (float64, both triangles)
//   K3             chol.hip's blocked float64 Cholesky + triangular inverse on J B J, read
//                  in float64 (mgp_potrf_trtri_f64), 8 experts per call: C^-T (float32),
//                  info[k]
//   natgrad_apply  lower tiles of L' = L W^-1, W^-1 read through the flip from C^-T, k over
//                  the band [j0, i0 + 64); float64 L' into the workspace (staging)
//   natgrad_t      t = L'^T g_mu: a column's rows dealt to four accumulators in a fixed order
//   natgrad_mu     mu' = mu - step L' t: one wave per row, a butterfly over its lanes
//   natgrad_commit where info[k] == 0: tril(q_sqrt[k]) <- L', q_mu[:, k] <- mu' (float32)
// A failed expert (info[k] != 0, its factor carries NaN) is never copied back.  No
// floating-point atomics; every sum has a fixed order, so two calls give the same bits.
#include <math.h>

#include "mgp_common.hpp"

namespace mgp {
namespace natgrad {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 64;
constexpr int KC = 16;        // k-chunk in LDS
constexpr int kMaxGroup = 8;  // K3's batch limit

struct Layout {
  size_t mat, linvt, chol, t, mu, total;
  int64_t ldl, strideL;
};
static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
static Layout layout(int64_t M, int64_t K) {
  Layout L;
  L.ldl = (M + 3) / 4 * 4;
  L.strideL = M * L.ldl;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
  L.mat = take((size_t)K * M * M * sizeof(double));      // J B J, then L'
  L.linvt = take((size_t)K * L.strideL * sizeof(float));  // C^-T of every expert
  L.chol = take(mgp_chol_workspace_bytes(M, (int32_t)(K < kMaxGroup ? K : kMaxGroup)));
  L.t = take((size_t)K * M * sizeof(double));
  L.mu = take((size_t)K * M * sizeof(double));
  L.total = o;
  return L;
}

template <bool GD>
__device__ __forceinline__ double grad_at(const void* g, int64_t idx) {
  if constexpr (GD) return static_cast<const double*>(g)[idx];
  else return (double)static_cast<const float*>(g)[idx];
}

// MODE 0: T = L^T G (lower tiles), out = J (I + scale (Phi(T) + Phi(T)^T)) J.
//   op(A)[i][k] = L[k][i] (k >= i), op(B)[k][j] = G[k][j] (k >= j), k in [i0, M).
// MODE 1: out = L Winv (lower tiles), Winv[k][j] = CinvT[M-1-k][M-1-j] (k >= j),
//   op(A)[i][k] = L[i][k] (k <= i), k in [j0, i0 + 64).
// 64 x 64 tile per workgroup, wave w: rows 32 (w >> 1) .., columns 32 (w & 1) .. as 2 x 2
// MFMA blocks; KC-deep chunks one ahead in registers.  Lane l supplies A[l & 15][l >> 4] and
// B[l >> 4][l & 15]; accumulator register r holds row (l >> 4) + 4 r, column l & 15.
template <int MODE, bool GD>
__global__ __launch_bounds__(256) void tri_kernel(const float* __restrict__ q_sqrt, int64_t ldqs, int64_t strideq,
                                                  const void* __restrict__ G, int64_t ldgs, int64_t strideg,
                                                  const float* __restrict__ CinvT, int64_t ldl, int64_t strideL,
                                                  int64_t M, double scale, double* __restrict__ out) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj > bi) return;
  const int e = blockIdx.z;
  const float* L = q_sqrt + (int64_t)e * strideq;
  const int64_t goff = (int64_t)e * strideg;
  const float* Ci = MODE == 1 ? CinvT + (int64_t)e * strideL : nullptr;
  out += (int64_t)e * M * M;
  constexpr int LA = kTile * KC / 256, LB = KC * kTile / 256;
  __shared__ double sa[kTile][KC + 1], sb[KC][kTile + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wi = (w >> 1) * 32, wj = (w & 1) * 32;
  const int64_t i0 = (int64_t)bi * kTile, j0 = (int64_t)bj * kTile;
  const int64_t klo = MODE == 0 ? i0 : j0;
  const int64_t khi = MODE == 0 ? M : (i0 + kTile < M ? i0 + kTile : M);
  doublex4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = doublex4{0.0, 0.0, 0.0, 0.0};
  double ra[LA], rb[LB];
  auto load = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < LA; ++q) {
      const int idx = tid + 256 * q;
      const int r_a = MODE == 0 ? idx % kTile : idx / KC, k_a = MODE == 0 ? idx / kTile : idx % KC;
      const int64_t i = i0 + r_a, k = k0 + k_a;
      double v = 0.0;
      if (i < M && k < M) {
        if (MODE == 0) { if (i <= k) v = (double)L[k * ldqs + i]; }
        else { if (k <= i) v = (double)L[i * ldqs + k]; }
      }
      ra[q] = v;
    }
#pragma unroll
    for (int q = 0; q < LB; ++q) {
      const int idx = tid + 256 * q;
      const int c_b = idx % kTile, k_b = idx / kTile;
      const int64_t j = j0 + c_b, k = k0 + k_b;
      double v = 0.0;
      if (j < M && k < M && j <= k) {
        if (MODE == 0) v = grad_at<GD>(G, goff + k * ldgs + j);
        else v = (double)Ci[(M - 1 - k) * ldl + (M - 1 - j)];
      }
      rb[q] = v;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int q = 0; q < LA; ++q) {
      const int idx = tid + 256 * q;
      sa[MODE == 0 ? idx % kTile : idx / KC][MODE == 0 ? idx / kTile : idx % KC] = ra[q];
    }
#pragma unroll
    for (int q = 0; q < LB; ++q) {
      const int idx = tid + 256 * q;
      sb[idx / kTile][idx % kTile] = rb[q];
    }
  };
  if (klo < khi) load(klo);
  for (int64_t k0 = klo; k0 < khi; k0 += KC) {
    store();
    __syncthreads();
    if (k0 + KC < khi) load(k0 + KC);
#pragma unroll
    for (int ks = 0; ks < KC / 4; ++ks) {
      double av[2], bv[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) av[t] = sa[wi + 16 * t + (lane & 15)][4 * ks + (lane >> 4)];
#pragma unroll
      for (int t = 0; t < 2; ++t) bv[t] = sb[4 * ks + (lane >> 4)][wj + 16 * t + (lane & 15)];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i = i0 + wi + 16 * a + (lane >> 4) + 4 * r, j = j0 + wj + 16 * b + (lane & 15);
        if (i >= M || j >= M) continue;
        const double v = acc[a][b][r];
        if (MODE == 0) {
          if (j > i) continue;   // the mirror element writes both
          const int64_t fi = M - 1 - i, fj = M - 1 - j;
          if (i == j) {
            out[fi * M + fi] = 1.0 + scale * v;   // Phi halves the diagonal, P + P^T doubles it
          } else {
            const double bv2 = scale * v;
            out[fi * M + fj] = bv2;
            out[fj * M + fi] = bv2;
          }
        } else {
          out[i * M + j] = v;   // exact zeros above the diagonal of a diagonal tile
        }
      }
}

// t[k][j] = sum_{i >= j} L'[i][j] g_mu[i]; grid (ceil(M / 64), K), thread (c, rg): column
// j0 + c, rows j0 + rg + 4 n in order; the four partial sums are added as (0 + 1) + (2 + 3).
template <bool GD>
__global__ __launch_bounds__(256) void t_kernel(const double* __restrict__ Lp, const void* __restrict__ g_mu,
                                                int64_t ldg, int64_t M, double* __restrict__ t) {
  __shared__ double part[4][kTile];
  const int e = blockIdx.y;
  Lp += (int64_t)e * M * M;
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int64_t j0 = (int64_t)blockIdx.x * kTile, j = j0 + c;
  double acc = 0.0;
  if (j < M) {
    for (int64_t i = j0 + rg; i < M; i += 4)
      if (i >= j) acc = fma(Lp[i * M + j], grad_at<GD>(g_mu, i * ldg + e), acc);
  }
  part[rg][c] = acc;
  __syncthreads();
  if (rg == 0 && j < M) t[(int64_t)e * M + j] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
}

// mu'[k][i] = mu[i] - scale sum_{j <= i} L'[i][j] t[j]; one wave per row.
__global__ __launch_bounds__(256) void mu_kernel(const double* __restrict__ Lp, const double* __restrict__ t,
                                                 const float* __restrict__ q_mu, int64_t ldq, int64_t M, double scale,
                                                 double* __restrict__ mu_out) {
  const int e = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= M) return;   // wave-uniform
  const double* row = Lp + (int64_t)e * M * M + i * M;
  const double* te = t + (int64_t)e * M;
  double acc = 0.0;
  for (int64_t j = lane; j <= i; j += 64) acc = fma(row[j], te[j], acc);
  acc = wave_sum(acc);
  if (lane == 0) mu_out[(int64_t)e * M + i] = (double)q_mu[i * ldq + e] - scale * acc;
}

// grid (M, K): row i of expert k, copied only where the factorisation succeeded
__global__ __launch_bounds__(256) void commit_kernel(const double* __restrict__ Lp, const double* __restrict__ mu,
                                                     const int32_t* __restrict__ info, float* __restrict__ q_mu,
                                                     int64_t ldq, float* __restrict__ q_sqrt, int64_t ldqs,
                                                     int64_t strideq, int64_t M) {
  const int e = blockIdx.y;
  if (info[e] != 0) return;
  const int64_t i = blockIdx.x;
  const double* row = Lp + (int64_t)e * M * M + i * M;
  float* dst = q_sqrt + (int64_t)e * strideq + i * ldqs;
  for (int64_t j = threadIdx.x; j <= i; j += 256) dst[j] = (float)row[j];
  if (threadIdx.x == 0) q_mu[i * ldq + e] = (float)mu[(int64_t)e * M + i];
}

template <bool GD>
static int run(float* q_mu, int64_t ldq, float* q_sqrt, int64_t ldqs, int64_t strideq, const void* g_q_mu,
               int64_t ldg, const void* g_q_sqrt, int64_t ldgs, int64_t strideg, int64_t M, int K, double scale,
               int32_t* info, char* ws, const Layout& L, hipStream_t s) {
  double* mat = (double*)(ws + L.mat);
  float* linvt = (float*)(ws + L.linvt);
  double* t = (double*)(ws + L.t);
  double* mu = (double*)(ws + L.mu);
  const unsigned nt = (unsigned)((M + kTile - 1) / kTile);
  const dim3 tiles(nt, nt, (unsigned)K);
  hipLaunchKernelGGL((tri_kernel<0, GD>), tiles, dim3(256), 0, s, q_sqrt, ldqs, strideq, g_q_sqrt, ldgs, strideg,
                     (const float*)nullptr, (int64_t)0, (int64_t)0, M, scale, mat);
  int rc = launch_status();
  if (rc) return rc;
  for (int k0 = 0; k0 < K; k0 += kMaxGroup) {
    const int nb = K - k0 < kMaxGroup ? K - k0 : kMaxGroup;
    rc = mgp_potrf_trtri_f64(mat + (int64_t)k0 * M * M, M, M * M, M, nb, linvt + (int64_t)k0 * L.strideL, L.ldl,
                             L.strideL, info + k0, ws + L.chol, mgp_chol_workspace_bytes(M, nb), s);
    if (rc) return rc;
  }
  hipLaunchKernelGGL((tri_kernel<1, false>), tiles, dim3(256), 0, s, q_sqrt, ldqs, strideq, (const void*)nullptr,
                     (int64_t)0, (int64_t)0, linvt, L.ldl, L.strideL, M, 0.0, mat);
  rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL((t_kernel<GD>), dim3(nt, (unsigned)K), dim3(256), 0, s, mat, g_q_mu, ldg, M, t);
  rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(mu_kernel, dim3((unsigned)((M + 3) / 4), (unsigned)K), dim3(256), 0, s, mat, t, q_mu, ldq, M,
                     scale, mu);
  rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(commit_kernel, dim3((unsigned)M, (unsigned)K), dim3(256), 0, s, mat, mu, info, q_mu, ldq,
                     q_sqrt, ldqs, strideq, M);
  return launch_status();
}

constexpr int64_t kMaxM = 1 << 20;   // grid and index headroom; far above any inducing-point count
constexpr int kMaxK = 65535;         // the expert index is a grid dimension

}  // namespace natgrad
}  // namespace mgp

using namespace mgp;

extern "C" size_t mgp_natgrad_workspace_bytes(int64_t M, int32_t K) {
  if (M < 1 || K < 1 || M > natgrad::kMaxM || K > natgrad::kMaxK) return 0;
  return natgrad::layout(M, K).total;
}

extern "C" int mgp_natgrad_step(float* q_mu, int64_t ldq, float* q_sqrt, int64_t ldqs, int64_t strideq,
                                const void* g_q_mu, int64_t ldg, const void* g_q_sqrt, int64_t ldgs,
                                int64_t strideg, int32_t grad_is_double, int64_t M, int32_t K, float step,
                                float grad_sign, int32_t* info, void* workspace, size_t workspace_bytes,
                                mgp_stream_t stream) {
  if (!q_mu) return -1;
  if (!q_sqrt) return -3;
  if (!g_q_mu) return -6;
  if (!g_q_sqrt) return -8;
  if (grad_is_double != 0 && grad_is_double != 1) return -11;
  if (M < 1) return -12;
  if (K < 1) return -13;
  if (!(step >= 0.f) || !(step < INFINITY)) return -14;
  if (!(fabsf(grad_sign) < INFINITY)) return -15;
  if (!info) return -16;
  if (M > natgrad::kMaxM || K > natgrad::kMaxK) return MGP_ERR_UNSUPPORTED;
  if (ldq < K) return -2;
  if (ldqs < M) return -4;
  if (K > 1 && strideq < ldqs * M) return -5;
  if (ldg < K) return -7;
  if (ldgs < M) return -9;
  if (K > 1 && strideg < ldgs * M) return -10;
  const natgrad::Layout L = natgrad::layout(M, K);
  if (!workspace || workspace_bytes < L.total) return MGP_ERR_WORKSPACE;
  if (!aligned16(workspace)) return MGP_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  if (step == 0.f)   // B = I, W = I: the parameters stay as they are, bit for bit
    return hip_status(hipMemsetAsync(info, 0, (size_t)K * sizeof(int32_t), s));
  const double scale = (double)step * (double)grad_sign;
  char* ws = (char*)workspace;
  return grad_is_double ? natgrad::run<true>(q_mu, ldq, q_sqrt, ldqs, strideq, g_q_mu, ldg, g_q_sqrt, ldgs, strideg, M,
                                             K, scale, info, ws, L, s)
                        : natgrad::run<false>(q_mu, ldq, q_sqrt, ldqs, strideq, g_q_mu, ldg, g_q_sqrt, ldgs, strideg,
                                              M, K, scale, info, ws, L, s);
}
