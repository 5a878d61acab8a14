// Data association and point predictions of the mixture predictive p(y | x) = sum_k w_k N(y |
// mu_f,k, s_k^2), s_k^2 = var_f,k + lik_var_k, from the weights [N][K] of mgp_mixture_predict
// (mixture.hip): the posterior responsibilities p(z = k | x, y) with their hard labels, assignment
// entropy and per-expert effective counts, and the modes of p(. | x).  The semantics are stated in
// mgp_hip.h and DESIGN "Data association and modes"; tests/mixture_assign_ref.py restates them
// in float64.
//
//   a_k = log w_k - log s_k - (Y - mu_k)^2 / (2 s_k^2),  resp_k = exp(a_k - logsumexp_j a_j)
//
// mixture_resp_kernel: one lane per point, the K values a_k in registers under static indices.
// The quadratic term is taken in float64 from the float32 inputs (Y - mu and var_f + lik_var are
// then exact), so that 25 sigma out, where it is about 300, a_k - max_j a_j still carries the
// 1e-4 gate; logs, the exponential and the normalisation are float32.  usage: the float32
// resp values of a workgroup go through LDS and are summed in float64 in the order of the
// points, one partial per (workgroup, expert) in the workspace, then one workgroup per expert
// adds the partials (deterministic, no atomics).
// mixture_modes_kernel: one lane per (point, start), the KMAX lanes of a point consecutive; the
// point's parameters (log w_k - log s_k, mu_k, 1 / (2 s_k^2)) in LDS as float64, read by all its
// lanes.  The climb (below) runs in float64 and the result is rounded to float32 once.  The
// lanes leave their limits in LDS and the point's first lane merges and orders them.
#include <math.h>

#include "mgp_common.hpp"

namespace mgp {
namespace mixassign {

constexpr int kThreads = 256;
constexpr int kMaxIter = 100;                         // evaluations of p' per start, at most
constexpr double kInvSqrt2Pi = 0.39894228040143268;
constexpr double kMergeTol = 1e-3;                    // limits within kMergeTol min_k s_k are one mode
constexpr double kStopTol = 1e-9;                     // a step below kStopTol min_k s_k ends the climb
constexpr double kRelevant = 0x1p-10;                 // an expert counts at y from this fraction of the largest term

template <int KMAX>
__global__ __launch_bounds__(kThreads) void mixture_resp_kernel(
    const float* __restrict__ mu_f, const float* __restrict__ var_f, int64_t ldf, const float* __restrict__ lik_var,
    const float* __restrict__ weights, const float* __restrict__ Y, int64_t N, int K, float* __restrict__ resp,
    int64_t ldr, int32_t* __restrict__ labels, float* __restrict__ entropy, double* __restrict__ partials) {
  __shared__ float r_lds[KMAX * (kThreads + 1)];
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = n < N;
  const double y = live ? (double)Y[n] : 0.0;
  double a[KMAX];
  double amax = -INFINITY;
  int lab = -1;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    a[k] = -INFINITY;
    if (live && k < K) {
      const float w = weights[n * K + k];
      const double d = y - (double)mu_f[(int64_t)k * ldf + n];
      const double v = (double)var_f[(int64_t)k * ldf + n] + (double)lik_var[k];
      if (w > 0.f) a[k] = (double)(logf(w) - 0.5f * logf((float)v)) - 0.5 * d * d / v;
      if (a[k] > amax) {   // strict: ties go to the lowest k
        amax = a[k];
        lab = k;
      }
    }
  }
  // b_k = a_k - max <= 0 in float32; e_k = exp(b_k), summed in ascending k
  float e[KMAX];
  float se = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    e[k] = (k < K && lab >= 0) ? expf((float)(a[k] - amax)) : 0.f;
    se += e[k];
  }
  const float lse = logf(se);
  float dot = 0.f;
  const float bad = (live && lab < 0) ? NAN : 0.f;   // no positive weight: NaN, label -1
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const float r = lab >= 0 ? e[k] / se : bad;
    if (k < K) {
      if (r != 0.f && lab >= 0) dot = fmaf(r, (float)(a[k] - amax), dot);
      if (live && resp) resp[n * ldr + k] = r;
    }
    e[k] = r;
  }
  if (live) {
    if (labels) labels[n] = lab;
    if (entropy) entropy[n] = lab >= 0 ? lse - dot : NAN;
  }
  if (partials) {   // uniform over the grid
    // the workgroup's float32 values, expert-major with a padded row (no bank conflicts either
    // way); thread k then adds expert k's column in float64, in the order of the points
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) r_lds[k * (kThreads + 1) + threadIdx.x] = live ? e[k] : 0.f;
    __syncthreads();
    if ((int)threadIdx.x < K) {
      double s = 0.0;
      for (int i = 0; i < kThreads; ++i) s += (double)r_lds[threadIdx.x * (kThreads + 1) + i];
      partials[(int64_t)blockIdx.x * K + threadIdx.x] = s;
    }
  }
}

// usage[k] = sum_b partials[b][k]: one workgroup per expert
__global__ __launch_bounds__(kThreads) void mixture_usage_kernel(const double* __restrict__ partials, int64_t nb,
                                                                 int K, double* __restrict__ usage) {
  __shared__ double scratch[16];
  const int k = blockIdx.x;
  double v = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += kThreads) v += partials[b * K + k];
  v = block_sum<double>(v, scratch);
  if (threadIdx.x == 0) usage[k] = v;
}

// The modes of p are the distinct limits of hill-climbing p from the expert means with w_k > 0
// (Carreira-Perpinan 2000).  With c_k(y) = log w_k - log s_k - (y - mu_k)^2 / (2 s_k^2), taken
// relative to max_k c_k(y) so that a start between distant experts divides nothing by zero,
// u_k = exp(c_k - max), i_k = 1 / s_k^2 and d_k = mu_k - y:
//   A = sum u_k i_k,   G = sum u_k i_k d_k  (p' up to a positive factor),
//   H = sum u_k i_k (i_k d_k^2 - 1)         (p'' up to the same factor)
//  step     uphill (the sign of G) by cap = max(|G / A|, s_rel / 2): the mean-shift step G / A,
//           which never decreases p, or half the bandwidth s_rel of the narrowest expert with
//           u_k >= 2^-10, i.e. that counts at y, where that is longer (mean-shift alone crawls
//           on a slope under a narrow expert; no feature of p near y is narrower than s_rel);
//           where H < 0 the Newton step -G / H on p' if it is shorter than cap (it is never
//           shorter than the mean-shift step, as 0 < -H <= A), so that a nearly flat stretch
//           cannot throw the iterate onto another hill
//  bracket  lo / hi: the last iterates with G > 0 / G < 0; once both exist a maximum lies
//           between them, and the bisection point replaces an iterate that is not strictly
//           inside
//  stop     G == 0, a step of at most 1e-9 min_k s_k or below the resolution of y, adjacent
//           endpoints, or kMaxIter evaluations: the last iterate is returned, the loop never
//           spins.  (On the 46000 starts of the test cases, K up to 32, none needs more than 30.)
template <int KMAX>
__global__ __launch_bounds__(kThreads) void mixture_modes_kernel(
    const float* __restrict__ mu_f, const float* __restrict__ var_f, int64_t ldf, const float* __restrict__ lik_var,
    const float* __restrict__ weights, int64_t N, int K, float* __restrict__ modes, float* __restrict__ mode_density,
    int64_t ldm, int32_t* __restrict__ count) {
  constexpr int kPoints = kThreads / KMAX;
  __shared__ double s_c[kThreads], s_m[kThreads], s_h[kThreads];   // log w - log s, mu, 1 / (2 s^2)
  __shared__ double s_y[kThreads], s_d[kThreads];                   // a start's limit and its density
  const int tid = threadIdx.x;
  const int j = tid % KMAX, base = tid - j;
  const int64_t n = (int64_t)blockIdx.x * kPoints + tid / KMAX;
  const bool have = n < N && j < K;
  double cj = -INFINITY, mj = 0.0, hj = 0.0;
  if (have) {
    const float w = weights[n * K + j];
    const double v = (double)var_f[(int64_t)j * ldf + n] + (double)lik_var[j];
    mj = (double)mu_f[(int64_t)j * ldf + n];
    hj = 0.5 / v;
    if (w > 0.f) cj = log((double)w) - 0.5 * log(v);
  }
  s_c[tid] = cj;
  s_m[tid] = mj;
  s_h[tid] = hj;
  s_y[tid] = NAN;
  s_d[tid] = NAN;
  __syncthreads();
  const bool start = have && cj > -INFINITY;
  double hmax = 0.0;
  if (n < N)
    for (int k = 0; k < K; ++k) hmax = fmax(hmax, s_h[base + k]);
  const double smin = sqrt(0.5 / hmax);
  if (start) {
    double y = mj, lo = -INFINITY, hi = INFINITY;
    const double tol = kStopTol * smin;
    double mx = 0.0, S0 = 0.0;
    for (int it = 0; it < kMaxIter; ++it) {
      mx = -INFINITY;
      for (int k = 0; k < K; ++k) {
        const double d = s_m[base + k] - y;
        mx = fmax(mx, s_c[base + k] - s_h[base + k] * d * d);
      }
      double A = 0.0, G = 0.0, H = 0.0, imax = 0.0;
      for (int k = 0; k < K; ++k) {
        const double d = s_m[base + k] - y, i2 = 2.0 * s_h[base + k];
        const double u = exp(s_c[base + k] - s_h[base + k] * d * d - mx);
        const double ui = u * i2;
        A += ui;
        G = fma(ui, d, G);
        H = fma(ui, i2 * d * d - 1.0, H);
        if (u >= kRelevant) imax = fmax(imax, i2);
      }
      if (!(G > 0.0) && !(G < 0.0)) break;   // a maximum to the last bit (or NaN inputs)
      if (G > 0.0) lo = y; else hi = y;
      const double ms = G / A;
      const double cap = fmax(fabs(ms), 0.5 / sqrt(imax));
      const double step = copysign(H < 0.0 ? fmin(fabs(G / H), cap) : cap, G);
      double yn = y + step;
      bool done = fabs(step) <= tol || yn == y;
      if (!done && lo > -INFINITY && hi < INFINITY && !(yn > lo && yn < hi)) {
        const double mid = lo + 0.5 * (hi - lo);
        if (mid == lo || mid == hi) break;
        yn = mid;
      }
      done = done || fabs(yn - y) <= tol;
      y = yn;
      if (done) break;
    }
    // the density at the returned iterate
    mx = -INFINITY;
    S0 = 0.0;
    for (int k = 0; k < K; ++k) {
      const double d = s_m[base + k] - y;
      mx = fmax(mx, s_c[base + k] - s_h[base + k] * d * d);
    }
    for (int k = 0; k < K; ++k) {
      const double d = s_m[base + k] - y;
      S0 += exp(s_c[base + k] - s_h[base + k] * d * d - mx);
    }
    s_y[tid] = y;
    s_d[tid] = exp(mx) * S0 * kInvSqrt2Pi;
  }
  __syncthreads();
  if (j != 0 || n >= N) return;
  // merge and order: the densest remaining limit is the next mode (ties: the lowest y) and
  // takes every limit within the tolerance with it
  const double tol = kMergeTol * smin;
  int cnt = 0;
  for (int round = 0; round < K; ++round) {
    int best = -1;
    double bd = 0.0, by = 0.0;
    for (int k = 0; k < K; ++k) {
      const double dk = s_d[base + k], yk = s_y[base + k];
      if (!(dk == dk) || !(yk == yk)) continue;
      if (best < 0 || dk > bd || (dk == bd && yk < by)) {
        best = k;
        bd = dk;
        by = yk;
      }
    }
    if (best < 0) break;
    if (modes) modes[n * ldm + cnt] = (float)by;
    if (mode_density) mode_density[n * ldm + cnt] = (float)bd;
    ++cnt;
    for (int k = 0; k < K; ++k)
      if (fabs(s_y[base + k] - by) <= tol) s_d[base + k] = NAN;
    s_d[base + best] = NAN;
  }
  for (int c = cnt; c < K; ++c) {
    if (modes) modes[n * ldm + c] = NAN;
    if (mode_density) mode_density[n * ldm + c] = NAN;
  }
  if (count) count[n] = cnt;
}

static int64_t resp_blocks(int64_t N) { return (N + kThreads - 1) / kThreads; }
static int kmax_of(int K) { return K <= 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : K <= 16 ? 16 : 32; }

}  // namespace mixassign
}  // namespace mgp

using namespace mgp;

extern "C" size_t mgp_mixture_responsibilities_workspace_bytes(int64_t N, int32_t K) {
  const int64_t nb = N > 0 ? mixassign::resp_blocks(N) : 1;
  return (size_t)nb * (size_t)(K > 0 ? K : 1) * sizeof(double);
}

extern "C" int mgp_mixture_responsibilities(const float* mu_f, const float* var_f, int64_t ldf, const float* lik_var,
                                            const float* weights, const float* Y, int64_t N, int32_t K, float* resp,
                                            int64_t ldr, int32_t* labels, float* entropy, double* usage,
                                            void* workspace, size_t workspace_bytes, mgp_stream_t stream) {
  if (!mu_f) return -1;
  if (!var_f) return -2;
  if (N > 0 && ldf < N) return -3;
  if (!lik_var) return -4;
  if (!weights) return -5;
  if (!Y) return -6;
  if (K < 1) return -8;
  if (K > 32) return MGP_ERR_UNSUPPORTED;
  if (resp && ldr < K) return -10;
  if (N <= 0) return MGP_OK;
  if (N > (int64_t)0x7fffffff * mixassign::kThreads) return MGP_ERR_UNSUPPORTED;
  if (usage && (!workspace || workspace_bytes < mgp_mixture_responsibilities_workspace_bytes(N, K)))
    return MGP_ERR_WORKSPACE;
  const int64_t nb = mixassign::resp_blocks(N);
  double* partials = usage ? (double*)workspace : nullptr;
  hipStream_t s = (hipStream_t)stream;
#define MGP_MIXRESP_CASE(KM)                                                                                  \
  if (K <= KM) {                                                                                              \
    hipLaunchKernelGGL((mixassign::mixture_resp_kernel<KM>), dim3((unsigned)nb), dim3(mixassign::kThreads), 0, \
                       s, mu_f, var_f, ldf, lik_var, weights, Y, N, K, resp, ldr, labels, entropy, partials); \
  } else
  MGP_MIXRESP_CASE(1) MGP_MIXRESP_CASE(2) MGP_MIXRESP_CASE(4) MGP_MIXRESP_CASE(8) MGP_MIXRESP_CASE(16)
  MGP_MIXRESP_CASE(32) {}
#undef MGP_MIXRESP_CASE
  int st = launch_status();
  if (st || !usage) return st;
  hipLaunchKernelGGL(mixassign::mixture_usage_kernel, dim3((unsigned)K), dim3(mixassign::kThreads), 0, s, partials,
                     nb, (int)K, usage);
  return launch_status();
}

extern "C" int mgp_mixture_modes(const float* mu_f, const float* var_f, int64_t ldf, const float* lik_var,
                                 const float* weights, int64_t N, int32_t K, float* modes, float* mode_density,
                                 int64_t ldm, int32_t* count, mgp_stream_t stream) {
  if (!mu_f) return -1;
  if (!var_f) return -2;
  if (N > 0 && ldf < N) return -3;
  if (!lik_var) return -4;
  if (!weights) return -5;
  if (K < 1) return -7;
  if (K > 32) return MGP_ERR_UNSUPPORTED;
  if ((modes || mode_density) && ldm < K) return -10;
  if (N <= 0) return MGP_OK;
  const int km = mixassign::kmax_of(K);
  const int64_t per = mixassign::kThreads / km;
  if (N > (int64_t)0x7fffffff * per) return MGP_ERR_UNSUPPORTED;
  const int64_t nb = (N + per - 1) / per;
  hipStream_t s = (hipStream_t)stream;
#define MGP_MIXMODES_CASE(KM)                                                                                  \
  if (K <= KM) {                                                                                               \
    hipLaunchKernelGGL((mixassign::mixture_modes_kernel<KM>), dim3((unsigned)nb), dim3(mixassign::kThreads), 0, \
                       s, mu_f, var_f, ldf, lik_var, weights, N, K, modes, mode_density, ldm, count);          \
  } else
  MGP_MIXMODES_CASE(1) MGP_MIXMODES_CASE(2) MGP_MIXMODES_CASE(4) MGP_MIXMODES_CASE(8) MGP_MIXMODES_CASE(16)
  MGP_MIXMODES_CASE(32) {}
#undef MGP_MIXMODES_CASE
  return launch_status();
}
