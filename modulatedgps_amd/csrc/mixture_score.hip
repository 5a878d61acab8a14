// Scores of the mixture predictive p(y | x) = sum_k w_k N(y | mu_f,k, s_k^2), s_k^2 = var_f,k +
// lik_var_k, from the weights [N][K] of mgp_mixture_predict (mixture.hip): the CDF and the
// survival function at a target (the PIT values of a calibration plot), the CRPS in closed
// form, and quantiles.  The semantics are stated in mgp_hip.h and DESIGN "Mixture scores";
// tests/mixture_score_ref.py restates them in float64.
//
//   t_k = (Y - mu_k) / s_k,  cdf = sum_k w_k erfc(-t_k / sqrt 2) / 2,  sf = sum_k w_k erfc(t_k / sqrt 2) / 2
//   A(m, v) = m erf(m / sqrt(2 v)) + sqrt(2 v / pi) exp(-m^2 / (2 v))
//   crps = sum_i w_i A(Y - mu_i, s_i^2) - sum_i w_i^2 s_i / sqrt(pi) - sum_{i<j} w_i w_j A(mu_i - mu_j, s_i^2 + s_j^2)
//
// mixture_score_kernel: mixture.hip's layout -- 4 consecutive lanes share a point.  Every lane
// holds the point's K triples (w, mu, s^2) in registers under static indices; lane c owns the
// experts i = 4 j + c (picked out of the static array by three selects, so nothing is indexed
// dynamically and nothing goes to scratch).  For an owned expert a lane takes one erfc and one
// exponential, which give its cdf, sf and A(Y - mu_i, s_i^2) terms, and then the pairs (i, k),
// k > i.  Butterfly shuffles merge the four lanes in a fixed order; lanes beyond N take part
// with zero weights.  A float64 block partial of crps goes to the workspace and a one-block
// kernel sums the partials (deterministic, no atomics).
// mixture_quantiles_kernel: one lane per (point, level), the Q levels of a point in consecutive
// lanes; a bracketed Newton iteration on the tail probability (below).
#include <math.h>

#include "mgp_common.hpp"

namespace mgp {
namespace mixscore {

constexpr int kThreads = 256;
constexpr int kLanes = 4;   // fixed for every N: per-point bits do not depend on the sharding
constexpr int kMaxLevels = 256;
constexpr int kMaxIter = 100;
constexpr float kInvSqrt2 = 0.70710678118654752f;
constexpr float kInvSqrtPi = 0.56418958354775629f;
constexpr float kSqrt2OverPi = 0.79788456080286536f;

__device__ __forceinline__ float lanes_sum(float v) {
#pragma unroll
  for (int off = 1; off < kLanes; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// a[j4 + c] of the lane's own c in 0 .. 3 (j4 a compile-time constant once unrolled); pad
// beyond KMAX
template <int KMAX>
__device__ __forceinline__ float pick4(const float (&a)[KMAX], int j4, int c, float pad) {
  float r = pad;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float x = (j4 + e < KMAX) ? a[j4 + e < KMAX ? j4 + e : 0] : pad;
    r = (c == e) ? x : r;
  }
  return r;
}

template <int KMAX>
__global__ __launch_bounds__(kThreads) void mixture_score_kernel(
    const float* __restrict__ mu_f, const float* __restrict__ var_f, int64_t ldf, const float* __restrict__ lik_var,
    const float* __restrict__ weights, const float* __restrict__ Y, int64_t N, int K, float* __restrict__ cdf,
    float* __restrict__ sf, float* __restrict__ crps, double* __restrict__ partials) {
  __shared__ double scratch[16];
  const int64_t gt = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t n = gt / kLanes;
  const int sub = (int)(gt % kLanes);
  const bool live = n < N;
  // padding experts and points beyond N: weight 0 at (mu, s^2) = (0, 1), every term a finite
  // number times zero
  float w[KMAX], m[KMAX], v[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const bool on = live && k < K;
    w[k] = on ? weights[n * K + k] : 0.f;
    m[k] = on ? mu_f[(int64_t)k * ldf + n] : 0.f;
    v[k] = on ? var_f[(int64_t)k * ldf + n] + lik_var[k] : 1.f;
  }
  const float y = live ? Y[n] : 0.f;
  float c_lo = 0.f, c_up = 0.f, first = 0.f, diag = 0.f, off = 0.f;
  constexpr int J = (KMAX + 3) / 4;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    if (4 * j >= K) break;
    const float ow = pick4<KMAX>(w, 4 * j, sub, 0.f), om = pick4<KMAX>(m, 4 * j, sub, 0.f);
    const float ov = pick4<KMAX>(v, 4 * j, sub, 1.f);
    const float os = sqrtf(ov);
    const float d = y - om;
    const float z = (d / os) * kInvSqrt2;
    // erfc on the positive side keeps the small tail to its own relative accuracy; the other
    // tail is 1 - it, and erf(|z|) = 1 - erfc(|z|) (its absolute error of an ulp of 1 stands
    // beside the exponential term of A, which is the larger one wherever erf is small)
    const float ec = erfcf(fabsf(z));
    const float tail = 0.5f * ec, body = 1.f - tail;
    c_lo = fmaf(ow, z < 0.f ? tail : body, c_lo);
    c_up = fmaf(ow, z < 0.f ? body : tail, c_up);
    const float a_own = fmaf(fabsf(d), 1.f - ec, os * kSqrt2OverPi * __expf(-z * z));
    first = fmaf(ow, a_own, first);
    diag = fmaf(ow * ow, os * kInvSqrtPi, diag);
    // pairs (i, k), k > i = 4 j + sub: always for k >= 4 j + 4, by the lane for the three before
#pragma unroll
    for (int k = 4 * j + 1; k < KMAX; ++k) {
      if (k >= K) break;
      const float two_v = 2.f * (ov + v[k]);
      const float inv = rsqrtf(two_v);
      const float dm = fabsf(om - m[k]);
      const float zz = dm * inv;
      const float a_pair = fmaf(dm, erff(zz), two_v * inv * kInvSqrtPi * __expf(-zz * zz));
      const float ww = (k > 4 * j + sub) ? ow * w[k] : 0.f;
      off = fmaf(ww, a_pair, off);
    }
  }
  // every lane of the wave takes part in the shuffles (points beyond N included)
  c_lo = lanes_sum(c_lo);
  c_up = lanes_sum(c_up);
  first = lanes_sum(first);
  diag = lanes_sum(diag);
  off = lanes_sum(off);
  float val = 0.f;
  if (live && sub == 0) {
    val = (first - diag) - off;
    if (cdf) cdf[n] = c_lo;
    if (sf) sf[n] = c_up;
    if (crps) crps[n] = val;
  }
  if (partials) {
    const double bs = block_sum<double>((double)val, scratch);
    if (threadIdx.x == 0) partials[blockIdx.x] = bs;
  }
}

__global__ __launch_bounds__(1024) void mixture_score_sum_partials_kernel(const double* __restrict__ p, int n,
                                                                          double* __restrict__ out) {
  __shared__ double scratch[16];
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) v += p[i];
  v = block_sum<double>(v, scratch);
  if (threadIdx.x == 0) *out = v;
}

// quantile(p): the root of h(y) = cdf(y) - p (p <= 1/2) or (1 - p) - sf(y) (p > 1/2), both
// increasing in y with the density as derivative, so that the tail probability is the
// quantity solved for and upper quantiles are as accurate as lower ones.
//  bracket  [min_k e_k, max_k e_k], e_k = mu_k + s_k z_p (the mixture CDF is a convex
//           combination of the experts' CDFs), widened by 4e-6 (|e| + max_k s_k) for the
//           rounding of z_p and e_k
//  iterate  Newton from the midpoint; the bisection point instead whenever the Newton iterate
//           is not finite or not strictly inside the bracket, or the bracket has not halved
//           over the last two iterations (a narrow expert between the iterate and the root
//           makes plain safeguarded Newton crawl)
//  stop     h == 0, or the midpoint equals an endpoint (adjacent floats); at most kMaxIter
template <int KMAX>
__global__ __launch_bounds__(kThreads) void mixture_quantiles_kernel(
    const float* __restrict__ mu_f, const float* __restrict__ var_f, int64_t ldf, const float* __restrict__ lik_var,
    const float* __restrict__ weights, int64_t N, int K, const float* __restrict__ levels, int Q,
    float* __restrict__ quantiles, int64_t ldq) {
  const int64_t gt = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t n = gt / Q;
  const int q = (int)(gt % Q);
  if (n >= N) return;
  const float p = levels[q];
  float* dst = quantiles + n * ldq + q;
  if (!(p > 0.f && p < 1.f)) {
    *dst = NAN;
    return;
  }
  const bool upper = p > 0.5f;
  const float pt = upper ? 1.f - p : p;   // exact: p in (1/2, 1)
  const float zt = normcdfinvf(pt);
  const float zp = upper ? -zt : zt;
  // w, mu and 1 / (s sqrt 2): the argument of erfc is (y - mu) r, the density w r exp(-.^2) / sqrt(pi)
  float w[KMAX], m[KMAX], r[KMAX];
  float lo = INFINITY, hi = -INFINITY, smax = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {
      w[k] = weights[n * K + k];
      m[k] = mu_f[(int64_t)k * ldf + n];
      const float s = sqrtf(var_f[(int64_t)k * ldf + n] + lik_var[k]);
      r[k] = kInvSqrt2 / s;
      const float e = fmaf(s, zp, m[k]);
      lo = fminf(lo, e);
      hi = fmaxf(hi, e);
      smax = fmaxf(smax, s);
    } else {
      w[k] = 0.f; m[k] = 0.f; r[k] = 1.f;
    }
  }
  float a = lo - 4e-6f * (fabsf(lo) + smax), b = hi + 4e-6f * (fabsf(hi) + smax);
  float y = a + 0.5f * (b - a);
  float width1 = b - a, width2 = INFINITY;   // the bracket one and two iterations ago
  for (int it = 0; it < kMaxIter; ++it) {
    float F = 0.f, dens = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k >= K) break;
      const float z = (y - m[k]) * r[k];
      F = fmaf(w[k], 0.5f * erfcf(upper ? z : -z), F);
      dens = fmaf(w[k] * r[k], __expf(-z * z), dens);
    }
    const float h = upper ? pt - F : F - pt;
    if (h == 0.f) break;
    if (h < 0.f) a = y; else b = y;
    const float mid = a + 0.5f * (b - a);
    if (mid == a || mid == b) break;
    const float width = b - a;
    const float yn = y - h / (dens * kInvSqrtPi);
    const bool bisect = !(yn > a && yn < b) || !(width <= 0.5f * width2);
    width2 = width1;
    width1 = width;
    y = bisect ? mid : yn;
  }
  *dst = y;
}

static int64_t score_blocks(int64_t N) { return (N * kLanes + kThreads - 1) / kThreads; }

}  // namespace mixscore
}  // namespace mgp

using namespace mgp;

extern "C" size_t mgp_mixture_score_workspace_bytes(int64_t N, int32_t K) {
  (void)K;
  const int64_t nb = N > 0 ? mixscore::score_blocks(N) : 1;
  return (size_t)nb * sizeof(double);
}

extern "C" int mgp_mixture_score(const float* mu_f, const float* var_f, int64_t ldf, const float* lik_var,
                                 const float* weights, const float* Y, int64_t N, int32_t K, float* cdf, float* sf,
                                 float* crps, double* crps_sum, void* workspace, size_t workspace_bytes,
                                 mgp_stream_t stream) {
  if (!mu_f) return -1;
  if (!var_f) return -2;
  if (N > 0 && ldf < N) return -3;
  if (!lik_var) return -4;
  if (!weights) return -5;
  if (!Y) return -6;
  if (K < 1) return -8;
  if (K > 32) return MGP_ERR_UNSUPPORTED;
  if (N <= 0) return MGP_OK;
  if (N > (int64_t)0x7fffffff * (mixscore::kThreads / mixscore::kLanes)) return MGP_ERR_UNSUPPORTED;
  const int64_t nb = mixscore::score_blocks(N);
  if (crps_sum && (!workspace || workspace_bytes < mgp_mixture_score_workspace_bytes(N, K)))
    return MGP_ERR_WORKSPACE;
  double* partials = crps_sum ? (double*)workspace : nullptr;
  hipStream_t s = (hipStream_t)stream;
#define MGP_MIXSCORE_CASE(KM)                                                                                \
  if (K <= KM) {                                                                                             \
    hipLaunchKernelGGL((mixscore::mixture_score_kernel<KM>), dim3((unsigned)nb), dim3(mixscore::kThreads), 0, \
                       s, mu_f, var_f, ldf, lik_var, weights, Y, N, K, cdf, sf, crps, partials);             \
  } else
  MGP_MIXSCORE_CASE(1) MGP_MIXSCORE_CASE(2) MGP_MIXSCORE_CASE(4) MGP_MIXSCORE_CASE(8) MGP_MIXSCORE_CASE(16)
  MGP_MIXSCORE_CASE(32) {}
#undef MGP_MIXSCORE_CASE
  int st = launch_status();
  if (st || !crps_sum) return st;
  hipLaunchKernelGGL(mixscore::mixture_score_sum_partials_kernel, dim3(1), dim3(1024), 0, s, partials, (int)nb,
                     crps_sum);
  return launch_status();
}

extern "C" int mgp_mixture_quantiles(const float* mu_f, const float* var_f, int64_t ldf, const float* lik_var,
                                     const float* weights, int64_t N, int32_t K, const float* levels, int32_t Q,
                                     float* quantiles, int64_t ldq, mgp_stream_t stream) {
  if (!mu_f) return -1;
  if (!var_f) return -2;
  if (N > 0 && ldf < N) return -3;
  if (!lik_var) return -4;
  if (!weights) return -5;
  if (K < 1) return -7;
  if (K > 32) return MGP_ERR_UNSUPPORTED;
  if (!levels) return -8;
  if (Q < 0) return -9;
  if (Q > mixscore::kMaxLevels) return MGP_ERR_UNSUPPORTED;
  if (!quantiles) return -10;
  if (ldq < Q) return -11;
  if (N <= 0 || Q == 0) return MGP_OK;
  if (N > (int64_t)0x7fffffff * mixscore::kThreads / Q) return MGP_ERR_UNSUPPORTED;
  const int64_t nb = (N * Q + mixscore::kThreads - 1) / mixscore::kThreads;
  hipStream_t s = (hipStream_t)stream;
#define MGP_MIXQ_CASE(KM)                                                                                        \
  if (K <= KM) {                                                                                                 \
    hipLaunchKernelGGL((mixscore::mixture_quantiles_kernel<KM>), dim3((unsigned)nb), dim3(mixscore::kThreads), 0, \
                       s, mu_f, var_f, ldf, lik_var, weights, N, K, levels, (int)Q, quantiles, ldq);             \
  } else
  MGP_MIXQ_CASE(1) MGP_MIXQ_CASE(2) MGP_MIXQ_CASE(4) MGP_MIXQ_CASE(8) MGP_MIXQ_CASE(16) MGP_MIXQ_CASE(32) {}
#undef MGP_MIXQ_CASE
  return launch_status();
}
