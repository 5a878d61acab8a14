// The mixture predictive of a trained SMGP: p(y | x) = sum_k w_k N(y | mu_f,k, s2_k),
// s2_k = var_f,k + lik_var_k (GaussianModified._predict_mean_and_var, likelihoods.py:31-32).
// The reference has no counterpart (its demos scatter predict_samples points at alpha
// 0.01); the semantics are stated in mgp_hip.h and DESIGN "Mixture predictive".
//
// Weights: RelaxedOneHotCategorical(1e-2, logits) relaxes argmax_k(g_k + logit_k), whose
// class probabilities are softmax_k(logits) by the Gumbel-max identity, so the Gumbel
// noise is integrated out and only the Gaussian noise of the logits (utils.py:27, as K6
// applies it) is sampled: w_k = mean_s softmax_k(mu_a + z_s sqrt(max(var_a + jitter, 0)));
// S == 0: the plug-in softmax_k(mu_a) of predict_assign.
//
// mixture_predict_kernel: K6's layout (elbo.hip) -- LANES consecutive lanes share a point
// and split its S samples.  A lane keeps K running softmax sums (the weights) and one
// running (max, sum) pair, the log-sum-exp over (s, k) of log_softmax_k(logits_s) +
// log N_k; butterfly shuffles merge the lanes, lane 0 of the point writes.  A float64
// block partial of log_density goes to the workspace and a one-block kernel sums the
// partials (deterministic, no atomics).  Per sample it draws one Philox block per four
// experts (K6: two) and takes 2 K exponentials and one logarithm (K6: 2 K logarithms
// for the Gumbels on top of its K exponentials).
// mixture_density_grid_kernel: the density on a grid of targets, threads along the grid.
#include <math.h>

#include "mgp_common.hpp"

namespace mgp {
namespace mixture {

constexpr int kThreads = 256;
// Lanes per point.  Fixed (K6's forward picks 4 / 8 / 16 by N): the float32 sums over a
// point's samples are then grouped the same way for every N, so the per-point outputs of
// a shard are bitwise those of the unsharded call.
constexpr int kLanes = 4;
constexpr float kHalfLog2Pi = 0.91893853320467274f;

template <int LANES>
__device__ __forceinline__ void lse_merge(float& run_max, float& run_sum) {
#pragma unroll
  for (int off = 1; off < LANES; off <<= 1) {
    const float om = __shfl_xor(run_max, off, 64), os = __shfl_xor(run_sum, off, 64);
    const float m = fmaxf(run_max, om);
    if (m != -INFINITY) run_sum = run_sum * __expf(run_max - m) + os * __expf(om - m);
    run_max = m;
  }
}

template <int LANES>
__device__ __forceinline__ float lanes_sum(float v) {
#pragma unroll
  for (int off = 1; off < LANES; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// logits x[k] = ma[k] + z sa[k] of sample s: z from the explicit array [S][N][K] or from
// Philox stream 0 keyed by (global n, s, k / 4) -- the z of elbo.hip's draw_noise, the
// same calls in the same order, so mgp_philox_noise reproduces it bit for bit.
template <int KMAX>
__device__ __forceinline__ void sample_logits(float (&x)[KMAX], const float (&ma)[KMAX], const float (&sa)[KMAX],
                                              const float* __restrict__ noise_z, int64_t N, int K, int64_t n,
                                              int s, uint32_t ng, uint32_t key0, uint32_t key1) {
  if (noise_z != nullptr) {
    const float* pz = noise_z + ((int64_t)s * N + n) * K;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) x[k] = (k < K) ? fmaf(pz[k], sa[k], ma[k]) : 0.f;
  } else {
#pragma unroll
    for (int kb = 0; kb < (KMAX + 3) / 4; ++kb) {
      if (4 * kb >= K) break;
      const u32x4 wz = philox4x32_10(u32x4{ng, (uint32_t)s, (uint32_t)kb, 0u}, key0, key1);
      float zz[4];
      box_muller4(wz, zz);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (4 * kb + e < KMAX) x[4 * kb + e] = fmaf(zz[e], sa[4 * kb + e], ma[4 * kb + e]);
      }
    }
  }
}

template <int KMAX, int LANES>
__global__ __launch_bounds__(kThreads) void mixture_predict_kernel(
    const float* __restrict__ mu_f, const float* __restrict__ var_f, const float* __restrict__ mu_a,
    const float* __restrict__ var_a, int64_t ldf, const float* __restrict__ lik_var,
    const float* __restrict__ Y, int64_t N, int K, int S, float jitter, const float* __restrict__ noise_z,
    uint32_t key0, uint32_t key1, int64_t n_offset, float* __restrict__ weights, float* __restrict__ mix_mean,
    float* __restrict__ mix_var, float* __restrict__ log_density, double* __restrict__ partials) {
  __shared__ double scratch[16];
  const int64_t gt = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t n = gt / LANES;
  const int sub = (int)(gt % LANES);
  const bool dens = Y != nullptr;
  float wsum[KMAX], mf[KMAX], s2[KMAX];
  float run_max = -INFINITY, run_sum = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) { wsum[k] = 0.f; mf[k] = 0.f; s2[k] = 1.f; }
  if (n < N) {
    float ma[KMAX], sa[KMAX], ln[KMAX];
    const float y = dens ? Y[n] : 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < K) {
        mf[k] = mu_f[(int64_t)k * ldf + n];
        s2[k] = var_f[(int64_t)k * ldf + n] + lik_var[k];
        ma[k] = mu_a[(int64_t)k * ldf + n];
        // S == 0: the plug-in weights, no noise and no jitter; else K6's clamp
        sa[k] = S > 0 ? sqrtf(fmaxf(var_a[(int64_t)k * ldf + n] + jitter, 0.f)) : 0.f;
        const float d = y - mf[k];
        ln[k] = -kHalfLog2Pi - 0.5f * logf(s2[k]) - 0.5f * d * d / s2[k];
      } else {
        ma[k] = 0.f; sa[k] = 0.f; ln[k] = 0.f;
      }
    }
    const uint32_t ng = (uint32_t)(n + n_offset);
    // S == 0: one pass over the means, by lane 0 of the point
    const int s_end = S > 0 ? S : 1;
    for (int s = sub; s < s_end; s += LANES) {
      float x[KMAX];
      if (S > 0) {
        sample_logits<KMAX>(x, ma, sa, noise_z, N, K, n, s, ng, key0, key1);
      } else {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) x[k] = ma[k];
      }
      float xm = -INFINITY;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) xm = fmaxf(xm, x[k]);
      float e[KMAX], den = 0.f, am = -INFINITY;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
          x[k] -= xm;
          e[k] = __expf(x[k]);
          den += e[k];
          x[k] += ln[k];
          am = fmaxf(am, x[k]);
        }
      }
      const float rden = __fdividef(1.f, den);
      float num = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
          wsum[k] = fmaf(e[k], rden, wsum[k]);
          if (dens) num += __expf(x[k] - am);
        }
      }
      if (dens) {
        // the sample's log sum_k softmax_k N_k = am + log(num) - log(den): fold the pair
        // (am - log den, num) into the running one (den in [1, K]: the fast logarithm's
        // absolute error is a few 1e-7)
        const float l = am - __logf(den);
        if (l > run_max) {
          run_sum = run_sum * __expf(run_max - l) + num;
          run_max = l;
        } else {
          run_sum = fmaf(num, __expf(l - run_max), run_sum);
        }
      }
    }
  }
  // every lane of the wave takes part in the shuffles (points beyond N included)
  if constexpr (LANES > 1) {
    lse_merge<LANES>(run_max, run_sum);
#pragma unroll
    for (int k = 0; k < KMAX; ++k) wsum[k] = lanes_sum<LANES>(wsum[k]);
  }
  float val = 0.f;
  if (n < N && sub == 0) {
    const float rs = S > 0 ? 1.f / (float)S : 1.f;
    float mean = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      wsum[k] *= rs;
      mean = fmaf(wsum[k], mf[k], mean);
    }
    float var = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const float d = mf[k] - mean;
      var = fmaf(wsum[k], fmaf(d, d, s2[k]), var);
    }
    if (weights) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) weights[n * K + k] = wsum[k];
    }
    if (mix_mean) mix_mean[n] = mean;
    if (mix_var) mix_var[n] = var;
    if (dens) {
      val = run_max + logf(run_sum) - (S > 0 ? logf((float)S) : 0.f);
      if (log_density) log_density[n] = val;
    }
  }
  if (partials) {
    const double bs = block_sum<double>((double)val, scratch);
    if (threadIdx.x == 0) partials[blockIdx.x] = bs;
  }
}

__global__ __launch_bounds__(1024) void mixture_sum_partials_kernel(const double* __restrict__ p, int n,
                                                                    double* __restrict__ out) {
  __shared__ double scratch[16];
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) v += p[i];
  v = block_sum<double>(v, scratch);
  if (threadIdx.x == 0) *out = v;
}

// density[n][g] = sum_k c_k exp(h_k (y_g - mu_k)^2), c_k = w_k / sqrt(2 pi s2_k),
// h_k = -1 / (2 s2_k).  TPP threads (32 .. 256, by G) walk the grid of one point, so
// a block covers 256 / TPP points and the stores run along G; the per-(n, k) constants
// (the reciprocal, the square root, the normaliser) are built once, in LDS.
__global__ __launch_bounds__(kThreads) void mixture_density_grid_kernel(
    const float* __restrict__ mu_f, const float* __restrict__ var_f, int64_t ldf, const float* __restrict__ lik_var,
    const float* __restrict__ weights, int64_t N, int K, const float* __restrict__ y_grid, int G, int tpp,
    float* __restrict__ density, int64_t ldd) {
  __shared__ float cm[kThreads / 32][32], cc[kThreads / 32][32], ch[kThreads / 32][32];
  const int ppb = kThreads / tpp;
  const int p = threadIdx.x / tpp, t = threadIdx.x % tpp;
  const int64_t n = (int64_t)blockIdx.x * ppb + p;
  if (n < N && t < K) {
    const float s2 = var_f[(int64_t)t * ldf + n] + lik_var[t];
    const float r = 1.f / s2;
    cm[p][t] = mu_f[(int64_t)t * ldf + n];
    cc[p][t] = weights[n * K + t] * sqrtf(0.15915494309189535f * r);
    ch[p][t] = -0.5f * r;
  }
  __syncthreads();
  if (n >= N) return;
  for (int g = t; g < G; g += tpp) {
    const float y = y_grid[g];
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
      const float d = y - cm[p][k];
      acc = fmaf(cc[p][k], __expf(ch[p][k] * d * d), acc);
    }
    density[n * ldd + g] = acc;
  }
}

static int64_t predict_blocks(int64_t N) { return (N * kLanes + kThreads - 1) / kThreads; }

}  // namespace mixture
}  // namespace mgp

using namespace mgp;

extern "C" size_t mgp_mixture_predict_workspace_bytes(int64_t N, int32_t K) {
  (void)K;
  const int64_t nb = N > 0 ? mixture::predict_blocks(N) : 1;
  return (size_t)nb * sizeof(double);
}

extern "C" int mgp_mixture_predict(const float* mu_f, const float* var_f, const float* mu_a, const float* var_a,
                                   int64_t ldf, const float* lik_var, const float* Y, int64_t N, int32_t K,
                                   int32_t S, float jitter, const float* noise_z, uint64_t seed, int64_t n_offset,
                                   float* weights, float* mix_mean, float* mix_var, float* log_density,
                                   double* log_density_sum, void* workspace, size_t workspace_bytes,
                                   mgp_stream_t stream) {
  if (!mu_f) return -1;
  if (!var_f) return -2;
  if (!mu_a) return -3;
  if (!var_a) return -4;
  if (N > 0 && ldf < N) return -5;
  if (!lik_var) return -6;
  if ((log_density || log_density_sum) && !Y) return -7;
  if (K < 1) return -9;
  if (K > 32) return MGP_ERR_UNSUPPORTED;
  if (S < 0) return -10;
  if (!(jitter >= 0.f)) return -11;
  if (n_offset < 0) return -14;
  if (N <= 0) return MGP_OK;
  const int64_t nb = mixture::predict_blocks(N);
  if (nb > 0x7fffffff) return MGP_ERR_UNSUPPORTED;
  if (log_density_sum && (!workspace || workspace_bytes < mgp_mixture_predict_workspace_bytes(N, K)))
    return MGP_ERR_WORKSPACE;
  double* partials = log_density_sum ? (double*)workspace : nullptr;
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
  hipStream_t s = (hipStream_t)stream;
#define MGP_MIX_CASE(KM)                                                                                       \
  if (K <= KM) {                                                                                                \
    hipLaunchKernelGGL((mixture::mixture_predict_kernel<KM, mixture::kLanes>), dim3((unsigned)nb),              \
                       dim3(mixture::kThreads), 0, s, mu_f, var_f, mu_a, var_a, ldf, lik_var, Y, N, K, S, jitter, \
                       noise_z, k0, k1, n_offset, weights, mix_mean, mix_var, log_density, partials);           \
  } else
  MGP_MIX_CASE(1) MGP_MIX_CASE(2) MGP_MIX_CASE(4) MGP_MIX_CASE(8) MGP_MIX_CASE(16) MGP_MIX_CASE(32) {}
#undef MGP_MIX_CASE
  int st = launch_status();
  if (st || !log_density_sum) return st;
  hipLaunchKernelGGL(mixture::mixture_sum_partials_kernel, dim3(1), dim3(1024), 0, s, partials, (int)nb,
                     log_density_sum);
  return launch_status();
}

extern "C" int mgp_mixture_density_grid(const float* mu_f, const float* var_f, int64_t ldf, const float* lik_var,
                                        const float* weights, int64_t N, int32_t K, const float* y_grid, int32_t G,
                                        float* density, int64_t ldd, mgp_stream_t stream) {
  if (!mu_f) return -1;
  if (!var_f) return -2;
  if (N > 0 && ldf < N) return -3;
  if (!lik_var) return -4;
  if (!weights) return -5;
  if (K < 1) return -7;
  if (K > 32) return MGP_ERR_UNSUPPORTED;
  if (!y_grid) return -8;
  if (G < 0) return -9;
  if (!density) return -10;
  if (ldd < G) return -11;
  if (N <= 0 || G == 0) return MGP_OK;
  const int tpp = G <= 32 ? 32 : G <= 64 ? 64 : G <= 128 ? 128 : 256;
  const int ppb = mixture::kThreads / tpp;
  const int64_t nb = (N + ppb - 1) / ppb;
  if (nb > 0x7fffffff) return MGP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(mixture::mixture_density_grid_kernel, dim3((unsigned)nb), dim3(mixture::kThreads), 0,
                     (hipStream_t)stream, mu_f, var_f, ldf, lik_var, weights, N, K, y_grid, G, tpp, density, ldd);
  return launch_status();
}
