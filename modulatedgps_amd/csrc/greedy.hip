// Greedy conditional-variance selection of inducing points (Burt, Rasmussen, van der Wilk
// 2020): a pivoted Cholesky of Kff that picks, M times, the input whose variance given the
// points already chosen is largest.  The semantics are stated in mgp_hip.h and DESIGN
// "Greedy variance selection"; tests/greedy_ref.py restates them in float64.
//
//   d[n] = variance
//   step i:  j = argmax_n d[n] (ties: lowest n);  stop if d[j] <= threshold * variance
//            c[n] = k(x_n, x_j) - sum_{t < i} L[t][n] L[t][j];  L[i][n] = c[n] / sqrt(d[j])
//            d[n] = max(d[n] - L[i][n]^2, 0)
//
// One step is one launch of step_kernel; the launch boundary is the only grid-wide ordering
// (no cooperative launch, no barrier across workgroups, no waiting on memory).  Step i - 1
// leaves one partial per workgroup, (max d, lowest row attaining it, sum of d); every
// workgroup of step i reduces them again to the same pivot -- a few KiB of L2 reads instead
// of a second launch.  A workgroup owns tiles of kTileRows rows; its kWaves waves split the
// t range (wave w takes t = w, w + kWaves, ...), each accumulating in float64 in ascending
// t, and the partial dots are added in LDS in wave order, so the order of every sum depends
// on i alone.  k(x_n, x_j) is float64 throughout (differences, scaled square, exp); L is
// stored float32 and d is updated with the rounded value.
//
// The step index is base + b: b counts the launches of one mgp_greedy_steps call (a kernel
// argument), base is the device word that only init_kernel and commit_kernel write -- the
// one launch that closes each call -- so no step reads a word that its own launch writes.
// A step that meets the threshold records its index in stop_step; later steps see
// stop_step < i and return at once.
#include <math.h>

#include "mgp_common.hpp"

namespace mgp {
namespace greedy {

constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr int kRowsPerLane = 4;                 // one float4 of a factor row per lane
constexpr int kTileRows = 64 * kRowsPerLane;    // every wave sweeps the whole tile
constexpr int kTChunk = 1024;                   // factor entries of the pivot row in LDS: 4 KiB
constexpr int kUnroll = 8;                      // float4 loads in flight per lane
constexpr int kMaxBlocks = 1024;                // partials every workgroup reduces again
constexpr int kMaxD = 32;
constexpr int64_t kMaxN = 0x7fffffff;
constexpr int32_t kNoStop = 0x7fffffff;

struct State {
  int32_t m;          // steps taken up to the last commit (= points chosen, unless stopped earlier)
  int32_t stop_step;  // the step at which d[j] <= threshold was met, kNoStop before
  double thresh;      // threshold * variance
};
static_assert(sizeof(State) == 16, "State layout");

static int64_t tiles(int64_t N) { return (N + kTileRows - 1) / kTileRows; }
static int64_t blocks(int64_t N) { const int64_t t = tiles(N); return t < kMaxBlocks ? t : kMaxBlocks; }

// the arrays of length M come last, so that their offsets do not depend on M
struct Layout {
  size_t state, pmax, psum, pidx, d, piv, dmax, trace, total;
  int64_t NB;
};
static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
static Layout layout(int64_t N, int64_t M) {
  Layout L;
  L.NB = blocks(N);
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
  L.state = take(sizeof(State));
  L.pmax = take((size_t)2 * kMaxBlocks * 8);
  L.psum = take((size_t)2 * kMaxBlocks * 8);
  L.pidx = take((size_t)2 * kMaxBlocks * 8);
  L.d = take((size_t)N * 8);
  L.piv = take((size_t)M * 8);
  L.dmax = take((size_t)M * 8);
  L.trace = take((size_t)M * 8);
  L.total = o;
  return L;
}

struct Best {
  double d;
  int64_t n;
};
// the larger d; of equal d the lower row
__device__ __forceinline__ Best better(Best a, Best b) {
  return (b.d > a.d || (b.d == a.d && b.n < a.n)) ? b : a;
}
__device__ __forceinline__ Best wave_best(Best v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Best o;
    o.d = __shfl_xor(v.d, off, kWave);
    o.n = __shfl_xor(v.n, off, kWave);
    v = better(v, o);
  }
  return v;
}
// every thread gets the block's best; sh: kWaves entries each.  The maximum is exact, so
// the order of the merge does not matter.
__device__ __forceinline__ Best block_best(Best v, double* sh_d, int64_t* sh_n) {
  v = wave_best(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) { sh_d[w] = v.d; sh_n[w] = v.n; }
  __syncthreads();
  Best r = {sh_d[0], sh_n[0]};
#pragma unroll
  for (int i = 1; i < kWaves; ++i) r = better(r, Best{sh_d[i], sh_n[i]});
  return r;
}
// the block's sum in a fixed order (butterfly within a wave, the waves in order); thread 0
__device__ __forceinline__ double block_total(double v, double* sh) {
  __syncthreads();
  return block_sum<double>(v, sh);
}

// sum of the NB partial sums: thread t takes t, t + kThreads, ... in order, then block_total
__device__ __forceinline__ double partials_total(const double* __restrict__ psum, int NB, double* sh) {
  double s = 0.0;
  for (int b = threadIdx.x; b < NB; b += kThreads) s += psum[b];
  return block_total(s, sh);
}

__global__ __launch_bounds__(kThreads) void init_kernel(int64_t N, const float* __restrict__ variance,
                                                        double rel_threshold, State* __restrict__ st,
                                                        double* __restrict__ d, double* __restrict__ pmax,
                                                        double* __restrict__ psum, int64_t* __restrict__ pidx) {
  __shared__ double sh[16];
  const double var = (double)variance[0];
  const int64_t nt = (N + kTileRows - 1) / kTileRows;
  double s = 0.0;
  for (int64_t tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    const int64_t n = tile * kTileRows + threadIdx.x;
    if (threadIdx.x < kTileRows && n < N) {
      d[n] = var;
      s += var;
    }
  }
  s = block_total(s, sh);
  if (threadIdx.x == 0) {
    pmax[blockIdx.x] = var;
    pidx[blockIdx.x] = (int64_t)blockIdx.x * kTileRows;   // the first row of the block's first tile
    psum[blockIdx.x] = s;
    if (blockIdx.x == 0) {
      State o;
      o.m = 0;
      o.stop_step = kNoStop;
      o.thresh = rel_threshold * var;
      *st = o;
    }
  }
}

template <int DP>
__global__ __launch_bounds__(kThreads) void step_kernel(
    const float* __restrict__ X, int64_t ldx, int64_t N, int D, const float* __restrict__ variance,
    const float* __restrict__ lengthscales, int n_ls, int64_t M, int b, float* __restrict__ L, int64_t ldl,
    const State* __restrict__ st, int32_t* __restrict__ stop_step, double* __restrict__ d,
    double* __restrict__ pmax, double* __restrict__ psum, int64_t* __restrict__ pidx, int64_t* __restrict__ piv,
    double* __restrict__ dmax, double* __restrict__ trace) {
  __shared__ __attribute__((aligned(16))) float lj[kTChunk];
  __shared__ double accs[kWaves][kTileRows];
  __shared__ double sh_d[16];
  __shared__ int64_t sh_n[kWaves];
  __shared__ double xj[DP], ls[DP];

  const int64_t i = (int64_t)st->m + b;
  // stop_step == i can only be this launch's own write, which says the same as the test below
  if (i >= M || __hip_atomic_load(stop_step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < i) return;
  const int NB = gridDim.x;
  const int par = (int)(i & 1);
  const double* pm = pmax + par * kMaxBlocks;
  const int64_t* pi = pidx + par * kMaxBlocks;
  Best best = {-1.0, N};
  for (int q = threadIdx.x; q < NB; q += kThreads) best = better(best, Best{pm[q], pi[q]});
  best = block_best(best, sh_d, sh_n);
  const int64_t j = best.n;
  const double dj = best.d;
  if (blockIdx.x == 0 && i > 0) {
    const double tr = partials_total(psum + par * kMaxBlocks, NB, sh_d);
    if (threadIdx.x == 0) trace[i - 1] = tr;
  }
  if (!(dj > st->thresh) || j < 0 || j >= N) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      __hip_atomic_store(stop_step, (int32_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    piv[i] = j;
    dmax[i] = dj;
  }
  const double var = (double)variance[0];
  if (threadIdx.x < DP) {
    const int c = threadIdx.x;
    xj[c] = c < D ? (double)X[j * ldx + c] : 0.0;
    ls[c] = c < D ? (double)lengthscales[n_ls == 1 ? 0 : c] : 1.0;
  }
  const double root = sqrt(dj);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t nt = (N + kTileRows - 1) / kTileRows;
  const bool one_chunk = i <= kTChunk;
  float* Li = L + i * ldl;

  Best mine = {-1.0, N};
  double dsum = 0.0;
  bool first = true;
  for (int64_t tile = blockIdx.x; tile < nt; tile += NB, first = false) {
    const int64_t n0 = tile * kTileRows + lane * kRowsPerLane;   // < round4(N) <= ldl or unused
    const bool live = n0 < N;
    double acc[kRowsPerLane] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t t0 = 0; t0 < i; t0 += kTChunk) {
      const int tc = (int)(i - t0 < kTChunk ? i - t0 : kTChunk);
      if (first || !one_chunk) {
        __syncthreads();
        for (int e = threadIdx.x; e < tc; e += kThreads) lj[e] = L[(t0 + e) * ldl + j];
        __syncthreads();
      }
      if (live) {
        const float* col = L + t0 * ldl + n0;
        int t = w;
        for (; t + (kUnroll - 1) * kWaves < tc; t += kUnroll * kWaves) {
          floatx4 v[kUnroll];
#pragma unroll
          for (int u = 0; u < kUnroll; ++u)
            v[u] = *reinterpret_cast<const floatx4*>(col + (int64_t)(t + u * kWaves) * ldl);
#pragma unroll
          for (int u = 0; u < kUnroll; ++u) {
            const double f = (double)lj[t + u * kWaves];
            acc[0] += (double)v[u].x * f;
            acc[1] += (double)v[u].y * f;
            acc[2] += (double)v[u].z * f;
            acc[3] += (double)v[u].w * f;
          }
        }
        for (; t < tc; t += kWaves) {
          const floatx4 v = *reinterpret_cast<const floatx4*>(col + (int64_t)t * ldl);
          const double f = (double)lj[t];
          acc[0] += (double)v.x * f;
          acc[1] += (double)v.y * f;
          acc[2] += (double)v.z * f;
          acc[3] += (double)v.w * f;
        }
      }
    }
    __syncthreads();   // the previous tile's accs have been read
#pragma unroll
    for (int q = 0; q < kRowsPerLane; ++q) accs[w][lane * kRowsPerLane + q] = acc[q];
    __syncthreads();
    if (threadIdx.x < kTileRows) {
      const int64_t n = tile * kTileRows + threadIdx.x;
      if (n < N) {
        double dot = accs[0][threadIdx.x];
#pragma unroll
        for (int q = 1; q < kWaves; ++q) dot += accs[q][threadIdx.x];
        double r2 = 0.0;
#pragma unroll
        for (int c = 0; c < DP; ++c) {
          if (c < D) {
            const double s = ((double)X[n * ldx + c] - xj[c]) / ls[c];
            r2 += s * s;
          }
        }
        const double kv = var * exp(-0.5 * r2);
        const float l = (float)((kv - dot) / root);
        Li[n] = l;
        const double lf = (double)l;
        double dn = d[n] - lf * lf;
        dn = dn > 0.0 ? dn : 0.0;
        d[n] = dn;
        dsum += dn;
        mine = better(mine, Best{dn, n});   // rows ascend within a thread: the first maximum stays
      } else if (n < ldl) {
        Li[n] = 0.f;                        // the pad of the last float4
      }
    }
  }
  mine = block_best(mine, sh_d, sh_n);
  dsum = block_total(dsum, sh_d);
  if (threadIdx.x == 0) {
    const int np = par ^ 1;
    pmax[np * kMaxBlocks + blockIdx.x] = mine.d;
    pidx[np * kMaxBlocks + blockIdx.x] = mine.n;
    psum[np * kMaxBlocks + blockIdx.x] = dsum;
  }
}

// closes a mgp_greedy_steps call of B launches: the steps taken so far and the stopped flag
__global__ void commit_kernel(State* __restrict__ st, int64_t M, int B, int32_t* __restrict__ state) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t m = (int64_t)st->m + B;
  if (m > M) m = M;
  const bool stopped = st->stop_step < m;
  if (stopped) m = st->stop_step;
  st->m = (int32_t)m;
  state[0] = (int32_t)m;
  state[1] = stopped ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void result_kernel(
    const float* __restrict__ X, int64_t ldx, int64_t N, int D, int NB, const State* __restrict__ st,
    const double* __restrict__ d, const double* __restrict__ psum, const int64_t* __restrict__ piv,
    const double* __restrict__ dmax_ws, const double* __restrict__ trace_ws, int64_t* __restrict__ indices,
    float* __restrict__ Z, int64_t ldz, double* __restrict__ dmax, double* __restrict__ trace,
    double* __restrict__ residual, int32_t* __restrict__ info) {
  __shared__ double sh[16];
  const int64_t m = st->m;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t e0 = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  for (int64_t t = e0; t < m; t += stride) {
    indices[t] = piv[t];
    dmax[t] = dmax_ws[t];
    if (t < m - 1) trace[t] = trace_ws[t];
  }
  for (int64_t e = e0; e < m * D; e += stride) {
    const int64_t t = e / D, c = e % D;
    const int64_t row = piv[t];
    Z[t * ldz + c] = (row >= 0 && row < N) ? X[row * ldx + c] : 0.f;
  }
  if (residual != nullptr)
    for (int64_t n = e0; n < N; n += stride) residual[n] = d[n];
  if (blockIdx.x == 0) {
    // the last step's trace: the sum no later step has reduced (the order a later step uses)
    const double tr = partials_total(psum + (m & 1) * kMaxBlocks, NB, sh);
    if (threadIdx.x == 0) {
      if (m > 0) trace[m - 1] = tr;
      info[0] = (int32_t)m;
      info[1] = st->stop_step <= m ? 1 : 0;
    }
  }
}

static bool in_limits(int64_t N, int D) { return D <= kMaxD && N <= kMaxN; }

}  // namespace greedy
}  // namespace mgp

using namespace mgp;
using greedy::Layout;
using greedy::State;

extern "C" size_t mgp_greedy_workspace_bytes(int64_t N, int64_t M, int32_t D) {
  if (N < 1 || M < 1 || D < 1 || !greedy::in_limits(N, D) || M > N) return 0;
  return greedy::layout(N, M).total;
}

extern "C" int mgp_greedy_init(int64_t N, int32_t D, const float* variance, double rel_threshold, void* workspace,
                               size_t workspace_bytes, mgp_stream_t stream) {
  if (N < 0) return -1;
  if (D < 1) return -2;
  if (!variance) return -3;
  if (!(rel_threshold >= 0.0)) return -4;
  if (!greedy::in_limits(N, D)) return MGP_ERR_UNSUPPORTED;
  if (N == 0) return MGP_OK;
  const Layout L = greedy::layout(N, 1);
  if (!workspace || workspace_bytes < L.total) return MGP_ERR_WORKSPACE;
  if (!aligned16(workspace)) return MGP_ERR_ALIGN;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(greedy::init_kernel, dim3((unsigned)L.NB), dim3(greedy::kThreads), 0, (hipStream_t)stream, N,
                     variance, rel_threshold, (State*)(ws + L.state), (double*)(ws + L.d), (double*)(ws + L.pmax),
                     (double*)(ws + L.psum), (int64_t*)(ws + L.pidx));
  return launch_status();
}

extern "C" int mgp_greedy_steps(const float* X, int64_t ldx, int64_t N, int32_t D, const float* variance,
                                const float* lengthscales, int32_t n_ls, int64_t M, int32_t B, float* L, int64_t ldl,
                                void* workspace, size_t workspace_bytes, int32_t* state, mgp_stream_t stream) {
  if (!X) return -1;
  if (N < 0) return -3;
  if (D < 1) return -4;
  if (!variance) return -5;
  if (!lengthscales) return -6;
  if (n_ls != 1 && n_ls != D) return -7;
  if (M < 1) return -8;
  if (B < 1) return -9;
  if (!L) return -10;
  if (!state) return -14;
  if (!greedy::in_limits(N, D)) return MGP_ERR_UNSUPPORTED;
  if (ldx < D) return -2;
  if (N == 0) return MGP_OK;
  if (M > N) return MGP_ERR_UNSUPPORTED;
  if (ldl < N) return -11;
  const Layout lay = greedy::layout(N, M);
  if (!workspace || workspace_bytes < lay.total) return MGP_ERR_WORKSPACE;
  if ((ldl & 3) || !aligned16(L) || !aligned16(workspace)) return MGP_ERR_ALIGN;
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  State* st = (State*)(ws + lay.state);
  const int64_t nb = B < M ? B : M;   // steps beyond M would return at once
  const dim3 grid((unsigned)lay.NB), block(greedy::kThreads);
  for (int64_t b = 0; b < nb; ++b) {
    const int rc = dispatch_dmax(D, [&](auto dm) {
      hipLaunchKernelGGL((greedy::step_kernel<decltype(dm)::value>), grid, block, 0, s, X, ldx, N, D, variance,
                         lengthscales, n_ls, M, (int)b, L, ldl, (const State*)st, &st->stop_step,
                         (double*)(ws + lay.d), (double*)(ws + lay.pmax), (double*)(ws + lay.psum),
                         (int64_t*)(ws + lay.pidx), (int64_t*)(ws + lay.piv), (double*)(ws + lay.dmax),
                         (double*)(ws + lay.trace));
      return launch_status();
    });
    if (rc) return rc;
  }
  hipLaunchKernelGGL(greedy::commit_kernel, dim3(1), dim3(64), 0, s, st, M, (int)nb, state);
  return launch_status();
}

extern "C" int mgp_greedy_result(const float* X, int64_t ldx, int64_t N, int32_t D, int64_t M, const void* workspace,
                                 size_t workspace_bytes, int64_t* indices, float* Z, int64_t ldz, double* dmax,
                                 double* trace, double* residual, int32_t* info, mgp_stream_t stream) {
  if (!X) return -1;
  if (N < 0) return -3;
  if (D < 1) return -4;
  if (M < 1) return -5;
  if (!indices) return -8;
  if (!Z) return -9;
  if (!dmax) return -11;
  if (!trace) return -12;
  if (!info) return -14;
  if (!greedy::in_limits(N, D)) return MGP_ERR_UNSUPPORTED;
  if (ldx < D) return -2;
  if (N == 0) return MGP_OK;
  if (M > N) return MGP_ERR_UNSUPPORTED;
  if (ldz < D) return -10;
  const Layout lay = greedy::layout(N, M);
  if (!workspace || workspace_bytes < lay.total) return MGP_ERR_WORKSPACE;
  if (!aligned16(workspace)) return MGP_ERR_ALIGN;
  const char* ws = (const char*)workspace;
  int64_t nb = (N + greedy::kThreads - 1) / greedy::kThreads;
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(greedy::result_kernel, dim3((unsigned)nb), dim3(greedy::kThreads), 0, (hipStream_t)stream, X,
                     ldx, N, D, (int)lay.NB, (const State*)(ws + lay.state), (const double*)(ws + lay.d),
                     (const double*)(ws + lay.psum), (const int64_t*)(ws + lay.piv), (const double*)(ws + lay.dmax),
                     (const double*)(ws + lay.trace), indices, Z, ldz, dmax, trace, residual, info);
  return launch_status();
}
