// On-device k-means: scipy.cluster.vq.kmeans / vq, the inducing-point initialisation of
// every reference demo (demos/demo_tf2.py:39, kmeans(Xtrain, num_ind, seed=0)[0]).  The
// semantics are stated in mgp_hip.h and DESIGN "k-means"; tests/kmeans_ref.py restates
// them in float64.
//
// One Lloyd iteration of R restarts ("runs") is five launches, each with the run index in
// blockIdx.y; a run whose done flag is set returns at once, so the runs advance in lockstep
// and the host only reads the R flags back after a block of iterations:
//   assign_kernel   a lane keeps kPPL point rows in registers, the codebook goes through
//                   LDS in 16 KiB tiles; LANES consecutive lanes share a point slot and
//                   split the codes of a tile, butterfly shuffles merge the pairs
//                   (d^2, index) lexicographically, so ties go to the lowest index as in
//                   vq.  d^2 = sum_d (x_d - c_d)^2 on the f32 differences (shift-invariant;
//                   never |x|^2 - 2 x.c + |c|^2).  Writes code, dist = sqrt(min d^2), a
//                   float64 block partial of dist, and counts the members per
//                   (chunk of 1024 points, code) with integer atomics.
//   scan_kernel     per code: exclusive prefix of its counts over the chunks, its member
//                   count; then the exclusive scan of the counts over the codes.
//   scatter_kernel  the stable counting sort: point n goes to segment offset + chunk
//                   prefix + rank among the earlier points of its chunk with its code.
//   segsum_kernel   one wave per code sums its members' rows in float64: lane l takes
//                   members l, l + 64, ... in order, a butterfly merges the lanes -- a
//                   fixed order, no floating-point atomics.
//   finish_kernel   one workgroup per run: avg = sum(partials) / N, diff = |avg_prev - avg|,
//                   compacts the new codebook over the empty codes (rows keep their order),
//                   updates k_active, the iteration count and the done flag.
// select_kernel picks the first run with the strictly smallest distortion.
#include <math.h>

#include "mgp_common.hpp"

namespace mgp {
namespace kmeans {

constexpr int kThreads = 256;
constexpr int kChunk = 1024;        // points per counting-sort chunk (= scatter block)
constexpr int kTileFloats = 4096;   // codebook tile in LDS: 16 KiB
constexpr int kPPL = 2;             // points per lane: one LDS read serves both
constexpr int kMaxD = 32;
constexpr int kMaxR = 64;
constexpr int64_t kMaxN = 0x7fffffff;

// per run, device resident
struct RunState {
  int32_t k_active;  // surviving codes
  int32_t iters;     // Lloyd iterations done
  int32_t done;      // diff <= thresh reached
  int32_t pad;
  double avg;        // mean distance of the last assignment (inf before the first)
  double diff;       // |avg_prev - avg| of the last iteration
};
static_assert(sizeof(RunState) == 32, "RunState layout");

// lanes per point slot: more lanes where N alone would leave CUs idle.  The result does
// not depend on it (the lexicographic minimum is exact and associative).
static int lanes_for(int64_t N) { return N >= 131072 ? 1 : N >= 8192 ? 4 : 16; }
static int64_t assign_blocks(int64_t N) {
  const int64_t ppb = (int64_t)(kThreads / lanes_for(N)) * kPPL;
  return (N + ppb - 1) / ppb;
}
static int64_t chunks(int64_t N) { return (N + kChunk - 1) / kChunk; }

struct Layout {
  size_t state, cb, cbnew, counts, segoff, cnt, code, dist, sorted, partials, total;
  int64_t G, NB;
};
static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
static Layout layout(int64_t N, int64_t k, int D, int R) {
  Layout L;
  L.G = chunks(N);
  L.NB = assign_blocks(N);
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
  L.state = take((size_t)R * sizeof(RunState));
  L.cb = take((size_t)R * k * D * 4);
  L.cbnew = take((size_t)R * k * D * 4);
  L.counts = take((size_t)R * k * 4);
  L.segoff = take((size_t)R * k * 4);
  L.cnt = take((size_t)R * L.G * k * 4);
  L.code = take((size_t)R * N * 4);
  L.dist = take((size_t)R * N * 4);
  L.sorted = take((size_t)R * N * 4);
  L.partials = take((size_t)R * L.NB * 8);
  L.total = o;
  return L;
}

template <int DP, int LANES>
__global__ __launch_bounds__(kThreads) void assign_kernel(
    const float* __restrict__ obs, int64_t ldo, int64_t N, int D, const float* __restrict__ cb, int64_t ldc,
    int64_t cb_stride, int64_t k, const RunState* __restrict__ st, int32_t* __restrict__ code,
    float* __restrict__ dist, int64_t n_stride, double* __restrict__ partials, int64_t p_stride,
    int32_t* __restrict__ cnt, int64_t cnt_stride) {
  __shared__ __attribute__((aligned(16))) float tile[kTileFloats];
  __shared__ double scratch[16];
  const int r = blockIdx.y;
  int64_t ka = k;
  if (st != nullptr) {
    if (st[r].done) return;
    ka = st[r].k_active;
  }
  cb += (int64_t)r * cb_stride;
  constexpr int SLOTS = kThreads / LANES;
  constexpr int TILE = kTileFloats / DP;
  const int slot = threadIdx.x / LANES, sub = threadIdx.x % LANES;
  float x[kPPL][DP], best[kPPL];
  int32_t bi[kPPL];
  int64_t n[kPPL];
#pragma unroll
  for (int p = 0; p < kPPL; ++p) {
    n[p] = (int64_t)blockIdx.x * (SLOTS * kPPL) + p * SLOTS + slot;
    best[p] = INFINITY;
    bi[p] = 0;
#pragma unroll
    for (int d = 0; d < DP; ++d) x[p][d] = (n[p] < N && d < D) ? obs[n[p] * ldo + d] : 0.f;
  }
  for (int64_t c0 = 0; c0 < ka; c0 += TILE) {
    const int kt = (int)(ka - c0 < TILE ? ka - c0 : TILE);
    __syncthreads();
    for (int e = threadIdx.x; e < kt * DP; e += kThreads) {
      const int c = e / DP, d = e % DP;
      tile[e] = d < D ? cb[(c0 + c) * ldc + d] : 0.f;
    }
    __syncthreads();
    for (int j = sub; j < kt; j += LANES) {
      const float* cj = tile + j * DP;
      float cv[DP];
      if constexpr (DP >= 4) {
#pragma unroll
        for (int q = 0; q < DP / 4; ++q) {
          const floatx4 v = reinterpret_cast<const floatx4*>(cj)[q];
          cv[4 * q] = v.x; cv[4 * q + 1] = v.y; cv[4 * q + 2] = v.z; cv[4 * q + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int d = 0; d < DP; ++d) cv[d] = cj[d];
      }
#pragma unroll
      for (int p = 0; p < kPPL; ++p) {
        float d2 = 0.f;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          const float t = x[p][d] - cv[d];
          d2 = fmaf(t, t, d2);
        }
        // strict: within a lane the indices ascend, so the first minimum stays
        if (d2 < best[p]) { best[p] = d2; bi[p] = (int32_t)(c0 + j); }
      }
    }
  }
  // every lane of the wave takes part in the shuffles (slots beyond N included)
  double val = 0.0;
#pragma unroll
  for (int p = 0; p < kPPL; ++p) {
    if constexpr (LANES > 1) {
#pragma unroll
      for (int off = 1; off < LANES; off <<= 1) {
        const float od = __shfl_xor(best[p], off, 64);
        const int32_t oi = __shfl_xor(bi[p], off, 64);
        if (od < best[p] || (od == best[p] && oi < bi[p])) { best[p] = od; bi[p] = oi; }
      }
    }
    if (sub == 0 && n[p] < N) {
      const float dv = sqrtf(best[p]);
      code[(int64_t)r * n_stride + n[p]] = bi[p];
      if (dist != nullptr) dist[(int64_t)r * n_stride + n[p]] = dv;
      val += (double)dv;
      if (cnt != nullptr) atomicAdd(cnt + (int64_t)r * cnt_stride + (n[p] / kChunk) * k + bi[p], 1);
    }
  }
  if (partials != nullptr) {
    const double bs = block_sum<double>(val, scratch);
    if (threadIdx.x == 0) partials[(int64_t)r * p_stride + blockIdx.x] = bs;
  }
}

// member counts per (chunk, code) of given labels (mgp_kmeans_update; the Lloyd iteration
// counts inside assign_kernel).  Labels outside [0, k) own nothing.
__global__ __launch_bounds__(kThreads) void hist_kernel(const int32_t* __restrict__ code, int64_t N, int64_t k,
                                                        int32_t* __restrict__ cnt) {
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n >= N) return;
  const int32_t c = code[n];
  if (c >= 0 && c < k) atomicAdd(cnt + (n / kChunk) * k + c, 1);
}

// inclusive scan of one int per thread over a 1024-thread block; sh[1023] = total after it
__device__ __forceinline__ int block_scan_1024(int v, int32_t* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int a = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
    __syncthreads();
    sh[threadIdx.x] += a;
    __syncthreads();
  }
  return sh[threadIdx.x];
}

__global__ __launch_bounds__(1024) void scan_kernel(const RunState* __restrict__ st, int32_t* __restrict__ cnt,
                                                    int64_t cnt_stride, int64_t G, int64_t k,
                                                    int32_t* __restrict__ counts, int32_t* __restrict__ segoff,
                                                    int64_t k_stride) {
  __shared__ int32_t sh[1024];
  const int r = blockIdx.x;
  int64_t ka = k;
  if (st != nullptr) {
    if (st[r].done) return;
    ka = st[r].k_active;
  }
  cnt += (int64_t)r * cnt_stride;
  counts += (int64_t)r * k_stride;
  segoff += (int64_t)r * k_stride;
  int carry = 0;
  for (int64_t base = 0; base < ka; base += 1024) {
    const int64_t c = base + threadIdx.x;
    int tot = 0;
    if (c < ka) {
      for (int64_t g = 0; g < G; ++g) {
        const int t = cnt[g * k + c];
        cnt[g * k + c] = tot;
        tot += t;
      }
      counts[c] = tot;
    }
    const int incl = block_scan_1024(tot, sh);
    if (c < ka) segoff[c] = carry + incl - tot;
    carry += sh[1023];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kChunk) void scatter_kernel(const RunState* __restrict__ st,
                                                         const int32_t* __restrict__ code, int64_t N,
                                                         int64_t n_stride, int64_t k,
                                                         const int32_t* __restrict__ cnt, int64_t cnt_stride,
                                                         const int32_t* __restrict__ segoff, int64_t k_stride,
                                                         int32_t* __restrict__ sorted) {
  __shared__ __attribute__((aligned(16))) int32_t codes[kChunk];
  const int r = blockIdx.y;
  int64_t ka = k;
  if (st != nullptr) {
    if (st[r].done) return;
    ka = st[r].k_active;
  }
  const int t = threadIdx.x;
  const int64_t n = (int64_t)blockIdx.x * kChunk + t;
  int32_t c = n < N ? code[(int64_t)r * n_stride + n] : -1;
  if (c < 0 || c >= ka) c = -1;
  codes[t] = c;
  __syncthreads();
  // rank among the earlier points of the chunk with the same code; the loop bound is the
  // wave's, so every lane of a wave reads the same address (broadcast)
  int rank = 0;
  const int m_end = ((t & ~63) + 64) / 4;
  for (int m4 = 0; m4 < m_end; ++m4) {
    const int4 v = reinterpret_cast<const int4*>(codes)[m4];
    const int m = 4 * m4;
    rank += (v.x == c && m < t) + (v.y == c && m + 1 < t) + (v.z == c && m + 2 < t) + (v.w == c && m + 3 < t);
  }
  if (c >= 0) {
    const int64_t pos = (int64_t)segoff[(int64_t)r * k_stride + c] +
                        cnt[(int64_t)r * cnt_stride + (int64_t)blockIdx.x * k + c] + rank;
    if (pos < N) sorted[(int64_t)r * n_stride + pos] = (int32_t)n;
  }
}

template <int DP>
__global__ __launch_bounds__(kThreads) void segsum_kernel(const float* __restrict__ obs, int64_t ldo, int64_t N,
                                                          int D, const RunState* __restrict__ st, int64_t k,
                                                          const int32_t* __restrict__ sorted, int64_t n_stride,
                                                          const int32_t* __restrict__ counts,
                                                          const int32_t* __restrict__ segoff, int64_t k_stride,
                                                          float* __restrict__ out, int64_t ldout,
                                                          int64_t out_stride) {
  const int r = blockIdx.y;
  int64_t ka = k;
  if (st != nullptr) {
    if (st[r].done) return;
    ka = st[r].k_active;
  }
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (c >= ka) return;   // wave-uniform
  const int m = counts[(int64_t)r * k_stride + c];
  const int64_t off = segoff[(int64_t)r * k_stride + c];
  sorted += (int64_t)r * n_stride;
  double acc[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) acc[d] = 0.0;
  for (int i = lane; i < m; i += 64) {
    const int64_t n = sorted[off + i];
    if (n < 0 || n >= N) continue;
    const float* row = obs + n * ldo;
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) acc[d] += (double)row[d];
  }
  float o = 0.f;
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    const double s = wave_sum(acc[d]);
    if (lane == d) o = m > 0 ? (float)(s / (double)m) : 0.f;
  }
  if (lane < D) out[(int64_t)r * out_stride + c * ldout + lane] = o;
}

__global__ __launch_bounds__(1024) void finish_kernel(RunState* __restrict__ st, const double* __restrict__ partials,
                                                      int64_t p_stride, int64_t NB, int64_t N, int D, int64_t k,
                                                      const float* __restrict__ cbnew, float* __restrict__ cb,
                                                      const int32_t* __restrict__ counts, double thresh,
                                                      int32_t* __restrict__ done_out) {
  __shared__ double scratch[16];
  __shared__ int32_t sh[1024];
  const int r = blockIdx.x;
  const RunState s = st[r];
  if (s.done) return;
  const int64_t ka = s.k_active;
  partials += (int64_t)r * p_stride;
  cbnew += (int64_t)r * k * D;
  cb += (int64_t)r * k * D;
  counts += (int64_t)r * k;
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < NB; i += 1024) v += partials[i];
  v = block_sum<double>(v, scratch);
  // drop the codes without members: the rows move up and keep their order
  int carry = 0;
  for (int64_t base = 0; base < ka; base += 1024) {
    const int64_t c = base + threadIdx.x;
    const int flag = (c < ka && counts[c] > 0) ? 1 : 0;
    const int incl = block_scan_1024(flag, sh);
    if (flag) {
      const int64_t pos = carry + incl - 1;
      for (int d = 0; d < D; ++d) cb[pos * D + d] = cbnew[c * D + d];
    }
    carry += sh[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double avg = v / (double)N;
    const double diff = fabs(s.avg - avg);
    RunState o;
    o.k_active = carry;
    o.iters = s.iters + 1;
    o.done = diff > thresh ? 0 : 1;
    o.pad = 0;
    o.avg = avg;
    o.diff = diff;
    st[r] = o;
    done_out[r] = o.done;
  }
}

// rows of the starting codebooks: obs[idx[r][j]] (restarts) or guess[j]
__global__ __launch_bounds__(kThreads) void init_kernel(const float* __restrict__ obs, int64_t ldo, int64_t N, int D,
                                                        const int64_t* __restrict__ idx,
                                                        const float* __restrict__ guess, int64_t ldg, int64_t k,
                                                        RunState* __restrict__ st, float* __restrict__ cb) {
  const int r = blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e == 0) {
    RunState o;
    o.k_active = (int32_t)k;
    o.iters = 0;
    o.done = 0;
    o.pad = 0;
    o.avg = INFINITY;
    o.diff = INFINITY;
    st[r] = o;
  }
  if (e >= k * D) return;
  const int64_t j = e / D;
  const int d = (int)(e % D);
  float v = 0.f;
  if (idx != nullptr) {
    const int64_t row = idx[(int64_t)r * k + j];
    if (row >= 0 && row < N) v = obs[row * ldo + d];
  } else {
    v = guess[j * ldg + d];
  }
  cb[(int64_t)r * k * D + e] = v;
}

__global__ __launch_bounds__(kThreads) void select_kernel(const RunState* __restrict__ st, int R, int64_t k, int D,
                                                          const float* __restrict__ cb, float* __restrict__ out,
                                                          int64_t ldcb, double* __restrict__ distortion,
                                                          int32_t* __restrict__ info) {
  __shared__ int win;
  if (threadIdx.x == 0) {
    int w = 0;
    double best = INFINITY;
    for (int r = 0; r < R; ++r) {
      if (st[r].avg < best) { best = st[r].avg; w = r; }
    }
    win = w;
    *distortion = st[w].avg;
    info[0] = st[w].k_active;
    info[1] = w;
    info[2] = st[w].iters;
    info[3] = st[w].done;
  }
  __syncthreads();
  const int w = win;
  const int64_t ne = (int64_t)st[w].k_active * D;
  for (int64_t e = threadIdx.x; e < ne; e += kThreads) out[(e / D) * ldcb + e % D] = cb[(int64_t)w * k * D + e];
}

// st, partials, cnt == nullptr: a plain vq (no run state, no block partials, no member counts)
static int launch_assign(const float* obs, int64_t ldo, int64_t N, int D, const float* cb, int64_t ldc,
                         int64_t cb_stride, int64_t k, int R, const RunState* st, int32_t* code, float* dist,
                         double* partials, int64_t p_stride, int32_t* cnt, int64_t cnt_stride, hipStream_t s) {
  const int lanes = lanes_for(N);
  const dim3 grid((unsigned)assign_blocks(N), (unsigned)R);
#define MGP_KM_ASSIGN(LV)                                                                                       \
  hipLaunchKernelGGL((assign_kernel<DPV, LV>), grid, dim3(kThreads), 0, s, obs, ldo, N, D, cb, ldc, cb_stride, k, \
                     st, code, dist, N, partials, p_stride, cnt, cnt_stride)
  return dispatch_dmax(D, [&](auto dm) {
    constexpr int DPV = decltype(dm)::value;
    if (lanes == 1) MGP_KM_ASSIGN(1);
    else if (lanes == 4) MGP_KM_ASSIGN(4);
    else MGP_KM_ASSIGN(16);
    return launch_status();
  });
#undef MGP_KM_ASSIGN
}

static int launch_segsum(const float* obs, int64_t ldo, int64_t N, int D, const RunState* st, int64_t k, int R,
                         const int32_t* sorted, const int32_t* counts, const int32_t* segoff, float* out,
                         int64_t ldout, int64_t out_stride, hipStream_t s) {
  const dim3 grid((unsigned)((k + kThreads / 64 - 1) / (kThreads / 64)), (unsigned)R);
  return dispatch_dmax(D, [&](auto dm) {
    hipLaunchKernelGGL((segsum_kernel<decltype(dm)::value>), grid, dim3(kThreads), 0, s, obs, ldo, N, D, st, k,
                       sorted, N, counts, segoff, k, out, ldout, out_stride);
    return launch_status();
  });
}

// the update half of an iteration: cnt (zeroed, then counted) -> counts, segoff, sorted -> means
static int launch_update(const float* obs, int64_t ldo, int64_t N, int D, const RunState* st, int64_t k, int R,
                         const int32_t* code, char* ws, const Layout& L, int32_t* counts, float* out, int64_t ldout,
                         int64_t out_stride, hipStream_t s) {
  int32_t* cnt = (int32_t*)(ws + L.cnt);
  int32_t* segoff = (int32_t*)(ws + L.segoff);
  int32_t* sorted = (int32_t*)(ws + L.sorted);
  hipLaunchKernelGGL(scan_kernel, dim3((unsigned)R), dim3(1024), 0, s, st, cnt, L.G * k, L.G, k, counts, segoff, k);
  int rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)L.G, (unsigned)R), dim3(kChunk), 0, s, st, code, N, N, k, cnt,
                     L.G * k, segoff, k, sorted);
  rc = launch_status();
  if (rc) return rc;
  return launch_segsum(obs, ldo, N, D, st, k, R, sorted, counts, segoff, out, ldout, out_stride, s);
}

static bool in_limits(int64_t N, int64_t k, int D, int R) {
  return D <= kMaxD && N <= kMaxN && k <= N && R <= kMaxR;
}

}  // namespace kmeans
}  // namespace mgp

using namespace mgp;
using kmeans::Layout;
using kmeans::RunState;

extern "C" int mgp_vq(const float* obs, int64_t ldo, const float* code_book, int64_t ldc, int64_t N, int64_t k,
                      int32_t D, int32_t* code, float* dist, mgp_stream_t stream) {
  if (!obs) return -1;
  if (!code_book) return -3;
  if (N < 0) return -5;
  if (k < 1) return -6;
  if (D < 1) return -7;
  if (!code) return -8;
  if (!dist) return -9;
  if (D > kmeans::kMaxD || N > kmeans::kMaxN || k > kmeans::kMaxN) return MGP_ERR_UNSUPPORTED;
  if (ldo < D) return -2;
  if (ldc < D) return -4;
  if (N == 0) return MGP_OK;
  return kmeans::launch_assign(obs, ldo, N, D, code_book, ldc, 0, k, 1, nullptr, code, dist, nullptr, 0, nullptr, 0,
                               (hipStream_t)stream);
}

extern "C" size_t mgp_kmeans_workspace_bytes(int64_t N, int64_t k, int32_t D, int32_t R) {
  if (N < 1 || k < 1 || D < 1 || R < 1 || !kmeans::in_limits(N, k, D, R)) return 0;
  return kmeans::layout(N, k, D, R).total;
}

extern "C" int mgp_kmeans_init(const float* obs, int64_t ldo, int64_t N, int32_t D, const int64_t* idx,
                               const float* guess, int64_t ldg, int64_t k, int32_t R, void* workspace,
                               size_t workspace_bytes, mgp_stream_t stream) {
  if (!obs) return -1;
  if (N < 1) return -3;
  if (D < 1) return -4;
  if (!idx && !guess) return -5;
  if (idx && guess) return -6;
  if (k < 1) return -8;
  if (R < 1 || (guess && R != 1)) return -9;
  if (!kmeans::in_limits(N, k, D, R)) return MGP_ERR_UNSUPPORTED;
  if (ldo < D) return -2;
  if (guess && ldg < D) return -7;
  const Layout L = kmeans::layout(N, k, D, R);
  if (!workspace || workspace_bytes < L.total) return MGP_ERR_WORKSPACE;
  if (!aligned16(workspace)) return MGP_ERR_ALIGN;
  char* ws = (char*)workspace;
  const int64_t nb = (k * D + kmeans::kThreads - 1) / kmeans::kThreads;
  if (nb > 0x7fffffff) return MGP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(kmeans::init_kernel, dim3((unsigned)nb, (unsigned)R), dim3(kmeans::kThreads), 0,
                     (hipStream_t)stream, obs, ldo, N, D, idx, guess, ldg, k, (RunState*)(ws + L.state),
                     (float*)(ws + L.cb));
  return launch_status();
}

extern "C" int mgp_kmeans_iterate(const float* obs, int64_t ldo, int64_t N, int32_t D, int64_t k, int32_t R,
                                  int32_t B, double thresh, void* workspace, size_t workspace_bytes, int32_t* done,
                                  mgp_stream_t stream) {
  if (!obs) return -1;
  if (N < 1) return -3;
  if (D < 1) return -4;
  if (k < 1) return -5;
  if (R < 1) return -6;
  if (B < 1) return -7;
  if (thresh != thresh) return -8;
  if (!done) return -11;
  if (!kmeans::in_limits(N, k, D, R)) return MGP_ERR_UNSUPPORTED;
  if (ldo < D) return -2;
  const Layout L = kmeans::layout(N, k, D, R);
  if (!workspace || workspace_bytes < L.total) return MGP_ERR_WORKSPACE;
  if (!aligned16(workspace)) return MGP_ERR_ALIGN;
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  RunState* st = (RunState*)(ws + L.state);
  float* cb = (float*)(ws + L.cb);
  float* cbnew = (float*)(ws + L.cbnew);
  int32_t* counts = (int32_t*)(ws + L.counts);
  int32_t* code = (int32_t*)(ws + L.code);
  double* partials = (double*)(ws + L.partials);
  for (int b = 0; b < B; ++b) {
    int rc = hip_status(hipMemsetAsync(ws + L.cnt, 0, (size_t)R * L.G * k * 4, s));
    if (rc) return rc;
    rc = kmeans::launch_assign(obs, ldo, N, D, cb, D, k * D, k, R, st, code, (float*)(ws + L.dist), partials, L.NB,
                               (int32_t*)(ws + L.cnt), L.G * k, s);
    if (rc) return rc;
    rc = kmeans::launch_update(obs, ldo, N, D, st, k, R, code, ws, L, counts, cbnew, D, k * D, s);
    if (rc) return rc;
    hipLaunchKernelGGL(kmeans::finish_kernel, dim3((unsigned)R), dim3(1024), 0, s, st, partials, L.NB, L.NB, N, D, k,
                       cbnew, cb, counts, thresh, done);
    rc = launch_status();
    if (rc) return rc;
  }
  return MGP_OK;
}

extern "C" int mgp_kmeans_select(int64_t N, int64_t k, int32_t D, int32_t R, const void* workspace,
                                 size_t workspace_bytes, float* code_book, int64_t ldcb, double* distortion,
                                 int32_t* info, mgp_stream_t stream) {
  if (N < 1) return -1;
  if (k < 1) return -2;
  if (D < 1) return -3;
  if (R < 1) return -4;
  if (!code_book) return -7;
  if (!distortion) return -9;
  if (!info) return -10;
  if (!kmeans::in_limits(N, k, D, R)) return MGP_ERR_UNSUPPORTED;
  if (ldcb < D) return -8;
  const Layout L = kmeans::layout(N, k, D, R);
  if (!workspace || workspace_bytes < L.total) return MGP_ERR_WORKSPACE;
  if (!aligned16(workspace)) return MGP_ERR_ALIGN;
  const char* ws = (const char*)workspace;
  hipLaunchKernelGGL(kmeans::select_kernel, dim3(1), dim3(kmeans::kThreads), 0, (hipStream_t)stream,
                     (const RunState*)(ws + L.state), R, k, D, (const float*)(ws + L.cb), code_book, ldcb,
                     distortion, info);
  return launch_status();
}

extern "C" int mgp_kmeans_update(const float* obs, int64_t ldo, int64_t N, int32_t D, const int32_t* code, int64_t k,
                                 float* means, int64_t ldm, int32_t* counts, void* workspace,
                                 size_t workspace_bytes, mgp_stream_t stream) {
  if (!obs) return -1;
  if (N < 1) return -3;
  if (D < 1) return -4;
  if (!code) return -5;
  if (k < 1) return -6;
  if (!means) return -7;
  if (!counts) return -9;
  if (!kmeans::in_limits(N, k, D, 1)) return MGP_ERR_UNSUPPORTED;
  if (ldo < D) return -2;
  if (ldm < D) return -8;
  const Layout L = kmeans::layout(N, k, D, 1);
  if (!workspace || workspace_bytes < L.total) return MGP_ERR_WORKSPACE;
  if (!aligned16(workspace)) return MGP_ERR_ALIGN;
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int rc = hip_status(hipMemsetAsync(ws + L.cnt, 0, (size_t)L.G * k * 4, s));
  if (rc) return rc;
  hipLaunchKernelGGL(kmeans::hist_kernel, dim3((unsigned)((N + kmeans::kThreads - 1) / kmeans::kThreads)),
                     dim3(kmeans::kThreads), 0, s, code, N, k, (int32_t*)(ws + L.cnt));
  rc = launch_status();
  if (rc) return rc;
  return kmeans::launch_update(obs, ldo, N, D, nullptr, k, 1, code, ws, L, counts, means, ldm, 0, s);
}
