// The structure that every stationary covariance family shares, templated on a family F
// (rbf.hip's FamSE, matern.hip's FamMatern): the float32 Kuf / Kuu tile kernel and the
// reverse mode of K(Z, X) (rows, fold, finish), with their launch sequences.  The two K1
// kernels (rbf.hip's rbf_kuf_x6_kernel: the MFMA expanded form about a reference point of
// kuf_image.hpp; matern.hip's matern_kuf_image_kernel: the VALU direct form) are different
// algorithms, not copies, and stay in their files.
//
// A family is a small struct, passed by value (its members are run-time data, e.g.
// FamMatern's nu2: one instruction stream per family), that says
//   kStageScaled        the tile kernel stages coordinates relative to Z[0] and scaled by
//                       tile_coef (SE), or raw, scaling each difference instead (Matern)
//   tile_coef(l)        a lengthscale's coefficient in the tile kernel
//   unit(acc)           k / var from acc = sum_d (scaled difference)^2
//   bwd_coef(l)         a lengthscale's coefficient in the backward rows
//   bwd_point<DMAX>(c, var, x, z, g, acc)   one (row, point) pair of the backward: adds the
//                       pair's terms to acc = {S0, T1[DMAX], T2[DMAX]}.  The families differ
//                       here on purpose (the sign of dx, what S0 holds, where the scale
//                       enters), so none of it is shared.
//   kGz, kGl, kS0OverVar  the finish: gZ = zfactor kGz T1 / l^2, g_ls = kGl sum_m T2 / l^3,
//                       g_var = sum_m S0 (/ var)
#pragma once
#include "mgp_common.hpp"

namespace mgp {

// ------------------------------------------------------------------ float32 Kuf / Kuu
// out [M][ldo] row-major (N contiguous); each thread owns 4 consecutive columns (one float4
// store per row), a wave writes 1 KiB contiguous per row.  The Z rows of the tile are staged
// once in LDS and read as wave-uniform broadcasts.  HBM-write bound: per element D
// subtracts + D FMAs (+ D multiplies where the coordinates are raw) + unit().
constexpr int kStatThreads = 256;
constexpr int kStatCols = 4;                          // columns per thread
constexpr int kStatTileN = kStatThreads * kStatCols;  // 1024 columns per workgroup
constexpr int kStatTileM = 64;                        // rows per workgroup (X re-read M/64 times)

template <class F, int DMAX>
__global__ __launch_bounds__(kStatThreads) void stat_tile_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ Z, int64_t ldz, int64_t N, int64_t M, int D,
    const float* __restrict__ variance, const float* __restrict__ ls, int n_ls, float jitter,
    float* __restrict__ out, int64_t ldo, F fam) {
  __shared__ float zs[kStatTileM][DMAX];
  __shared__ float cs[DMAX];
  const int t = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * kStatTileN + (int64_t)t * kStatCols;
  const int64_t m0 = (int64_t)blockIdx.y * kStatTileM;

  if (t < DMAX) cs[t] = (t < D) ? fam.tile_coef(ls[n_ls == 1 ? 0 : t]) : 0.f;
  if constexpr (F::kStageScaled) __syncthreads();
  auto staged = [&](const float* __restrict__ P, int64_t ld, int64_t i, int d) {
    if constexpr (F::kStageScaled) return (P[i * ld + d] - Z[d]) * cs[d];
    else return P[i * ld + d];
  };
  for (int i = t; i < kStatTileM * DMAX; i += kStatThreads) {
    const int r = i / DMAX, d = i % DMAX;
    const int64_t m = m0 + r;
    zs[r][d] = (m < M && d < D) ? staged(Z, ldz, m, d) : 0.f;
  }
  float xs[kStatCols][DMAX];
#pragma unroll
  for (int j = 0; j < kStatCols; ++j) {
    const int64_t n = n0 + j;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) xs[j][d] = (n < N && d < D) ? staged(X, ldx, n, d) : 0.f;
  }
  const float var = variance[0];
  __syncthreads();
  float c[DMAX];  // raw coordinates: the scale of each difference
#pragma unroll
  for (int d = 0; d < DMAX; ++d) c[d] = F::kStageScaled ? 1.f : cs[d];

  const int rows = (int)((M - m0) < kStatTileM ? (M - m0) : kStatTileM);
  for (int r = 0; r < rows; ++r) {
    const int64_t m = m0 + r;
    float v[kStatCols];
#pragma unroll
    for (int j = 0; j < kStatCols; ++j) {
      float acc = 0.f;
#pragma unroll
      for (int d = 0; d < DMAX; ++d) {
        float diff = zs[r][d] - xs[j][d];
        if constexpr (!F::kStageScaled) diff *= c[d];
        acc = fmaf(diff, diff, acc);
      }
      v[j] = var * fam.unit(acc);
      if (jitter != 0.f && m == n0 + j) v[j] += jitter;
    }
    float* o = out + m * ldo + n0;
    if (n0 + kStatCols <= N) {
      *reinterpret_cast<floatx4*>(o) = floatx4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int j = 0; j < kStatCols; ++j)
        if (n0 + j < N) o[j] = v[j];
    }
  }
}

template <class F>
int stat_tile_launch(F fam, const float* X, int64_t ldx, const float* Z, int64_t ldz, int64_t N, int64_t M, int D,
                     const float* variance, const float* ls, int n_ls, float jitter, float* out, int64_t ldo,
                     hipStream_t stream) {
  if (N <= 0 || M <= 0) return MGP_OK;
  const dim3 grid((unsigned)((N + kStatTileN - 1) / kStatTileN), (unsigned)((M + kStatTileM - 1) / kStatTileM));
  return dispatch_dmax(D, [&](auto dm) {
    hipLaunchKernelGGL((stat_tile_kernel<F, decltype(dm)::value>), grid, dim3(kStatThreads), 0, stream, X, ldx, Z,
                       ldz, N, M, D, variance, ls, n_ls, jitter, out, ldo, fam);
    return launch_status();
  });
}

// ------------------------------------------------------------------ backward
// Reverse mode of K(Z, X) for a cotangent gK [M][N]: per row m of Z the sums over n
//   S0_m, T1_md, T2_md   (what bwd_point adds; centred terms, no cancellation between large
//                         ones; coincident points contribute exact zeros to T1 and T2)
// and from them g_var, gZ and g_ls (stat_bwd_finish_body).  For Kuu (X = Z, symmetric gK)
// z enters both arguments: gZ doubles (zfactor).
// Kernel 1: 4 waves x 2 rows of Z per block, lanes stride over an n-chunk four points at a
// time; each lane accumulates its <= 64 points in float32, the lane / chunk reduction and
// everything after it is float64 in a fixed order (no atomics: two calls give the same
// bits).  Kernel 2 folds the chunks (one thread per sum), kernel 3 writes the grads.
// VEC (ldx % 4 == 0, ldx >= DMAX, X 16-byte aligned): a point's coordinates come in
// DMAX / 4 dwordx4 loads instead of DMAX dword loads at a 4 ldx-byte lane stride -- the
// strided dword loads cost the address unit 8x the cycles and bounded this kernel.  The
// loads' form only: the same values either way.
constexpr int kStatRows = 2;         // rows of Z per wave
constexpr int64_t kStatChunk = 4096;  // points per chunk (blockIdx.y)

// one workgroup's rows (blockIdx.x) over the points [nb, ne); part: this chunk's [M][NS]
template <class F, int DMAX, bool VEC>
__device__ __forceinline__ void stat_bwd_rows_body(F fam, const float* __restrict__ X, int64_t ldx,
                                                   const float* __restrict__ Z, int64_t ldz, int64_t nb, int64_t ne,
                                                   int64_t M, int D, const float* __restrict__ variance,
                                                   const float* __restrict__ ls, int n_ls,
                                                   const float* __restrict__ gK, int64_t ldg,
                                                   double* __restrict__ part) {
  constexpr int NS = 1 + 2 * DMAX, R = kStatRows;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * 4 * R + R * w;
  float c[DMAX], z[R][DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) c[d] = (d < D) ? fam.bwd_coef(ls[n_ls == 1 ? 0 : d]) : 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int d = 0; d < DMAX; ++d) z[r][d] = (m0 + r < M && d < D) ? Z[(m0 + r) * ldz + d] : 0.f;
  const float var = variance[0];
  float acc[R][NS];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[r][j] = 0.f;
  auto point = [&](int64_t n) {
    float x[DMAX], g[R];
    if constexpr (VEC && DMAX >= 4) {
#pragma unroll
      for (int q4 = 0; q4 < DMAX / 4; ++q4) {
        const floatx4 v = *reinterpret_cast<const floatx4*>(X + n * ldx + 4 * q4);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[4 * q4 + j] = (4 * q4 + j < D) ? v[j] : 0.f;
      }
    } else {
#pragma unroll
      for (int d = 0; d < DMAX; ++d) x[d] = (d < D) ? X[n * ldx + d] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) g[r] = (m0 + r < M) ? gK[(m0 + r) * ldg + n] : 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) fam.template bwd_point<DMAX>(c, var, x, z[r], g[r], acc[r]);
  };
  int64_t n = nb + lane;
  for (; n + 192 < ne; n += 256) {  // four points' loads in flight
    point(n);
    point(n + 64);
    point(n + 128);
    point(n + 192);
  }
  for (; n < ne; n += 64) point(n);
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const double v = wave_sum<double>((double)acc[r][j]);
      if (lane == 0 && m0 + r < M) part[(m0 + r) * NS + j] = v;
    }
}

template <class F, int DMAX, bool VEC>
__global__ __launch_bounds__(256) void stat_bwd_rows_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ Z, int64_t ldz, int64_t N, int64_t M, int D,
    const float* __restrict__ variance, const float* __restrict__ ls, int n_ls, const float* __restrict__ gK,
    int64_t ldg, double* __restrict__ part, F fam) {
  constexpr int NS = 1 + 2 * DMAX;
  const int64_t nb = (int64_t)blockIdx.y * kStatChunk;
  const int64_t ne = (nb + kStatChunk < N) ? nb + kStatChunk : N;
  stat_bwd_rows_body<F, DMAX, VEC>(fam, X, ldx, Z, ldz, nb, ne, M, D, variance, ls, n_ls, gK, ldg,
                                   part + (int64_t)blockIdx.y * M * NS);
}

// part[0][m][j] = sum over the chunks of part[ch][m][j] (in place: each thread
// reads only its own (m, j) of every chunk), one thread per (m, j), fixed order.
// blockIdx.y: the layer of a batched call (part advances by slab doubles).  static: no
// template, and both files include this header.
static __global__ __launch_bounds__(256) void stat_bwd_fold_kernel(double* __restrict__ part, int nchunks,
                                                                   int64_t total, int64_t slab) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  part += blockIdx.y * slab;
  if (idx >= total) return;
  double v = part[idx];
  for (int ch = 1; ch < nchunks; ++ch) v += part[(int64_t)ch * total + idx];
  part[idx] = v;
}

// the grads of one folded part [M][NS]; 256 threads, scratch >= 16 doubles of LDS.
// variance is read only where F::kS0OverVar; acc_var: g_var's own accumulate flag.
template <class F, int DMAX>
__device__ __forceinline__ void stat_bwd_finish_body(const double* __restrict__ part, int64_t M, int D,
                                                     const float* __restrict__ variance,
                                                     const float* __restrict__ ls, int n_ls, float zfactor,
                                                     int accumulate, float* __restrict__ gZ, int64_t ldgz,
                                                     double* __restrict__ g_var, double* __restrict__ g_ls,
                                                     double* scratch, int acc_var) {
  constexpr int NS = 1 + 2 * DMAX;
  double gl[DMAX], il[DMAX], s0tot = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    gl[d] = 0.0;
    il[d] = (d < D) ? 1.0 / (double)ls[n_ls == 1 ? 0 : d] : 0.0;
  }
  for (int64_t m = threadIdx.x; m < M; m += 256) {
    s0tot += part[m * NS];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      if (d >= D) break;
      // kGz, kGl = 1.0 multiply exactly: every family keeps the bits of its own product order
      const double gz = (double)zfactor * F::kGz * il[d] * il[d] * part[m * NS + 1 + d];
      gZ[m * ldgz + d] = (float)(accumulate ? (double)gZ[m * ldgz + d] + gz : gz);
      gl[d] += F::kGl * il[d] * il[d] * il[d] * part[m * NS + 1 + DMAX + d];
    }
  }
  double gv = block_sum<double>(s0tot, scratch);
  if constexpr (F::kS0OverVar) gv /= (double)variance[0];
  if (threadIdx.x == 0) *g_var = acc_var ? *g_var + gv : gv;
  double giso = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    if (d >= D) break;
    __syncthreads();
    const double v = block_sum<double>(gl[d], scratch);
    if (threadIdx.x == 0) {
      if (n_ls == 1) giso += v;
      else g_ls[d] = accumulate ? g_ls[d] + v : v;
    }
  }
  if (threadIdx.x == 0 && n_ls == 1) g_ls[0] = accumulate ? g_ls[0] + giso : giso;
}

template <class F, int DMAX>
__global__ __launch_bounds__(256) void stat_bwd_finish_kernel(const double* __restrict__ part, int64_t M, int D,
                                                              const float* __restrict__ variance,
                                                              const float* __restrict__ ls, int n_ls, float zfactor,
                                                              int accumulate, float* __restrict__ gZ, int64_t ldgz,
                                                              double* __restrict__ g_var, double* __restrict__ g_ls) {
  __shared__ double scratch[16];
  stat_bwd_finish_body<F, DMAX>(part, M, D, variance, ls, n_ls, zfactor, accumulate, gZ, ldgz, g_var, g_ls, scratch,
                                accumulate);
}

inline int stat_bwd_chunks(int64_t N) { return (int)((N + kStatChunk - 1) / kStatChunk); }

// rows over max(chunks, 1) [M][NS] slabs of part (no points: zeros instead), fold, finish
template <class F>
int stat_bwd_launch(F fam, const float* X, int64_t ldx, const float* Z, int64_t ldz, int64_t N, int64_t M, int D,
                    const float* variance, const float* ls, int n_ls, const float* gK, int64_t ldg, int symmetric,
                    int accumulate, float* gZ, int64_t ldgz, double* g_var, double* g_ls, double* part,
                    hipStream_t s) {
  const int nch = stat_bwd_chunks(N);
  const float zf = symmetric ? 2.f : 1.f;
  const dim3 grid((unsigned)((M + 4 * kStatRows - 1) / (4 * kStatRows)), (unsigned)(nch > 0 ? nch : 1));
  return dispatch_dmax(D, [&](auto dm) {
    constexpr int DM = decltype(dm)::value, NS = 1 + 2 * DM;
    constexpr bool kVec = DM >= 4;  // below 4 the second launch is the first's instance
    if (nch == 0)
      (void)hipMemsetAsync(part, 0, (size_t)(M * NS) * sizeof(double), s);
    else if (kVec && ldx % 4 == 0 && ldx >= DM && aligned16(X))
      hipLaunchKernelGGL((stat_bwd_rows_kernel<F, DM, kVec>), grid, dim3(256), 0, s, X, ldx, Z, ldz, N, M, D,
                         variance, ls, n_ls, gK, ldg, part, fam);
    else
      hipLaunchKernelGGL((stat_bwd_rows_kernel<F, DM, false>), grid, dim3(256), 0, s, X, ldx, Z, ldz, N, M, D,
                         variance, ls, n_ls, gK, ldg, part, fam);
    if (nch > 1)
      hipLaunchKernelGGL(stat_bwd_fold_kernel, dim3((unsigned)((M * NS + 255) / 256)), dim3(256), 0, s, part, nch,
                         M * NS, (int64_t)0);
    hipLaunchKernelGGL((stat_bwd_finish_kernel<F, DM>), dim3(1), dim3(256), 0, s, part, M, D, variance, ls, n_ls, zf,
                       accumulate, gZ, ldgz, g_var, g_ls);
    return launch_status();
  });
}

}  // namespace mgp
