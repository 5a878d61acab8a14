// Matern-3/2 and Matern-5/2 covariance blocks beside rbf.hip's SquaredExponential ones:
// Kuf = K(Z, X) and Kuu = K(Z, Z) + jitter I in float32, K1 for Matern (the Kuf fragment
// image of frag_image.hpp, written directly), Kuu in float64 for K3's float64-input path,
// and the reverse mode of K(Z, X).
//
// Reference: GPflow 2.7 Matern32 / Matern52 (IsotropicStationary.K_r) as the original
// ModulatedGPs used them in place of SquaredExponential at MixtureGPs/models.py:135, 139.
//   s = sqrt(nu2) sqrt(sum_d ((z_d - x_d) / l_d)^2),  nu2 = 2 nu in {3, 5}
//   nu2 = 3: k = var (1 + s) exp(-s)          nu2 = 5: k = var (1 + s + s^2 / 3) exp(-s)
//
// Numerics: the direct form only.  Each z_d - x_d is formed on the raw float32 coordinates
// as the first operation, scaled by c_d = sqrt(nu2) / l_d, squared and summed (fmaf chain in
// dimension order); no expanded |z|^2 + |x|^2 - 2 z.x and no reference point.  Every value
// is a function of coordinate differences alone, so K(Z + c, X + c) = K(Z, X) bit for bit
// whenever the shifted coordinates are exact, K(Z, Z) is bitwise symmetric ((a - b)^2 =
// (b - a)^2), and the float32 error is a few ulp of s^2 plus v_sqrt_f32 / v_exp_f32 (1 ulp
// each): |err| <= ~1e-6 var.  Both families share one instruction stream: with q3 = 1/3 or
// 0 the polynomial is 1 + s (1 + q3 s).
//
// Roofline: every kernel here does 3 D VALU operations per element (subtract, scale, fma)
// plus ~10 for sqrt / exp / polynomial, against 4 B (f32), 6 B (image) written per element.
#include "kuf_image.hpp"
#include "mgp_common.hpp"

namespace mgp {

constexpr int kMatThreads = 256;
constexpr int kMatCols = 4;                        // columns per thread (f32 kernel)
constexpr int kMatTileN = kMatThreads * kMatCols;  // 1024 columns per workgroup
constexpr int kMatTileM = 64;                      // rows per workgroup

__host__ __device__ inline float matern_sqrt_nu(int nu2) { return nu2 == 5 ? 2.2360679774997897f : 1.7320508075688772f; }
__host__ __device__ inline float matern_q3(int nu2) { return nu2 == 5 ? (1.f / 3.f) : 0.f; }

// k / var from s^2 (v_sqrt_f32, v_exp_f32)
__device__ __forceinline__ float matern_unit(float s2, float q3) {
  const float s = __builtin_amdgcn_sqrtf(s2);
  return fmaf(s, fmaf(s, q3, 1.f), 1.f) * __expf(-s);
}

// ------------------------------------------------------------------ float32 Kuf / Kuu
// Layout as rbf.hip's rbf_kernel: out [M][ldo], a thread owns 4 consecutive columns (one
// float4 store per row), the tile's raw Z rows staged in LDS and read as broadcasts.
template <int DMAX>
__global__ __launch_bounds__(kMatThreads) void matern_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ Z, int64_t ldz, int64_t N, int64_t M, int D,
    const float* __restrict__ variance, const float* __restrict__ ls, int n_ls, int nu2, float jitter,
    float* __restrict__ out, int64_t ldo) {
  __shared__ float zs[kMatTileM][DMAX];
  __shared__ float cs[DMAX];
  const int t = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * kMatTileN + (int64_t)t * kMatCols;
  const int64_t m0 = (int64_t)blockIdx.y * kMatTileM;
  if (t < DMAX) cs[t] = (t < D) ? matern_sqrt_nu(nu2) / ls[n_ls == 1 ? 0 : t] : 0.f;
  for (int i = t; i < kMatTileM * DMAX; i += kMatThreads) {
    const int r = i / DMAX, d = i % DMAX;
    const int64_t m = m0 + r;
    zs[r][d] = (m < M && d < D) ? Z[m * ldz + d] : 0.f;
  }
  float xs[kMatCols][DMAX];
#pragma unroll
  for (int j = 0; j < kMatCols; ++j) {
    const int64_t n = n0 + j;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) xs[j][d] = (n < N && d < D) ? X[n * ldx + d] : 0.f;
  }
  const float var = variance[0], q3 = matern_q3(nu2);
  __syncthreads();
  float c[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) c[d] = cs[d];

  const int rows = (int)((M - m0) < kMatTileM ? (M - m0) : kMatTileM);
  for (int r = 0; r < rows; ++r) {
    const int64_t m = m0 + r;
    float v[kMatCols];
#pragma unroll
    for (int j = 0; j < kMatCols; ++j) {
      float acc = 0.f;
#pragma unroll
      for (int d = 0; d < DMAX; ++d) {
        const float tt = (zs[r][d] - xs[j][d]) * c[d];
        acc = fmaf(tt, tt, acc);
      }
      v[j] = var * matern_unit(acc, q3);
      if (jitter != 0.f && m == n0 + j) v[j] += jitter;
    }
    float* o = out + m * ldo + n0;
    if (n0 + kMatCols <= N) {
      *reinterpret_cast<floatx4*>(o) = floatx4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int j = 0; j < kMatCols; ++j)
        if (n0 + j < N) o[j] = v[j];
    }
  }
}

// ------------------------------------------------------------------ K1 for Matern
// The Kuf fragment image (frag_image.hpp: Afr[nb][mk][plane][lane][8]) without an f32 Kuf.
// Geometry of kuf_image.hpp's blocks: 4 waves x 32 columns x 128 rows, block `bid` is row
// block bid % row_blocks of column group bid / row_blocks.  Lane (c32 = lane & 31,
// h = lane >> 5) owns column 32 nb + c32; its 8 elements of k-step mk are rows
// 16 mk + kperm(h, j), computed here on the VALU in that order (the two lane halves read two
// LDS addresses per row: broadcasts), split and stored as 16-B fragments.  Rows >= M and
// columns >= N are zeros.  Trailer: float 0 = the variance (Kuf <= variance: the split-f16
// scale bound), floats [32, 64) = zeros (no reference point).
template <int DMAX, bool F16>
__global__ __launch_bounds__(kMatThreads) void matern_kuf_image_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ Z, int64_t ldz, int64_t N, int64_t M, int D,
    const float* __restrict__ variance, const float* __restrict__ ls, int n_ls, int nu2, int nmk, int row_blocks,
    bf16x8* __restrict__ Kfr, float* __restrict__ tr) {
  __shared__ float zs[kKufRows][DMAX];
  __shared__ float cs[DMAX];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, h = lane >> 5, c32 = lane & 31;
  const int64_t bid = blockIdx.x;
  const int64_t rb = bid % row_blocks, cg = bid / row_blocks;
  const int64_t nb = cg * 4 + w;
  const int64_t n = 32 * nb + c32;
  const int64_t m0 = kKufRows * rb;
  if (t < DMAX) cs[t] = (t < D) ? matern_sqrt_nu(nu2) / ls[n_ls == 1 ? 0 : t] : 0.f;
  for (int i = t; i < kKufRows * DMAX; i += kMatThreads) {
    const int r = i / DMAX, d = i % DMAX;
    const int64_t m = m0 + r;
    zs[r][d] = (m < M && d < D) ? Z[m * ldz + d] : 0.f;
  }
  float x[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) x[d] = (n < N && d < D) ? X[n * ldx + d] : 0.f;
  const float var = variance[0], q3 = matern_q3(nu2);
  if (bid == 0) {
    if (t == 0) tr[0] = var;
    if (t >= kKufCentreFloats && t < 2 * kKufCentreFloats) tr[t] = 0.f;
  }
  __syncthreads();
  float c[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) c[d] = cs[d];
  // split-f16: the image scale (a power of two) folds into the variance multiplier
  const float mult = F16 ? var * ldexpf(1.f, img_exp(var)) : var;
  const bool col_ok = n < N;
#pragma unroll 1
  for (int ks = 0; ks < kKufRows / 16; ++ks) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = 16 * ks + kperm(h, j);
      float acc = 0.f;
#pragma unroll
      for (int d = 0; d < DMAX; ++d) {
        const float tt = (zs[r][d] - x[d]) * c[d];
        acc = fmaf(tt, tt, acc);
      }
      v[j] = matern_unit(acc, q3) * mult;
      if (!col_ok || m0 + r >= M) v[j] = 0.f;
      // the split must see v as the rounded f32 product (kuf_image.hpp: without this the
      // multiply is contracted into the hi / lo conversions and the planes disagree)
      asm volatile("" : "+v"(v[j]));
    }
    store_fragment<F16, 0>(Kfr + ((nb * nmk + (kKufRows / 16) * rb + ks) * 3) * 64 + lane, v);
  }
}

// ------------------------------------------------------------------ float64 Kuu
// Kuu = K(Z, Z) + jitter I as doubles [M][ld] (differences of the float32 inputs, scaling,
// sqrt and exp all in double) for K3's float64-input path.  One thread per element;
// bitwise symmetric.
__global__ __launch_bounds__(256) void matern_kuu_f64_kernel(const float* __restrict__ Z, int64_t ldz, int64_t M, int D,
                                                             const float* __restrict__ variance,
                                                             const float* __restrict__ ls, int n_ls, int nu2,
                                                             double jitter, double* __restrict__ out, int64_t ld) {
  const int64_t j = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const int64_t i = (int64_t)blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= M || j >= M) return;
  const double rt = nu2 == 5 ? 2.23606797749978969641 : 1.73205080756887729353;
  double acc = 0.0;
  for (int d = 0; d < D; ++d) {
    const double tt = ((double)Z[i * ldz + d] - (double)Z[j * ldz + d]) * (rt / (double)ls[n_ls == 1 ? 0 : d]);
    acc = fma(tt, tt, acc);
  }
  const double s = sqrt(acc);
  const double p = nu2 == 5 ? 1.0 + s + s * s * (1.0 / 3.0) : 1.0 + s;
  out[i * ld + j] = (double)variance[0] * p * exp(-s) + (i == j ? jitter : 0.0);
}

// ------------------------------------------------------------------ backward
// Reverse mode of K(Z, X) for a cotangent gK [M][N].  With g(s) = dk / d(r^2) / var
// (nu2 = 3: -(3/2) e^-s; nu2 = 5: -(5/6)(1 + s) e^-s; nothing divides by s), w = gK var g and
//   S0_m = sum_n gK k / var,  T1_md = sum_n w (z_d - x_d),  T2_md = sum_n w (z_d - x_d)^2:
//   g_var = sum_m S0,  gZ_md = 2 T1_md / l_d^2,  g_ls_d = -2 sum_m T2_md / l_d^3.
// Coincident points contribute exact zeros to T1 and T2.  For Kuu (X = Z, symmetric gK) z
// enters both arguments: gZ doubles.  Kernel 1 as rbf.hip's: 4 waves x 2 rows of Z per
// block, lanes stride over an n-chunk (VEC: ldx % 4 == 0, ldx >= DMAX and X 16-byte aligned, a
// point's coordinates come in DMAX / 4 dwordx4 loads); each lane accumulates its <= 64 points in float32,
// the lane reduction and everything after it is float64 in a fixed order (kernel 2 folds
// the chunks, kernel 3 writes the gradients; no atomics: two calls give the same bits).
constexpr int kMatRows = 2;       // rows of Z per wave
constexpr int64_t kMatChunk = 4096;

template <int DMAX, bool VEC>
__global__ __launch_bounds__(256) void matern_bwd_rows_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ Z, int64_t ldz, int64_t N, int64_t M, int D,
    const float* __restrict__ variance, const float* __restrict__ ls, int n_ls, int nu2,
    const float* __restrict__ gK, int64_t ldg, double* __restrict__ part_all) {
  constexpr int NS = 1 + 2 * DMAX, R = kMatRows;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * 4 * R + R * w;
  const int64_t nb = (int64_t)blockIdx.y * kMatChunk;
  const int64_t ne = (nb + kMatChunk < N) ? nb + kMatChunk : N;
  double* part = part_all + (int64_t)blockIdx.y * M * NS;
  float c[DMAX], z[R][DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) c[d] = (d < D) ? matern_sqrt_nu(nu2) / ls[n_ls == 1 ? 0 : d] : 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int d = 0; d < DMAX; ++d) z[r][d] = (m0 + r < M && d < D) ? Z[(m0 + r) * ldz + d] : 0.f;
  const float var = variance[0], q3 = matern_q3(nu2);
  const float ga = nu2 == 5 ? -(5.f / 6.f) : -1.5f, gb = nu2 == 5 ? 1.f : 0.f;
  float acc[R][NS];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[r][j] = 0.f;
  auto point = [&](int64_t n) {
    float x[DMAX], g[R];
    if constexpr (VEC) {
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
    for (int r = 0; r < R; ++r) {
      float dx[DMAX], s2 = 0.f;
#pragma unroll
      for (int d = 0; d < DMAX; ++d) {
        dx[d] = z[r][d] - x[d];
        const float tt = dx[d] * c[d];
        s2 = fmaf(tt, tt, s2);
      }
      const float s = __builtin_amdgcn_sqrtf(s2), e = __expf(-s);
      acc[r][0] = fmaf(g[r], fmaf(s, fmaf(s, q3, 1.f), 1.f) * e, acc[r][0]);
      const float wv = g[r] * (var * (ga * fmaf(s, gb, 1.f) * e));
#pragma unroll
      for (int d = 0; d < DMAX; ++d) {
        const float tw = wv * dx[d];
        acc[r][1 + d] += tw;
        acc[r][1 + DMAX + d] = fmaf(tw, dx[d], acc[r][1 + DMAX + d]);
      }
    }
  };
  int64_t n = nb + lane;
  for (; n + 192 < ne; n += 256) {   // four points' loads in flight
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

// part[0][idx] = sum over the chunks of part[ch][idx], one thread per idx, fixed order
__global__ __launch_bounds__(256) void matern_bwd_fold_kernel(double* __restrict__ part, int nchunks, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  double v = part[idx];
  for (int ch = 1; ch < nchunks; ++ch) v += part[(int64_t)ch * total + idx];
  part[idx] = v;
}

template <int DMAX>
__global__ __launch_bounds__(256) void matern_bwd_finish_kernel(const double* __restrict__ part, int64_t M, int D,
                                                                const float* __restrict__ ls, int n_ls, float zfactor,
                                                                int accumulate, float* __restrict__ gZ, int64_t ldgz,
                                                                double* __restrict__ g_var, double* __restrict__ g_ls) {
  constexpr int NS = 1 + 2 * DMAX;
  __shared__ double scratch[16];
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
      const double gz = (double)zfactor * 2.0 * il[d] * il[d] * part[m * NS + 1 + d];
      gZ[m * ldgz + d] = (float)(accumulate ? (double)gZ[m * ldgz + d] + gz : gz);
      gl[d] += -2.0 * il[d] * il[d] * il[d] * part[m * NS + 1 + DMAX + d];
    }
  }
  const double gv = block_sum<double>(s0tot, scratch);
  if (threadIdx.x == 0) *g_var = accumulate ? *g_var + gv : gv;
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

static int matern_dmax(int D) { return D <= 1 ? 1 : D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : 32; }

static int matern_launch(const float* X, int64_t ldx, const float* Z, int64_t ldz, int64_t N, int64_t M, int D,
                         const float* variance, const float* ls, int n_ls, int nu2, float jitter, float* out,
                         int64_t ldo, hipStream_t stream) {
  dim3 grid((unsigned)((N + kMatTileN - 1) / kMatTileN), (unsigned)((M + kMatTileM - 1) / kMatTileM));
  dim3 block(kMatThreads);
#define MGP_MAT_CASE(DM)                                                                                  \
  if (D <= DM) {                                                                                          \
    hipLaunchKernelGGL(matern_kernel<DM>, grid, block, 0, stream, X, ldx, Z, ldz, N, M, D, variance, ls,   \
                       n_ls, nu2, jitter, out, ldo);                                                      \
    return launch_status();                                                                               \
  }
  MGP_MAT_CASE(1)
  MGP_MAT_CASE(2)
  MGP_MAT_CASE(4)
  MGP_MAT_CASE(8)
  MGP_MAT_CASE(16)
  MGP_MAT_CASE(32)
#undef MGP_MAT_CASE
  return MGP_ERR_UNSUPPORTED;
}

}  // namespace mgp

using namespace mgp;

extern "C" int mgp_matern_kuf(const float* X, int64_t ldx, const float* Z, int64_t ldz, int64_t N, int64_t M,
                              int32_t D, const float* variance, const float* lengthscales, int32_t n_ls,
                              int32_t nu2, float* Kuf, int64_t ldk, mgp_stream_t stream) {
  if (!X) return -1;
  if (ldx < D) return -2;
  if (!Z) return -3;
  if (ldz < D) return -4;
  if (D < 1) return -7;
  if (D > 32) return MGP_ERR_UNSUPPORTED;
  if (!variance) return -8;
  if (!lengthscales) return -9;
  if (n_ls != 1 && n_ls != D) return -10;
  if (nu2 != 3 && nu2 != 5) return -11;
  if (!Kuf) return -12;
  if (ldk < N) return -13;
  if (ldk % 4 || !aligned16(Kuf)) return MGP_ERR_ALIGN;
  if (N <= 0 || M <= 0) return MGP_OK;
  return matern_launch(X, ldx, Z, ldz, N, M, D, variance, lengthscales, n_ls, nu2, 0.f, Kuf, ldk,
                       (hipStream_t)stream);
}

extern "C" int mgp_matern_kuu(const float* Z, int64_t ldz, int64_t M, int32_t D, const float* variance,
                              const float* lengthscales, int32_t n_ls, int32_t nu2, float jitter, float* Kuu,
                              int64_t ldk, mgp_stream_t stream) {
  if (!Z) return -1;
  if (ldz < D) return -2;
  if (D < 1) return -4;
  if (D > 32) return MGP_ERR_UNSUPPORTED;
  if (!variance) return -5;
  if (!lengthscales) return -6;
  if (n_ls != 1 && n_ls != D) return -7;
  if (nu2 != 3 && nu2 != 5) return -8;
  if (!(jitter >= 0.f)) return -9;
  if (!Kuu) return -10;
  if (ldk < M) return -11;
  if (ldk % 4 || !aligned16(Kuu)) return MGP_ERR_ALIGN;
  if (M <= 0) return MGP_OK;
  return matern_launch(Z, ldz, Z, ldz, M, M, D, variance, lengthscales, n_ls, nu2, jitter, Kuu, ldk,
                       (hipStream_t)stream);
}

extern "C" int mgp_matern_kuf_image(const float* X, int64_t ldx, const float* Z, int64_t ldz, int64_t N, int64_t M,
                                    int32_t D, const float* variance, const float* lengthscales, int32_t n_ls,
                                    int32_t nu2, void* Kfr, size_t kfr_bytes, int32_t kfr_format,
                                    mgp_stream_t stream) {
  if (!X) return -1;
  if (ldx < D) return -2;
  if (!Z) return -3;
  if (ldz < D) return -4;
  if (D < 1) return -7;
  if (D > 32) return MGP_ERR_UNSUPPORTED;
  if (!variance) return -8;
  if (!lengthscales) return -9;
  if (n_ls != 1 && n_ls != D) return -10;
  if (nu2 != 3 && nu2 != 5) return -11;
  if (!Kfr) return -12;
  if (kfr_format != 0 && kfr_format != 1) return -14;
  if (N <= 0 || M <= 0) return MGP_OK;
  if (kfr_bytes < mgp_x6_cols_bytes(M, N)) return -13;
  if (!aligned16(Kfr)) return MGP_ERR_ALIGN;
  const int nmk = kuf_nmk(M), row_blocks = kuf_row_blocks(M);
  const dim3 grid((unsigned)kuf_blocks(M, N)), block(kMatThreads);
  hipStream_t s = (hipStream_t)stream;
  float* tr = trailer(Kfr, cols_planes(M, N));
#define MGP_MAT_IMG_CASE(DM)                                                                                 \
  if (D <= DM) {                                                                                             \
    if (kfr_format == 1)                                                                                     \
      hipLaunchKernelGGL((matern_kuf_image_kernel<DM, true>), grid, block, 0, s, X, ldx, Z, ldz, N, M, D,     \
                         variance, lengthscales, n_ls, nu2, nmk, row_blocks, (bf16x8*)Kfr, tr);              \
    else                                                                                                     \
      hipLaunchKernelGGL((matern_kuf_image_kernel<DM, false>), grid, block, 0, s, X, ldx, Z, ldz, N, M, D,    \
                         variance, lengthscales, n_ls, nu2, nmk, row_blocks, (bf16x8*)Kfr, tr);              \
    return launch_status();                                                                                  \
  }
  MGP_MAT_IMG_CASE(1)
  MGP_MAT_IMG_CASE(2)
  MGP_MAT_IMG_CASE(4)
  MGP_MAT_IMG_CASE(8)
  MGP_MAT_IMG_CASE(16)
  MGP_MAT_IMG_CASE(32)
#undef MGP_MAT_IMG_CASE
  return MGP_ERR_UNSUPPORTED;
}

// K3's workspace for one matrix, then the float64 Kuu [M][M]
extern "C" size_t mgp_matern_chol_workspace_bytes(int64_t M) {
  if (M <= 0) return 0;
  return mgp_chol_workspace_bytes(M, 1) + (size_t)M * (size_t)M * sizeof(double);
}

extern "C" int mgp_matern_kuu_potrf_trtri(const float* Z, int64_t ldz, int64_t M, int32_t D, const float* variance,
                                          const float* lengthscales, int32_t n_ls, int32_t nu2, float jitter,
                                          float* L, float* LinvT, int64_t ldl, int32_t* info, void* workspace,
                                          size_t workspace_bytes, mgp_stream_t stream) {
  if (!Z) return -1;
  if (ldz < D) return -2;
  if (D < 1) return -4;
  if (D > 32) return MGP_ERR_UNSUPPORTED;
  if (!variance) return -5;
  if (!lengthscales) return -6;
  if (n_ls != 1 && n_ls != D) return -7;
  if (nu2 != 3 && nu2 != 5) return -8;
  if (!(jitter >= 0.f)) return -9;
  if (!LinvT) return -11;
  if (ldl < M) return -12;
  if (!info) return -13;
  if (M <= 0) return MGP_OK;
  if (!workspace || workspace_bytes < mgp_matern_chol_workspace_bytes(M)) return MGP_ERR_WORKSPACE;
  if (ldl % 4 || !aligned16(workspace) || !aligned16(LinvT) || (L && !aligned16(L))) return MGP_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const size_t chol_bytes = mgp_chol_workspace_bytes(M, 1);
  double* Ad = (double*)((char*)workspace + chol_bytes);
  const dim3 grid((unsigned)((M + 15) / 16), (unsigned)((M + 15) / 16));
  hipLaunchKernelGGL(matern_kuu_f64_kernel, grid, dim3(256), 0, s, Z, ldz, M, D, variance, lengthscales, n_ls, nu2,
                     (double)jitter, Ad, M);
  const int st = launch_status();
  if (st) return st;
  return mgp_potrf_trtri_f64_l(Ad, M, 0, M, 1, L, LinvT, ldl, 0, info, workspace, chol_bytes, s);
}

extern "C" size_t mgp_matern_backward_workspace_bytes(int64_t N, int64_t M, int32_t D) {
  if (N < 0 || M <= 0 || D < 1 || D > 32) return 0;
  const int64_t nch = (N + kMatChunk - 1) / kMatChunk;
  return (size_t)((nch > 0 ? nch : 1) * M * (1 + 2 * matern_dmax(D))) * sizeof(double);
}

extern "C" int mgp_matern_backward(const float* X, int64_t ldx, const float* Z, int64_t ldz, int64_t N, int64_t M,
                                   int32_t D, const float* variance, const float* lengthscales, int32_t n_ls,
                                   int32_t nu2, const float* gK, int64_t ldg, int32_t symmetric, int32_t accumulate,
                                   float* gZ, int64_t ldgz, double* g_var, double* g_ls, void* workspace,
                                   size_t workspace_bytes, mgp_stream_t stream) {
  if (!X) return -1;
  if (ldx < D) return -2;
  if (!Z) return -3;
  if (ldz < D) return -4;
  if (D < 1) return -7;
  if (D > 32) return MGP_ERR_UNSUPPORTED;
  if (!variance) return -8;
  if (!lengthscales) return -9;
  if (n_ls != 1 && n_ls != D) return -10;
  if (nu2 != 3 && nu2 != 5) return -11;
  if (!gK) return -12;
  if (ldg < N) return -13;
  if (!gZ) return -16;
  if (ldgz < D) return -17;
  if (!g_var) return -18;
  if (!g_ls) return -19;
  if (N <= 0 || M <= 0) return MGP_OK;
  if (!workspace || workspace_bytes < mgp_matern_backward_workspace_bytes(N, M, D)) return MGP_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int nch = (int)((N + kMatChunk - 1) / kMatChunk);
  double* part = (double*)workspace;
  const float zf = symmetric ? 2.f : 1.f;
  const int acc = accumulate ? 1 : 0;
  const dim3 grid((unsigned)((M + 4 * kMatRows - 1) / (4 * kMatRows)), (unsigned)nch);
#define MGP_MAT_BWD_CASE(DM)                                                                                    \
  if (D <= DM) {                                                                                                \
    /* the point loads' form only (dwordx4 or dword): the same values either way */                             \
    if (DM >= 4 && ldx % 4 == 0 && ldx >= DM && aligned16(X))                                                   \
      hipLaunchKernelGGL((matern_bwd_rows_kernel<DM, (DM >= 4)>), grid, dim3(256), 0, s, X, ldx, Z, ldz, N, M, D, \
                         variance, lengthscales, n_ls, nu2, gK, ldg, part);                                     \
    else                                                                                                        \
      hipLaunchKernelGGL((matern_bwd_rows_kernel<DM, false>), grid, dim3(256), 0, s, X, ldx, Z, ldz, N, M, D,    \
                         variance, lengthscales, n_ls, nu2, gK, ldg, part);                                     \
    if (nch > 1)                                                                                                \
      hipLaunchKernelGGL(matern_bwd_fold_kernel, dim3((unsigned)((M * (1 + 2 * DM) + 255) / 256)), dim3(256), 0, \
                         s, part, nch, M * (1 + 2 * DM));                                                       \
    hipLaunchKernelGGL(matern_bwd_finish_kernel<DM>, dim3(1), dim3(256), 0, s, part, M, D, lengthscales, n_ls,   \
                       zf, acc, gZ, ldgz, g_var, g_ls);                                                         \
    return launch_status();                                                                                     \
  }
  MGP_MAT_BWD_CASE(1)
  MGP_MAT_BWD_CASE(2)
  MGP_MAT_BWD_CASE(4)
  MGP_MAT_BWD_CASE(8)
  MGP_MAT_BWD_CASE(16)
  MGP_MAT_BWD_CASE(32)
#undef MGP_MAT_BWD_CASE
  return MGP_ERR_UNSUPPORTED;
}
