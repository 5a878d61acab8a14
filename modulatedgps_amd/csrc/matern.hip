// Matern-3/2 and Matern-5/2 covariance blocks beside rbf.hip's SquaredExponential ones:
// Kuf = K(Z, X) and Kuu = K(Z, Z) + jitter I in float32, K1 for Matern (the Kuf fragment
// image of frag_image.hpp, written directly), Kuu in float64 for K3's float64-input path,
// and the reverse mode of K(Z, X).  The float32 tile kernel and the backward's rows, fold
// and finish are stationary.hpp's templates, instantiated here for FamMatern; this file
// holds the family, K1, the float64 Kuu and the entries.
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
#include "stationary.hpp"

namespace mgp {

constexpr int kMatThreads = 256;

// Matern-3/2 and 5/2 as one family of stationary.hpp; nu2 is run-time data, so one
// instruction stream serves both.  Tile and backward: c_d = sqrt(nu2) / l_d on the raw
// difference.  Backward: with g(s) = dk / d(r^2) / var (nu2 = 3: -(3/2) e^-s; nu2 = 5:
// -(5/6)(1 + s) e^-s; nothing divides by s) and w = gK var g the sums are
//   S0_m = sum_n gK k / var,  T1_md = sum_n w (z_d - x_d),  T2_md = sum_n w (z_d - x_d)^2:
//   g_var = sum_m S0,  gZ_md = 2 T1_md / l_d^2,  g_ls_d = -2 sum_m T2_md / l_d^3.
struct FamMatern {
  int nu2;
  static constexpr bool kStageScaled = false;
  static constexpr double kGz = 2.0, kGl = -2.0;
  static constexpr bool kS0OverVar = false;
  __device__ float q3() const { return nu2 == 5 ? (1.f / 3.f) : 0.f; }
  __device__ float tile_coef(float l) const { return (nu2 == 5 ? 2.2360679774997897f : 1.7320508075688772f) / l; }
  __device__ float bwd_coef(float l) const { return tile_coef(l); }
  // k / var from s^2 (v_sqrt_f32, v_exp_f32)
  __device__ float unit(float s2) const {
    const float s = __builtin_amdgcn_sqrtf(s2);
    return fmaf(s, fmaf(s, q3(), 1.f), 1.f) * __expf(-s);
  }
  template <int DMAX>
  __device__ void bwd_point(const float (&c)[DMAX], float var, const float (&x)[DMAX], const float (&z)[DMAX],
                            float g, float (&acc)[1 + 2 * DMAX]) const {
    const float ga = nu2 == 5 ? -(5.f / 6.f) : -1.5f, gb = nu2 == 5 ? 1.f : 0.f;
    float dx[DMAX], s2 = 0.f;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      dx[d] = z[d] - x[d];
      const float tt = dx[d] * c[d];
      s2 = fmaf(tt, tt, s2);
    }
    const float s = __builtin_amdgcn_sqrtf(s2), e = __expf(-s);
    acc[0] = fmaf(g, fmaf(s, fmaf(s, q3(), 1.f), 1.f) * e, acc[0]);
    const float wv = g * (var * (ga * fmaf(s, gb, 1.f) * e));
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      const float tw = wv * dx[d];
      acc[1 + d] += tw;
      acc[1 + DMAX + d] = fmaf(tw, dx[d], acc[1 + DMAX + d]);
    }
  }
};

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
  const FamMatern fam{nu2};
  __shared__ float zs[kKufRows][DMAX];
  __shared__ float cs[DMAX];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, h = lane >> 5, c32 = lane & 31;
  const int64_t bid = blockIdx.x;
  const int64_t rb = bid % row_blocks, cg = bid / row_blocks;
  const int64_t nb = cg * 4 + w;
  const int64_t n = 32 * nb + c32;
  const int64_t m0 = kKufRows * rb;
  if (t < DMAX) cs[t] = (t < D) ? fam.tile_coef(ls[n_ls == 1 ? 0 : t]) : 0.f;
  for (int i = t; i < kKufRows * DMAX; i += kMatThreads) {
    const int r = i / DMAX, d = i % DMAX;
    const int64_t m = m0 + r;
    zs[r][d] = (m < M && d < D) ? Z[m * ldz + d] : 0.f;
  }
  float x[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) x[d] = (n < N && d < D) ? X[n * ldx + d] : 0.f;
  const float var = variance[0];
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
      v[j] = fam.unit(acc) * mult;
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
  return stat_tile_launch(FamMatern{nu2}, X, ldx, Z, ldz, N, M, D, variance, lengthscales, n_ls, 0.f, Kuf, ldk,
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
  return stat_tile_launch(FamMatern{nu2}, Z, ldz, Z, ldz, M, M, D, variance, lengthscales, n_ls, jitter, Kuu, ldk,
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
  return dispatch_dmax(D, [&](auto dm) {
    constexpr int DM = decltype(dm)::value;
    if (kfr_format == 1)
      hipLaunchKernelGGL((matern_kuf_image_kernel<DM, true>), grid, block, 0, s, X, ldx, Z, ldz, N, M, D, variance,
                         lengthscales, n_ls, nu2, nmk, row_blocks, (bf16x8*)Kfr, tr);
    else
      hipLaunchKernelGGL((matern_kuf_image_kernel<DM, false>), grid, block, 0, s, X, ldx, Z, ldz, N, M, D, variance,
                         lengthscales, n_ls, nu2, nmk, row_blocks, (bf16x8*)Kfr, tr);
    return launch_status();
  });
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
  const int64_t nch = stat_bwd_chunks(N);
  return (size_t)((nch > 0 ? nch : 1) * M * (1 + 2 * dmax_of(D))) * sizeof(double);
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
  return stat_bwd_launch(FamMatern{nu2}, X, ldx, Z, ldz, N, M, D, variance, lengthscales, n_ls, gK, ldg, symmetric,
                         accumulate, gZ, ldgz, g_var, g_ls, (double*)workspace, (hipStream_t)stream);
}
