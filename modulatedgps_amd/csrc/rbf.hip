// K1 / K2: RBF (SquaredExponential) covariance blocks Kuf = K(Z, X) and
// Kuu = K(Z, Z) + jitter I.
//
// Reference: MixtureGPs/models.py:135 (covariances.Kuu) and :139
// (self.kernel.K(Z, Xnew)); GPflow 2.7 SquaredExponential.K_r2(r2) =
// var * exp(-0.5 r2), r2 = square_distance(X / l, X2 / l).
//
// The float32 tile kernel (kuf_image.hpp's "rbf_kernel") and the backward's rows, fold and
// finish are stationary.hpp's templates, instantiated here for FamSE; this file holds the
// family, K1 (the image kernel), the batched backward and the entries.
//
// Roofline: HBM-write bound.  Algorithmic bytes = 4 * (N*D + M*D + M*N); per
// output element the kernel does D subtracts + D FMAs + 1 exp2, far below the
// f32 VALU ridge.
//
// Numerics: direct-difference form sum_d (z_d - x_d)^2 * c_d^2 (exact symmetric,
// never negative) instead of GPflow's |a|^2 + |b|^2 - 2ab expansion; the
// exp(-0.5 r2) is evaluated as exp2(-r2') with c_d = sqrt(0.5 log2 e) / l_d.
// Both operands are taken relative to the first row of Z before they are scaled
// (z_d - Z[0]_d, x_d - Z[0]_d, subtracted where the coordinates are loaded), so the
// rounding of a scaled coordinate grows with the data's spread about that point, not
// with its distance from the origin: K(Z + c, X + c) = K(Z, X), bit for bit whenever
// the shifted coordinates and their differences are exact in float32.
#include "kuf_image.hpp"
#include "mgp_common.hpp"
#include "stationary.hpp"

namespace mgp {

#ifndef MGP_RBF_PACKED
#define MGP_RBF_PACKED 1
#endif
typedef float floatx2v __attribute__((ext_vector_type(2)));

// SquaredExponential as a family of stationary.hpp.  Tile: c_d = sqrt(0.5 log2 e) / l_d and
// k / var = exp2(-acc).  Backward: for K = var exp(-1/2 sum_d (z_d - x_d)^2 / l_d^2) and
// w_mn = gK_mn k_mn the sums are
//   S0_m = sum_n w_mn,  T1_md = sum_n w_mn (x_nd - z_md),  T2_md = sum_n w_mn (x_nd - z_md)^2
//   g_var = sum w / var,  g_z_md = T1_md / l_d^2,  g_l_d = sum_m T2_md / l_d^3.
struct FamSE {
  static constexpr bool kStageScaled = true;
  static constexpr double kGz = 1.0, kGl = 1.0;
  static constexpr bool kS0OverVar = true;
  __device__ float tile_coef(float l) const { return 0.8493218002880191f / l; }  // sqrt(0.5 * log2(e))
  __device__ float unit(float acc) const { return exp2f(-acc); }
  __device__ float bwd_coef(float l) const {  // -1 / (2 l^2)
    const float c = 1.f / l;
    return -0.5f * c * c;
  }
  template <int DMAX>
  __device__ void bwd_point(const float (&hc2)[DMAX], float var, const float (&x)[DMAX], const float (&z)[DMAX],
                            float g, float (&acc)[1 + 2 * DMAX]) const {
    if constexpr (MGP_RBF_PACKED && DMAX % 2 == 0) {
      // coordinate pairs on packed f32 VALU ops (v_pk_add / v_pk_mul / v_pk_fma_f32):
      // half the instructions of the per-coordinate terms
      floatx2v dx[DMAX / 2], qv = {0.f, 0.f};
#pragma unroll
      for (int p = 0; p < DMAX / 2; ++p) {
        dx[p] = floatx2v{x[2 * p], x[2 * p + 1]} - floatx2v{z[2 * p], z[2 * p + 1]};
        qv = floatx2v{hc2[2 * p], hc2[2 * p + 1]} * dx[p] * dx[p] + qv;
      }
      const float wv = g * (var * __expf(qv[0] + qv[1]));
      acc[0] += wv;
      const floatx2v w2 = {wv, wv};
#pragma unroll
      for (int p = 0; p < DMAX / 2; ++p) {
        const floatx2v t = w2 * dx[p];
        floatx2v a1 = {acc[1 + 2 * p], acc[2 + 2 * p]};
        floatx2v a2 = {acc[1 + DMAX + 2 * p], acc[2 + DMAX + 2 * p]};
        a1 += t;
        a2 = t * dx[p] + a2;
        acc[1 + 2 * p] = a1[0];
        acc[2 + 2 * p] = a1[1];
        acc[1 + DMAX + 2 * p] = a2[0];
        acc[2 + DMAX + 2 * p] = a2[1];
      }
    } else {
      float dx[DMAX], q = 0.f;
#pragma unroll
      for (int d = 0; d < DMAX; ++d) {
        dx[d] = x[d] - z[d];
        q = fmaf(hc2[d] * dx[d], dx[d], q);
      }
      const float wv = g * (var * __expf(q));
      acc[0] += wv;
#pragma unroll
      for (int d = 0; d < DMAX; ++d) {
        const float t = wv * dx[d];
        acc[1 + d] += t;
        acc[1 + DMAX + d] = fmaf(t, dx[d], acc[1 + DMAX + d]);
      }
    }
  }
};

// K1 writing Kuf's split-bf16 / split-f16 image (frag_image.hpp layout) instead of f32
// Kuf: one block of kuf_image.hpp per 256-thread workgroup (the body, its layout and
// numerics are documented there; the K3 step launches run the same blocks as their
// Kuf side job, mgp_kuu_potrf_trtri_kuf).
constexpr int kRbfThreads = 256;
template <int DMAX, bool F16 = false>
__global__ __launch_bounds__(kRbfThreads) void rbf_kuf_x6_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ Z, int64_t ldz, int64_t N,
    int64_t M, int D, const float* __restrict__ variance, const float* __restrict__ ls, int n_ls, int nmk,
    bf16x8* __restrict__ Kfr, float* __restrict__ bound, int row_blocks) {
  __shared__ float lds[kuf_block_lds_floats<DMAX>()];
  const KufImageArgs a = {X, ldx, Z, ldz, N, M, D, variance, ls, n_ls, nmk, row_blocks, Kfr, F16 ? bound : nullptr,
                          bound + kKufCentreFloats};
  kuf_image_block<DMAX, F16>(a, blockIdx.x, threadIdx.x, true, lds);
}

// The layers of mgp_rbf_backward_batch: per layer the Kuf cotangent's chunks
// (blockIdx.y < nch, over X) and the Kuu cotangent's (blockIdx.y == nch, X = Z, all
// M points in one chunk), each into its own part slab; blockIdx.z = layer.
constexpr int kRbfMaxBatch = 8;
struct RbfBwdLayers {
  const float* Z[kRbfMaxBatch]; const float* var[kRbfMaxBatch]; const float* ls[kRbfMaxBatch];
  const float* gKuf[kRbfMaxBatch]; const float* gKuu[kRbfMaxBatch];
  float* gZ[kRbfMaxBatch]; double* g_var[kRbfMaxBatch]; double* g_ls[kRbfMaxBatch];
};
template <int DMAX, bool VEC>
__global__ __launch_bounds__(256) void rbf_bwd_rows_batch_kernel(const float* __restrict__ X, int64_t ldx,
                                                                 int64_t N, int64_t ldz, int64_t M, int D, int n_ls,
                                                                 RbfBwdLayers lay, int64_t ldgf, int64_t ldgu,
                                                                 int64_t nchunk, int nch, int64_t slab,
                                                                 double* __restrict__ ws) {
  constexpr int NS = 1 + 2 * DMAX;
  const int b = blockIdx.z, y = blockIdx.y;
  double* part = ws + (int64_t)b * slab + (int64_t)y * M * NS;
  if (y < nch) {
    const int64_t nb = (int64_t)y * nchunk, ne = (nb + nchunk < N) ? nb + nchunk : N;
    stat_bwd_rows_body<FamSE, DMAX, VEC>(FamSE{}, X, ldx, lay.Z[b], ldz, nb, ne, M, D, lay.var[b], lay.ls[b], n_ls,
                                         lay.gKuf[b], ldgf, part);
  } else {
    stat_bwd_rows_body<FamSE, DMAX, VEC>(FamSE{}, lay.Z[b], ldz, lay.Z[b], ldz, 0, M, M, D, lay.var[b], lay.ls[b],
                                         n_ls, lay.gKuu[b], ldgu, part);
  }
}

// layer blockIdx.x: the Kuf contribution (folded slab 0; accumulate as given), then
// the Kuu one (slab nch, symmetric) added to it -- the two finishes of the per-call path
template <int DMAX>
__global__ __launch_bounds__(256) void rbf_bwd_finish_batch_kernel(const double* __restrict__ ws, int64_t slab,
                                                                   int nch, int64_t M, int D, int n_ls,
                                                                   RbfBwdLayers lay, int accumulate, int64_t ldgz) {
  constexpr int NS = 1 + 2 * DMAX;
  __shared__ double scratch[16];
  const int b = blockIdx.x;
  const double* part = ws + (int64_t)b * slab;
  stat_bwd_finish_body<FamSE, DMAX>(part, M, D, lay.var[b], lay.ls[b], n_ls, 1.f, accumulate & 1, lay.gZ[b], ldgz,
                                    lay.g_var[b], lay.g_ls[b], scratch, accumulate != 0);
  __syncthreads();
  stat_bwd_finish_body<FamSE, DMAX>(part + (int64_t)nch * M * NS, M, D, lay.var[b], lay.ls[b], n_ls, 2.f, 1,
                                    lay.gZ[b], ldgz, lay.g_var[b], lay.g_ls[b], scratch, 1);
}

}  // namespace mgp

using namespace mgp;

extern "C" int mgp_rbf_kuf(const float* X, int64_t ldx, const float* Z, int64_t ldz, int64_t N,
                           int64_t M, int32_t D, const float* variance, const float* lengthscales,
                           int32_t n_ls, float* Kuf, int64_t ldk, mgp_stream_t stream) {
  if (!X) return -1;
  if (ldx < D) return -2;
  if (!Z) return -3;
  if (ldz < D) return -4;
  if (N < 0) return -5;
  if (M < 0) return -6;
  if (D < 1) return -7;
  if (D > 32) return MGP_ERR_UNSUPPORTED;
  if (!variance) return -8;
  if (!lengthscales) return -9;
  if (n_ls != 1 && n_ls != D) return -10;
  if (!Kuf) return -11;
  if (ldk < N) return -12;
  if (ldk % 4 || !aligned16(Kuf)) return MGP_ERR_ALIGN;
  return stat_tile_launch(FamSE{}, X, ldx, Z, ldz, N, M, D, variance, lengthscales, n_ls, 0.f, Kuf, ldk,
                          (hipStream_t)stream);
}

extern "C" int mgp_rbf_kuu(const float* Z, int64_t ldz, int64_t M, int32_t D, const float* variance,
                           const float* lengthscales, int32_t n_ls, float jitter, float* Kuu,
                           int64_t ldk, mgp_stream_t stream) {
  if (!Z) return -1;
  if (ldz < D) return -2;
  if (M < 0) return -3;
  if (D < 1) return -4;
  if (D > 32) return MGP_ERR_UNSUPPORTED;
  if (!variance) return -5;
  if (!lengthscales) return -6;
  if (n_ls != 1 && n_ls != D) return -7;
  if (!Kuu) return -9;
  if (ldk < M) return -10;
  if (ldk % 4 || !aligned16(Kuu)) return MGP_ERR_ALIGN;
  return stat_tile_launch(FamSE{}, Z, ldz, Z, ldz, M, M, D, variance, lengthscales, n_ls, jitter, Kuu, ldk,
                          (hipStream_t)stream);
}

static int rbf_kuf_image(const float* X, int64_t ldx, const float* Z, int64_t ldz, int64_t N, int64_t M, int32_t D,
                         const float* variance, const float* lengthscales, int32_t n_ls, void* Kfr,
                         size_t kfr_bytes, mgp_stream_t stream, bool f16) {
  if (!X) return -1;
  if (ldx < D) return -2;
  if (!Z) return -3;
  if (ldz < D) return -4;
  if (N < 0) return -5;
  if (M < 0) return -6;
  if (D < 1) return -7;
  if (D > 32) return MGP_ERR_UNSUPPORTED;
  if (!variance) return -8;
  if (!lengthscales) return -9;
  if (n_ls != 1 && n_ls != D) return -10;
  if (!Kfr) return -11;
  if (N == 0 || M == 0) return MGP_OK;
  if (kfr_bytes < mgp_x6_cols_bytes(M, N)) return -12;
  if (!aligned16(Kfr)) return MGP_ERR_ALIGN;
  const int nmk = kuf_nmk(M);
  const int row_blocks = kuf_row_blocks(M);
  const dim3 grid((unsigned)kuf_blocks(M, N)), block(kRbfThreads);
  hipStream_t s = (hipStream_t)stream;
  float* bound = trailer(Kfr, cols_planes(M, N));  // image trailer (frag_image.hpp)
  return dispatch_dmax(D, [&](auto dm) {
    constexpr int DM = decltype(dm)::value;
    if (f16)
      hipLaunchKernelGGL((rbf_kuf_x6_kernel<DM, true>), grid, block, 0, s, X, ldx, Z, ldz, N, M, D, variance,
                         lengthscales, n_ls, nmk, (bf16x8*)Kfr, bound, row_blocks);
    else
      hipLaunchKernelGGL((rbf_kuf_x6_kernel<DM, false>), grid, block, 0, s, X, ldx, Z, ldz, N, M, D, variance,
                         lengthscales, n_ls, nmk, (bf16x8*)Kfr, bound, row_blocks);
    return launch_status();
  });
}

extern "C" int mgp_rbf_kuf_x6(const float* X, int64_t ldx, const float* Z, int64_t ldz, int64_t N, int64_t M,
                              int32_t D, const float* variance, const float* lengthscales, int32_t n_ls,
                              void* Kfr, size_t kfr_bytes, mgp_stream_t stream) {
  return rbf_kuf_image(X, ldx, Z, ldz, N, M, D, variance, lengthscales, n_ls, Kfr, kfr_bytes, stream, false);
}

extern "C" int mgp_rbf_kuf_f16(const float* X, int64_t ldx, const float* Z, int64_t ldz, int64_t N, int64_t M,
                               int32_t D, const float* variance, const float* lengthscales, int32_t n_ls,
                               void* Kfr, size_t kfr_bytes, mgp_stream_t stream) {
  return rbf_kuf_image(X, ldx, Z, ldz, N, M, D, variance, lengthscales, n_ls, Kfr, kfr_bytes, stream, true);
}

extern "C" size_t mgp_rbf_backward_workspace_bytes(int64_t N, int64_t M, int32_t D) {
  const int64_t nch = stat_bwd_chunks(N);
  return (size_t)((nch > 0 ? nch : 1) * (M > 0 ? M : 1) * (1 + 2 * dmax_of(D))) * sizeof(double);
}

extern "C" int mgp_rbf_backward(const float* X, int64_t ldx, const float* Z, int64_t ldz, int64_t N, int64_t M,
                                int32_t D, const float* variance, const float* lengthscales, int32_t n_ls,
                                const float* gK, int64_t ldg, int32_t symmetric, int32_t accumulate, float* gZ,
                                int64_t ldgz, double* g_var, double* g_ls, void* workspace,
                                size_t workspace_bytes, mgp_stream_t stream) {
  if (!X) return -1;
  if (ldx < D) return -2;
  if (!Z) return -3;
  if (ldz < D) return -4;
  if (N < 0) return -5;
  if (M < 0) return -6;
  if (D < 1) return -7;
  if (D > 32) return MGP_ERR_UNSUPPORTED;
  if (!variance) return -8;
  if (!lengthscales) return -9;
  if (n_ls != 1 && n_ls != D) return -10;
  if (!gK) return -11;
  if (ldg < N) return -12;
  if (!gZ) return -15;
  if (ldgz < D) return -16;
  if (!g_var) return -17;
  if (!g_ls) return -18;
  if (M == 0) return MGP_OK;
  if (!workspace || workspace_bytes < mgp_rbf_backward_workspace_bytes(N, M, D)) return MGP_ERR_WORKSPACE;
  return stat_bwd_launch(FamSE{}, X, ldx, Z, ldz, N, M, D, variance, lengthscales, n_ls, gK, ldg, symmetric, accumulate,
                         gZ, ldgz, g_var, g_ls, (double*)workspace, (hipStream_t)stream);
}

static int64_t rbf_bwd_batch_nch(int64_t N) {
  const int64_t n = stat_bwd_chunks(N);
  return n > 0 ? n : 1;
}

extern "C" size_t mgp_rbf_backward_batch_workspace_bytes(int64_t N, int64_t M, int32_t D) {
  return (size_t)((rbf_bwd_batch_nch(N) + 1) * (M > 0 ? M : 1) * (1 + 2 * dmax_of(D))) * sizeof(double);
}

extern "C" int mgp_rbf_backward_batch(int32_t batch, const float* X, int64_t ldx, int64_t N,
                                      const float* const* Z, int64_t ldz, int64_t M, int32_t D,
                                      const float* const* variance, const float* const* lengthscales, int32_t n_ls,
                                      const float* const* gKuf, int64_t ldgf, const float* const* gKuu, int64_t ldgu,
                                      int32_t accumulate, float* const* gZ, int64_t ldgz, double* const* g_var,
                                      double* const* g_ls, void* workspace, size_t workspace_bytes,
                                      mgp_stream_t stream) {
  if (batch < 1 || batch > kRbfMaxBatch) return -1;
  if (!X) return -2;
  if (ldx < D) return -3;
  if (N < 0) return -4;
  if (!Z) return -5;
  if (ldz < D) return -6;
  if (M < 0) return -7;
  if (D < 1) return -8;
  if (D > 32) return MGP_ERR_UNSUPPORTED;
  if (!variance) return -9;
  if (!lengthscales) return -10;
  if (n_ls != 1 && n_ls != D) return -11;
  if (!gKuf) return -12;
  if (ldgf < N) return -13;
  if (!gKuu) return -14;
  if (ldgu < M) return -15;
  if (!gZ) return -16;
  if (ldgz < D) return -17;
  if (!g_var) return -18;
  if (!g_ls) return -19;
  if (accumulate < 0 || accumulate > 2) return -20;
  RbfBwdLayers lay = {};
  for (int b = 0; b < batch; ++b) {
    if (!Z[b]) return -5;
    if (!variance[b]) return -9;
    if (!lengthscales[b]) return -10;
    if (!gKuf[b]) return -12;
    if (!gKuu[b]) return -14;
    if (!gZ[b]) return -16;
    if (!g_var[b]) return -18;
    if (!g_ls[b]) return -19;
    lay.Z[b] = Z[b], lay.var[b] = variance[b], lay.ls[b] = lengthscales[b], lay.gKuf[b] = gKuf[b];
    lay.gKuu[b] = gKuu[b], lay.gZ[b] = gZ[b], lay.g_var[b] = g_var[b], lay.g_ls[b] = g_ls[b];
  }
  if (M == 0) return MGP_OK;
  const size_t per = mgp_rbf_backward_batch_workspace_bytes(N, M, D);
  if (!workspace || workspace_bytes < (size_t)batch * per) return MGP_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t chunk = kStatChunk, slab = (int64_t)(per / sizeof(double));
  const int nch = (int)rbf_bwd_batch_nch(N);
  double* ws = (double*)workspace;
  bool zvec = ldz % 4 == 0;
  for (int b = 0; b < batch; ++b) zvec = zvec && aligned16(Z[b]);
  const dim3 grid((unsigned)((M + 4 * kStatRows - 1) / (4 * kStatRows)), (unsigned)(nch + 1), (unsigned)batch);
  // the point loads' form only (dwordx4 or dword): the same values either way
  return dispatch_dmax(D, [&](auto dm) {
    constexpr int DM = decltype(dm)::value, NS = 1 + 2 * DM;
    constexpr bool kVec = DM >= 4;  // below 4 the second launch is the first's instance
    if (kVec && ldx % 4 == 0 && ldx >= DM && aligned16(X) && ldz >= DM && zvec)
      hipLaunchKernelGGL((rbf_bwd_rows_batch_kernel<DM, kVec>), grid, dim3(256), 0, s, X, ldx, N, ldz, M, D, n_ls, lay,
                         ldgf, ldgu, chunk, nch, slab, ws);
    else
      hipLaunchKernelGGL((rbf_bwd_rows_batch_kernel<DM, false>), grid, dim3(256), 0, s, X, ldx, N, ldz, M, D, n_ls,
                         lay, ldgf, ldgu, chunk, nch, slab, ws);
    if (nch > 1)
      hipLaunchKernelGGL(stat_bwd_fold_kernel, dim3((unsigned)((M * NS + 255) / 256), (unsigned)batch), dim3(256), 0,
                         s, ws, nch, M * NS, slab);
    hipLaunchKernelGGL(rbf_bwd_finish_batch_kernel<DM>, dim3((unsigned)batch), dim3(256), 0, s, ws, slab, nch, M, D,
                       n_ls, lay, accumulate, ldgz);
    return launch_status();
  });
}
