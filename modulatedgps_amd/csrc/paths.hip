// Pathwise posterior function samples of a whitened SVGP layer (Matheron's rule with a
// random-Fourier-feature prior; Wilson et al. 2020, "Efficiently sampling functions from
// Gaussian process posteriors").  The reference has no counterpart; DESIGN "Pathwise
// samples" is the specification.  A sample of expert k is the function
//     f(x) = Phi(x) w + A(x)^T r,    A(x) = L^-1 k(Z, x),
//     phi_j(x) = sqrt(2 var / R) cos(2 pi (Omega_j . x + phase_j)),
// with the whitened residual r = v - L^-1 Phi(Z) w formed once at setup.  Evaluating C
// frozen samples at N points is one GEMM over the stacked k-space [R features; M inducing]:
//     out[c][n] = sum_{j < R} W[j][c] cos(2 pi (Omega_j . x_n + phase_j))
//               + sum_{m < M} W[R + m][c] A[m][n]
// (the prior rows of W carry the sqrt(2 var / R) scale; Omega and phase are in turns).
// The cosine rows are generated into LDS from X and Omega chunk by chunk -- the [R][N]
// feature matrix never exists in HBM -- and the A rows are K4's f32 output, read as they are.
//
// gfx950 mapping (the tile of fullcov.hip): 256 threads = 4 waves as 2 x 2, wave tile
// 64 x 64 = 2 x 2 accumulators of v_mfma_f32_32x32x2_f32 (exact f32 products, f32
// accumulation), workgroup tile 128 sample columns c x 128 points n, both operands k-major
// in 16-row chunks, global / generated -> registers -> LDS, double buffered, one barrier
// per chunk.  The k order is fixed (features 0 .. R-1 padded to a chunk, then m = 0 .. M-1)
// and a point's column is computed from that point alone, so out[c][n] does not depend on N
// or on the point's position in the call: a shard returns the bits of the unsharded call.
// No atomics; every global access is guarded (any N, M, R, C).
#include "mgp_common.hpp"

namespace mgp {

constexpr int kPtBT = 128;   // tile edge (sample columns and points)
constexpr int kPtBK = 16;    // k rows per chunk
constexpr int kPtNT = 256;   // threads
constexpr int kPtMaxD = 32;
constexpr int kPtV4 = kPtBK * kPtBT / 4 / kPtNT;   // float4 per thread, operand and chunk
constexpr int kPtChunk = kPtBK * 2 * kPtBT;        // floats of one chunk (W rows and feature / A rows)

// cos(2 pi t).  |Omega . x| reaches hundreds of radians, so the argument is reduced first:
// t - rint(t) is exact in f32 and lies in [-1/2, 1/2], the best-conditioned part of the
// hardware cosine (v_cos_f32 takes turns, domain [-256, 256]).
__device__ __forceinline__ float cos_turns(float t) {
  const float f = t - rintf(t);
#ifdef MGP_PATH_COSF
  return cosf(6.283185307179586f * f);
#else
  return __builtin_amdgcn_cosf(f);
#endif
}

// grid: workgroup t -> sample tile t % cT, point tile t / cT (neighbours share A's tile).
__global__ __launch_bounds__(kPtNT) void path_eval_kernel(const float* __restrict__ X, int64_t ldx, int64_t N, int D,
                                                          const float* __restrict__ Omega, int64_t ldo,
                                                          const float* __restrict__ phase, int64_t R,
                                                          const float* __restrict__ A, int64_t lda, int64_t M,
                                                          const float* __restrict__ W, int64_t ldw, int64_t C,
                                                          int64_t cT, float* __restrict__ out, int64_t ldout) {
  __shared__ __attribute__((aligned(16))) float lds[2 * kPtChunk];
  __shared__ __attribute__((aligned(16))) float sX[kPtMaxD * kPtBT];   // the tile's points, [d][n]
  const int64_t c0 = (int64_t)(blockIdx.x % cT) * kPtBT, n0 = (int64_t)(blockIdx.x / cT) * kPtBT;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = w >> 1, wc = w & 1;
  const int h = lane >> 5, l32 = lane & 31;

  for (int idx = threadIdx.x; idx < kPtBT * D; idx += kPtNT) {
    const int p = idx / D, d = idx % D;
    sX[d * kPtBT + p] = n0 + p < N ? X[(n0 + p) * ldx + d] : 0.f;
  }
  __syncthreads();

  const int nR = (int)((R + kPtBK - 1) / kPtBK);   // feature chunks (the last one zero padded)
  const int nchunks = nR + (int)((M + kPtBK - 1) / kPtBK);
  const float* WA = W + R * ldw;                   // the rows of W that meet A

  // chunk ch of both operands: rp = W rows, rq = cosine rows (ch < nR) or A rows
  auto produce = [&](int ch, floatx4 (&rp)[kPtV4], floatx4 (&rq)[kPtV4]) {
#pragma unroll
    for (int q = 0; q < kPtV4; ++q) {
      const int idx = threadIdx.x + kPtNT * q;
      const int r = idx / (kPtBT / 4), c = (idx % (kPtBT / 4)) * 4;
      if (ch < nR) {
        const int64_t j = (int64_t)ch * kPtBK + r;
        rp[q] = load4_guarded(W, ldw, j, c0 + c, R, C);
        floatx4 t = {0.f, 0.f, 0.f, 0.f};
        if (j < R) {
          const float* om = Omega + j * ldo;
          const float ph = phase[j];
          t = floatx4{ph, ph, ph, ph};
          for (int d = 0; d < D; ++d) {
            const float o = om[d];
            const floatx4 x = *reinterpret_cast<const floatx4*>(sX + d * kPtBT + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = fmaf(o, x[e], t[e]);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) t[e] = cos_turns(t[e]);
        }
        rq[q] = t;
      } else {
        const int64_t m = (int64_t)(ch - nR) * kPtBK + r;
        rp[q] = load4_guarded(WA, ldw, m, c0 + c, M, C);
        rq[q] = load4_guarded(A, lda, m, n0 + c, M, N);
      }
    }
  };
  auto store_chunk = [&](float* __restrict__ sP, const floatx4 (&rp)[kPtV4], const floatx4 (&rq)[kPtV4]) {
    float* sQ = sP + kPtBK * kPtBT;
#pragma unroll
    for (int q = 0; q < kPtV4; ++q) {
      const int idx = threadIdx.x + kPtNT * q;
      *reinterpret_cast<floatx4*>(sP + idx * 4) = rp[q];
      *reinterpret_cast<floatx4*>(sQ + idx * 4) = rq[q];
    }
  };

  floatx16 acc[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[r][c][e] = 0.f;
  floatx4 rp[kPtV4], rq[kPtV4];
  produce(0, rp, rq);
  store_chunk(lds, rp, rq);
  __syncthreads();
#pragma nounroll
  for (int ch = 0; ch < nchunks; ++ch) {
    const float* sP = lds + (ch & 1) * kPtChunk;
    const float* sQ = sP + kPtBK * kPtBT;
    const bool more = ch + 1 < nchunks;
    if (more) produce(ch + 1, rp, rq);
    float fa[kPtBK / 2][2], fb[kPtBK / 2][2];
#pragma unroll
    for (int ks = 0; ks < kPtBK / 2; ++ks) {
      const int kl = 2 * ks + h;
#pragma unroll
      for (int r = 0; r < 2; ++r) fa[ks][r] = sP[kl * kPtBT + wr * 64 + 32 * r + l32];
#pragma unroll
      for (int c = 0; c < 2; ++c) fb[ks][c] = sQ[kl * kPtBT + wc * 64 + 32 * c + l32];
    }
#pragma unroll
    for (int ks = 0; ks < kPtBK / 2; ++ks)
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][c] = mfma32x32x2(fa[ks][r], fb[ks][c], acc[r][c]);
    if (more) store_chunk(lds + ((ch + 1) & 1) * kPtChunk, rp, rq);
    __syncthreads();
  }

#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int64_t col = n0 + wc * 64 + 32 * c + l32;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int64_t row = c0 + wr * 64 + 32 * r + acc_row(e, lane);
        if (row < C && col < N) out[row * ldout + col] = acc[r][c][e];
      }
    }
}

}  // namespace mgp

using namespace mgp;

extern "C" int mgp_path_eval(const float* X, int64_t ldx, int64_t N, int32_t D, const float* Omega, int64_t ldo,
                             const float* phase, int64_t R, const float* A, int64_t lda, int64_t M, const float* W,
                             int64_t ldw, int32_t C, float* out, int64_t ldout, mgp_stream_t stream) {
  if (!X) return -1;
  if (D < 1) return -4;
  if (D > kPtMaxD) return MGP_ERR_UNSUPPORTED;
  if (ldx < D) return -2;
  if (!Omega) return -5;
  if (ldo < D) return -6;
  if (!phase) return -7;
  if (R < 1) return -8;
  if (M < 0) return -11;
  if (M > 0 && !A) return -9;
  if (M > 0 && lda < N) return -10;
  if (!W) return -12;
  if (C < 1) return -14;
  if (ldw < C) return -13;
  if (!out) return -15;
  if (ldout < N) return -16;
  if (ldw % 4 || !aligned16(W)) return MGP_ERR_ALIGN;
  if (M > 0 && (lda % 4 || !aligned16(A))) return MGP_ERR_ALIGN;
  if (N <= 0) return MGP_OK;
  if (R > 0x7fffffffLL - kPtBK || M > 0x7fffffffLL - kPtBK || R + M > 0x7fffffffLL - 2 * kPtBK)
    return MGP_ERR_UNSUPPORTED;
  const int64_t nT = (N + kPtBT - 1) / kPtBT, cT = ((int64_t)C + kPtBT - 1) / kPtBT;
  if (nT > 0x7fffffffLL / cT) return MGP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(path_eval_kernel, dim3((unsigned)(nT * cT)), dim3(kPtNT), 0, (hipStream_t)stream, X, ldx, N,
                     (int)D, Omega, ldo, phase, R, A, lda, M, W, ldw, (int64_t)C, cT, out, ldout);
  return launch_status();
}
