// The fragment-image builders (layout: frag_image.hpp): the split-bf16 / split-f16 images of the
// triangular operands (tril(q_sqrt), L^-T) and of column operands, their scale bounds (absmax, the
// batched q_sqrt images with the KL terms, the column-norm bound of the C_k images).
#include <algorithm>

#include "frag_image.hpp"
#include "qsqrt_jobs.hpp"

namespace mgp {

// A-operand image of a batch of triangular matrices: element (k-row m, row m')
// = S_b[m][m'] kept where m >= m' (LOWER: L_k = tril(q_sqrt[k]), K5) or m <= m'
// (upper: LinvT, K4's T[k][i] = L^-T[k][i]).  One wave per fragment block
// (b, mb, mk): grid.x = batch * nmb * nmk / 4.
// TRANS: the source is stored transposed (element (m, m') read at S[m' ld + m]).
// bound != nullptr: split-f16 image, scaled by 2^img_exp(*bound).
template <bool LOWER, bool TRANS = false, bool FULL = false>
__global__ __launch_bounds__(256) void split_tri_kernel(const float* __restrict__ src, int64_t ld,
                                                        int64_t stride, int64_t M, int nmb, int nmk,
                                                        int64_t nfrag, bf16x8* __restrict__ img,
                                                        const float* __restrict__ bound = nullptr) {
  // (a grid of fewer than nfrag / 4 workgroups walks the fragments with a stride)
  for (int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); f < nfrag; f += (int64_t)gridDim.x * 4)
    split_tri_frag<LOWER, TRANS, FULL>(src, ld, stride, M, nmb, nmk, f, threadIdx.x & 63, img, bound);
}

// ------------------------------------------------------------------ tril(q_sqrt) work of two layers
// mgp_qsqrt_images_kl_f16_batch: the split-f16 images of tril(q_sqrt) and the whitened KL
// terms of both SMGP layers in three launches (blockIdx.y / x = the layer) instead of five
// per layer (bound memset, absmax, split, KL partials, KL final): the KL partial sums also
// fold the images' scale bounds (the maxima of the lower triangles they read), the final
// launch writes both KL terms and both bounds, the split launch follows.  Same sums in the
// same order and the same bound as the per-layer launches: bit-identical results.
struct QLayer {
  const float* q_mu;
  const float* q_sqrt;
  bf16x8* Lfr;
  float* bound;     // Lfr's trailer
  double* kl_out;
  double* part;     // [nblk][3] partial sums
  float* bmax;      // [nblk] block maxima
};

// The tril(q_sqrt) work runs on the side stream beside K3's chain: with MGP_QS_GRID > 0 its
// two wide launches (the KL partials and the image split) walk their blocks / fragments in a
// grid-stride loop over at most MGP_QS_GRID workgroups per layer, so that they hold fewer CUs
// while the chain's step launches dispatch (same per-block and per-fragment work: the same bits;
// 256 against the full grids: ELBO step 3.186-3.234 vs 3.229-3.238 ms and c4r 0.696-0.700 vs
// 0.702-0.706 ms on one box, even on another, profiles/r06v_qsqrt_side_grid_ab.log, r06w_*;
// 16 or 64 put the side work on the critical path).
#ifndef MGP_QS_GRID
#define MGP_QS_GRID 256
#endif
constexpr int kQsGrid = MGP_QS_GRID;

__global__ __launch_bounds__(256) void kl_absmax2_kernel(QLayer l0, QLayer l1, int64_t ldq, int64_t ldqs,
                                                         int64_t strideq, int64_t M, int K, int nrb, int nblk) {
  __shared__ double scratch[16];
  __shared__ float smax[4];
  const QLayer& l = blockIdx.y ? l1 : l0;
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {   // (uniform per workgroup)
    const KlPartial r = kl_partials_thread(l.q_mu, ldq, l.q_sqrt, ldqs, strideq, M, K, nrb, blk, threadIdx.x, 256);
    const float m = wave_max_f32(r.amax);
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = m;
    const double a = block_sum<double>((double)r.tr, scratch);   // (its barriers publish smax)
    const double b = block_sum<double>((double)r.ld, scratch);
    const double c = block_sum<double>((double)r.mh, scratch);
    if (threadIdx.x == 0) {
      l.part[3 * blk + 0] = a;
      l.part[3 * blk + 1] = b;
      l.part[3 * blk + 2] = c;
      l.bmax[blk] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    }
    __syncthreads();   // smax / scratch reused by the next block
  }
}

// One 1024-thread block per layer: kl_final_kernel's sums, and the image bound.
__global__ __launch_bounds__(1024) void kl_final2_kernel(QLayer l0, QLayer l1, int nblk, double MK) {
  __shared__ double scratch[16];
  __shared__ float smax[16];
  const QLayer& l = blockIdx.x ? l1 : l0;
  double tr, ld, mh;
  kl_final_thread(l.part, nblk, threadIdx.x, 1024, tr, ld, mh);
  float m = 0.f;
  for (int i = threadIdx.x; i < nblk; i += 1024) m = fmaxf(m, l.bmax[i]);
  m = wave_max_f32(m);
  if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = m;
  tr = block_sum<double>(tr, scratch);   // (its barriers publish smax)
  ld = block_sum<double>(ld, scratch);
  mh = block_sum<double>(mh, scratch);
  if (threadIdx.x == 0) {
    *l.kl_out = 0.5 * (mh - MK - ld + tr);
    float b = 0.f;
    for (int i = 0; i < 16; ++i) b = fmaxf(b, smax[i]);
    *l.bound = b;
  }
}

__global__ __launch_bounds__(256) void split_lower2_kernel(QLayer l0, QLayer l1, int64_t ldqs, int64_t strideq,
                                                           int64_t M, int nmb, int nmk, int64_t nfrag) {
  const QLayer& l = blockIdx.y ? l1 : l0;
  for (int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); f < nfrag; f += (int64_t)gridDim.x * 4)
    split_tri_frag<true>(l.q_sqrt, ldqs, strideq, M, nmb, nmk, f, threadIdx.x & 63, l.Lfr, l.bound);
}

// split_tri_kernel<false> (the split-f16 L^-T images) for two matrices at src and
// src + stride into two images in one launch: blockIdx.y = the matrix (same fragments,
// same arithmetic as two launches: bit-identical).
__global__ __launch_bounds__(256) void split_upper2_kernel(const float* __restrict__ src, int64_t ld, int64_t stride,
                                                           int64_t M, int nmb, int nmk, int64_t nfrag,
                                                           bf16x8* __restrict__ img0, const float* __restrict__ bound0,
                                                           bf16x8* __restrict__ img1,
                                                           const float* __restrict__ bound1) {
  const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= nfrag) return;
  const bool second = blockIdx.y != 0;
  bf16x8* img = second ? img1 : img0;
  const float* bound = second ? bound1 : bound0;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int mk = (int)(f % nmk);
  const int mb = (int)((f / nmk) % nmb);
  const int64_t mc = 32 * (int64_t)mb + r;
  const float* S = src + (second ? stride : 0);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t m = 16 * (int64_t)mk + kperm(h, j);
    v[j] = (m < M && mc < M && m <= mc) ? S[m * ld + mc] : 0.f;
  }
  store_split_f16<true>(img + f * 3 * 64 + lane, v, ldexpf(1.f, img_exp(*bound)));
}

// One wave per fragment block (nb, mk): grid.x = nnb * nmk / 4.
__global__ __launch_bounds__(256) void split_cols_kernel(const float* __restrict__ A, int64_t lda, int64_t M,
                                                         int64_t N, int nmk, int64_t nfrag,
                                                         bf16x8* __restrict__ Afr,
                                                         const float* __restrict__ bound = nullptr) {
  const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= nfrag) return;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int mk = (int)(f % nmk);
  const int64_t n = 32 * (f / nmk) + r;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t m = 16 * (int64_t)mk + kperm(h, j);
    v[j] = (m < M && n < N) ? A[m * lda + n] : 0.f;
  }
  if (bound)
    store_split_f16<true>(Afr + f * 3 * 64 + lane, v, ldexpf(1.f, img_exp(*bound)));
  else
    store_split(Afr + f * 3 * 64 + lane, v);
}

// max |x| over a batch of row-major matrices (rows x cols; TRI 0: all entries,
// 1: column <= row, 2: column >= row) -> *out as float bits through atomicMax
// (non-negative floats order as their bit patterns; *out zeroed beforehand).
// Waves stride over rows; one atomic per workgroup after an LDS reduction (a
// same-address atomic per wave serialises at the L2: 96 us at K M = 8192 rows).
template <int TRI>
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ src, int64_t ld, int64_t stride,
                                                     int64_t rows, int64_t cols, int64_t nrows_total,
                                                     unsigned int* __restrict__ out) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // TRI 0: blockIdx.y strides over column chunks of kAbsChunk (few long rows)
  constexpr int64_t kAbsChunk = 8192;
  float m = 0.f;
  for (int64_t gr = (int64_t)blockIdx.x * 4 + w; gr < nrows_total; gr += (int64_t)gridDim.x * 4) {
    const int64_t b = gr / rows, r = gr % rows;
    const float* row = src + b * stride + r * ld;
    int64_t c0 = TRI == 2 ? r : 0;
    int64_t c1 = TRI == 1 ? (r + 1 < cols ? r + 1 : cols) : cols;
    if (TRI == 0) {
      c0 = (int64_t)blockIdx.y * kAbsChunk;
      c1 = c0 + kAbsChunk < cols ? c0 + kAbsChunk : cols;
    }
    if (TRI != 2 && (ld & 3) == 0 && ((uintptr_t)row & 15) == 0) {  // float4 loads (c0 % 4 == 0), scalar tail
      const int64_t c4 = c0 + ((c1 - c0) & ~(int64_t)3);
#pragma unroll 4
      for (int64_t c = c0 + 4 * lane; c < c4; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(row + c);
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
      }
      for (int64_t c = c4 + lane; c < c1; c += 64) m = fmaxf(m, fabsf(row[c]));
    } else {
      for (int64_t c = c0 + lane; c < c1; c += 64) m = fmaxf(m, fabsf(row[c]));
    }
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 8, 64));
  m = fmaxf(m, __shfl_xor(m, 4, 64));
  m = fmaxf(m, __shfl_xor(m, 2, 64));
  m = fmaxf(m, __shfl_xor(m, 1, 64));
  if (lane == 0) red[w] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(out, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

// Launch shape of absmax_kernel<TRI>: <= 1024 row groups (one atomic per workgroup; 256
// left the reduction of K q_sqrt triangles latency-bound at 34 us for 32 MB, round 4);
// TRI 0 adds column chunks so a few long rows still fill the chip.
template <int TRI>
static void launch_absmax(const float* src, int64_t ld, int64_t stride, int64_t rows, int64_t cols,
                          int64_t nrows_total, float* out, hipStream_t s) {
  const int64_t gx = std::min<int64_t>((nrows_total + 3) / 4, TRI == 0 ? 64 : 1024);
  const int64_t gy = TRI == 0 ? std::min<int64_t>((cols + 8191) / 8192, 64) : 1;
  hipLaunchKernelGGL(absmax_kernel<TRI>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, s, src, ld, stride, rows,
                     cols, nrows_total, (unsigned int*)out);
}

// max over k, j of ||tril(q_sqrt[k])[:, j]||_2 -> *out (float bits, atomicMax; zeroed
// beforehand).  Workgroup = (32 columns, expert k): thread (ty, tx) sums rows
// ty, ty + 8, ... of column 32 blockIdx.x + tx (row-contiguous loads), LDS sums
// the 8 partials, one atomic per workgroup.
__global__ __launch_bounds__(256) void colnorm_max_kernel(const float* __restrict__ q, int64_t ldq, int64_t sq,
                                                          int64_t M, unsigned int* __restrict__ out) {
  __shared__ float part[8][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t j = (int64_t)blockIdx.x * 32 + tx;
  const float* Q = q + (int64_t)blockIdx.y * sq;
  float v = 0.f;
  if (j < M) {
#pragma unroll 8
    for (int64_t i = ty; i < M; i += 8) {
      const float x = i >= j ? Q[i * ldq + j] : 0.f;
      v = fmaf(x, x, v);
    }
  }
  part[ty][tx] = v;
  __syncthreads();
  if (threadIdx.x < 32) {
    float c = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) c += part[r][threadIdx.x];
    c = sqrtf(c);
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) c = fmaxf(c, __shfl_xor(c, off, 32));
    if (threadIdx.x == 0) atomicMax(out, __float_as_uint(c));
  }
}

// The launches of these kernels from other files (declared in frag_image.hpp).
void launch_split_tri(TriImage form, const float* src, int64_t ld, int64_t stride, int64_t M, int nmb, int nmk,
                      int64_t nfrag, bf16x8* img, const float* bound, hipStream_t s) {
  const dim3 grid((unsigned)((nfrag + 3) / 4));
  if (form == TriImage::kUpperTrans)
    hipLaunchKernelGGL((split_tri_kernel<false, true>), grid, dim3(256), 0, s, src, ld, stride, M, nmb, nmk, nfrag,
                       img, bound);
  else if (form == TriImage::kLowerTrans)
    hipLaunchKernelGGL((split_tri_kernel<true, true>), grid, dim3(256), 0, s, src, ld, stride, M, nmb, nmk, nfrag,
                       img, bound);
  else
    hipLaunchKernelGGL((split_tri_kernel<true, false, true>), grid, dim3(256), 0, s, src, ld, stride, M, nmb, nmk,
                       nfrag, img, bound);
}

void launch_absmax_tri(AbsTri tri, const float* src, int64_t ld, int64_t stride, int64_t rows, int64_t cols,
                       int64_t nrows_total, float* out, hipStream_t s) {
  switch (tri) {
    case AbsTri::kAll: return launch_absmax<0>(src, ld, stride, rows, cols, nrows_total, out, s);
    case AbsTri::kLower: return launch_absmax<1>(src, ld, stride, rows, cols, nrows_total, out, s);
    case AbsTri::kUpper: return launch_absmax<2>(src, ld, stride, rows, cols, nrows_total, out, s);
  }
}

}  // namespace mgp

using namespace mgp;

extern "C" size_t mgp_x6_lower_bytes(int64_t M, int32_t K) {
  if (M <= 0 || K <= 0) return 0;
  return lower_planes(M, K) + kTrailer;
}

extern "C" size_t mgp_x6_cols_bytes(int64_t M, int64_t N) {
  if (M <= 0 || N <= 0) return 0;
  return cols_planes(M, N) + kTrailer;
}

extern "C" int mgp_split_lower_x6(const float* q_sqrt, int64_t ldqs, int64_t strideq, int64_t M, int32_t K,
                                  void* Lfr, size_t lfr_bytes, mgp_stream_t stream) {
  if (!q_sqrt) return -1;
  if (ldqs < M) return -2;
  if (K > 1 && strideq < ldqs * M) return -3;
  if (M < 0) return -4;
  if (K < 0) return -5;
  if (!Lfr) return -6;
  if (M == 0 || K == 0) return MGP_OK;
  if (lfr_bytes < mgp_x6_lower_bytes(M, K)) return MGP_ERR_WORKSPACE;
  if (!aligned16(Lfr)) return MGP_ERR_ALIGN;
  const int64_t Mp = x6_mp(M);
  const int nmb = (int)(Mp / 32), nmk = (int)(Mp / 16);
  const int64_t nfrag = (int64_t)K * nmb * nmk;
  hipLaunchKernelGGL(split_tri_kernel<true>, dim3((unsigned)((nfrag + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, q_sqrt, ldqs, strideq, M, nmb, nmk, nfrag, (bf16x8*)Lfr);
  return launch_status();
}

extern "C" int mgp_split_upper_x6(const float* LinvT, int64_t ldl, int64_t M, void* Tfr, size_t tfr_bytes,
                                  mgp_stream_t stream) {
  if (!LinvT) return -1;
  if (ldl < M) return -2;
  if (M < 0) return -3;
  if (!Tfr) return -4;
  if (M == 0) return MGP_OK;
  if (tfr_bytes < mgp_x6_lower_bytes(M, 1)) return MGP_ERR_WORKSPACE;
  if (!aligned16(Tfr)) return MGP_ERR_ALIGN;
  const int64_t Mp = x6_mp(M);
  const int nmb = (int)(Mp / 32), nmk = (int)(Mp / 16);
  const int64_t nfrag = (int64_t)nmb * nmk;
  hipLaunchKernelGGL(split_tri_kernel<false>, dim3((unsigned)((nfrag + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, LinvT, ldl, (int64_t)0, M, nmb, nmk, nfrag, (bf16x8*)Tfr);
  return launch_status();
}

extern "C" int mgp_split_cols_x6(const float* A, int64_t lda, int64_t M, int64_t N, void* Afr,
                                 size_t afr_bytes, mgp_stream_t stream) {
  if (!A) return -1;
  if (lda < N) return -2;
  if (M < 0) return -3;
  if (N < 0) return -4;
  if (!Afr) return -5;
  if (M == 0 || N == 0) return MGP_OK;
  if (afr_bytes < mgp_x6_cols_bytes(M, N)) return MGP_ERR_WORKSPACE;
  if (!aligned16(Afr)) return MGP_ERR_ALIGN;
  const int nmk = (int)(x6_mp(M) / 16);
  const int64_t nfrag = (x6_np(N) / 32) * nmk;
  hipLaunchKernelGGL(split_cols_kernel, dim3((unsigned)((nfrag + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     A, lda, M, N, nmk, nfrag, (bf16x8*)Afr);
  return launch_status();
}

// absmax of the source into the trailer, then the scaled split.
extern "C" int mgp_split_lower_f16(const float* q_sqrt, int64_t ldqs, int64_t strideq, int64_t M, int32_t K,
                                   void* Lfr, size_t lfr_bytes, mgp_stream_t stream) {
  if (!q_sqrt) return -1;
  if (ldqs < M) return -2;
  if (K > 1 && strideq < ldqs * M) return -3;
  if (M < 0) return -4;
  if (K < 0) return -5;
  if (!Lfr) return -6;
  if (M == 0 || K == 0) return MGP_OK;
  if (lfr_bytes < mgp_x6_lower_bytes(M, K)) return MGP_ERR_WORKSPACE;
  if (!aligned16(Lfr)) return MGP_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  float* bound = trailer(Lfr, lower_planes(M, K));
  int st = hip_status(hipMemsetAsync(bound, 0, sizeof(float), s));
  if (st) return st;
  const int64_t rows = (int64_t)K * M;
  launch_absmax<1>(q_sqrt, ldqs, strideq, M, M, rows, bound, s);
  st = launch_status();
  if (st) return st;
  const int64_t Mp = x6_mp(M);
  const int nmb = (int)(Mp / 32), nmk = (int)(Mp / 16);
  const int64_t nfrag = (int64_t)K * nmb * nmk;
  hipLaunchKernelGGL(split_tri_kernel<true>, dim3((unsigned)((nfrag + 3) / 4)), dim3(256), 0, s, q_sqrt, ldqs,
                     strideq, M, nmb, nmk, nfrag, (bf16x8*)Lfr, (const float*)bound);
  return launch_status();
}

// Per layer: the KL partial sums [nblk][3] doubles, then the block maxima [nblk] floats.
static int64_t qsqrt_nblk(int64_t M, int32_t K) { return (int64_t)K * ((M + kKlRows - 1) / kKlRows) + 1; }

extern "C" size_t mgp_qsqrt_workspace_bytes(int64_t M, int32_t K) {
  if (M <= 0 || K <= 0) return 0;
  const int64_t n = qsqrt_nblk(M, K);
  return (size_t)((n * 3 * 8 + n * 4 + 15) / 16 * 16);
}

extern "C" int mgp_qsqrt_images_kl_f16_batch(int32_t batch, const float* const* q_mu, int64_t ldq,
                                             const float* const* q_sqrt, int64_t ldqs, int64_t strideq, int64_t M,
                                             int32_t K, void* const* Lfr, size_t lfr_bytes, double* const* kl_out,
                                             void* workspace, size_t workspace_bytes, mgp_stream_t stream) {
  if (batch < 1 || batch > 2) return -1;
  if (!q_mu) return -2;
  if (ldq < K) return -3;
  if (!q_sqrt) return -4;
  if (ldqs < M) return -5;
  if (K > 1 && strideq < ldqs * M) return -6;
  if (M < 1) return -7;
  if (K < 1) return -8;
  if (!Lfr) return -9;
  if (lfr_bytes < mgp_x6_lower_bytes(M, K)) return -10;
  if (!kl_out) return -11;
  if ((ldqs & 3) || (strideq & 3)) return MGP_ERR_ALIGN;   // the KL sums' float4 rows
  const size_t wb = mgp_qsqrt_workspace_bytes(M, K);
  if (!workspace || workspace_bytes < wb * (size_t)batch) return MGP_ERR_WORKSPACE;
  if (!aligned16(workspace)) return MGP_ERR_ALIGN;
  const int64_t nblk = qsqrt_nblk(M, K);
  QLayer l[2];
  for (int b = 0; b < 2; ++b) {
    const int s = b < batch ? b : 0;
    if (!q_mu[s]) return -2;
    if (!q_sqrt[s]) return -4;
    if (!Lfr[s]) return -9;
    if (!kl_out[s]) return -11;
    if (!aligned16(q_sqrt[s]) || !aligned16(Lfr[s])) return MGP_ERR_ALIGN;
    char* w = (char*)workspace + wb * (size_t)s;
    l[b] = QLayer{q_mu[s], q_sqrt[s], (bf16x8*)Lfr[s], trailer(Lfr[s], lower_planes(M, K)), kl_out[s],
                  (double*)w, (float*)(w + nblk * 3 * 8)};
  }
  hipStream_t st = (hipStream_t)stream;
  const int nrb = (int)((M + kKlRows - 1) / kKlRows);
  const int64_t kgrid = kQsGrid > 0 && nblk > kQsGrid ? kQsGrid : nblk;
  hipLaunchKernelGGL(kl_absmax2_kernel, dim3((unsigned)kgrid, (unsigned)batch), dim3(256), 0, st, l[0], l[1], ldq,
                     ldqs, strideq, M, K, nrb, (int)nblk);
  int rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(kl_final2_kernel, dim3((unsigned)batch), dim3(1024), 0, st, l[0], l[1], (int)nblk,
                     (double)M * (double)K);
  rc = launch_status();
  if (rc) return rc;
  const int64_t Mp = x6_mp(M);
  const int nmb = (int)(Mp / 32), nmk = (int)(Mp / 16);
  const int64_t nfrag = (int64_t)K * nmb * nmk;
  const int64_t sgrid = kQsGrid > 0 && (nfrag + 3) / 4 > kQsGrid ? kQsGrid : (nfrag + 3) / 4;
  hipLaunchKernelGGL(split_lower2_kernel, dim3((unsigned)sgrid, (unsigned)batch), dim3(256), 0, st, l[0],
                     l[1], ldqs, strideq, M, nmb, nmk, nfrag);
  return launch_status();
}

// L^-T (upper triangle) as a split-f16 T image for mgp_trsm_stats_f16: absmax
// of the triangle into the trailer, then the scaled split.
extern "C" int mgp_split_upper_f16(const float* LinvT, int64_t ldl, int64_t M, void* Tfr, size_t tfr_bytes,
                                   mgp_stream_t stream) {
  if (!LinvT) return -1;
  if (ldl < M) return -2;
  if (M < 0) return -3;
  if (!Tfr) return -4;
  if (M == 0) return MGP_OK;
  if (tfr_bytes < mgp_x6_lower_bytes(M, 1)) return MGP_ERR_WORKSPACE;
  if (!aligned16(Tfr)) return MGP_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  float* bound = trailer(Tfr, lower_planes(M, 1));
  int st = hip_status(hipMemsetAsync(bound, 0, sizeof(float), s));
  if (st) return st;
  launch_absmax<2>(LinvT, ldl, (int64_t)0, M, M, M, bound, s);
  st = launch_status();
  if (st) return st;
  const int64_t Mp = x6_mp(M);
  const int nmb = (int)(Mp / 32), nmk = (int)(Mp / 16);
  const int64_t nfrag = (int64_t)nmb * nmk;
  hipLaunchKernelGGL(split_tri_kernel<false>, dim3((unsigned)((nfrag + 3) / 4)), dim3(256), 0, s, LinvT, ldl,
                     (int64_t)0, M, nmb, nmk, nfrag, (bf16x8*)Tfr, (const float*)bound);
  return launch_status();
}

// mgp_split_upper_f16 whose trailer already holds max |LinvT| (written by
// mgp_kuu_potrf_trtri_ex into mgp_x6_bound_ptr(Tfr)): the split alone.
extern "C" int mgp_split_upper_f16_bounded(const float* LinvT, int64_t ldl, int64_t M, void* Tfr, size_t tfr_bytes,
                                           mgp_stream_t stream) {
  if (!LinvT) return -1;
  if (ldl < M) return -2;
  if (M < 0) return -3;
  if (!Tfr) return -4;
  if (M == 0) return MGP_OK;
  if (tfr_bytes < mgp_x6_lower_bytes(M, 1)) return MGP_ERR_WORKSPACE;
  if (!aligned16(Tfr)) return MGP_ERR_ALIGN;
  const int64_t Mp = x6_mp(M);
  const int nmb = (int)(Mp / 32), nmk = (int)(Mp / 16);
  const int64_t nfrag = (int64_t)nmb * nmk;
  const float* bound = trailer(Tfr, lower_planes(M, 1));
  hipLaunchKernelGGL(split_tri_kernel<false>, dim3((unsigned)((nfrag + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     LinvT, ldl, (int64_t)0, M, nmb, nmk, nfrag, (bf16x8*)Tfr, bound);
  return launch_status();
}

// mgp_split_upper_f16_bounded for `batch` (1 or 2) matrices at LinvT + b strideL into the
// images Tfr[b] (host array of device pointers) in one launch; bit-identical.
extern "C" int mgp_split_upper_f16_bounded_batch(int32_t batch, const float* LinvT, int64_t ldl, int64_t strideL,
                                                 int64_t M, void* const* Tfr, size_t tfr_bytes,
                                                 mgp_stream_t stream) {
  if (batch < 1 || batch > 2) return -9;   // its own code (-1 .. -8 name the arguments)
  if (!LinvT) return -2;
  if (ldl < M) return -3;
  if (batch > 1 && strideL < ldl * M) return -4;
  if (M < 0) return -5;
  if (!Tfr) return -6;
  for (int b = 0; b < batch; ++b) {
    if (!Tfr[b]) return -6;
    if (!aligned16(Tfr[b])) return MGP_ERR_ALIGN;
  }
  if (M == 0) return MGP_OK;
  if (tfr_bytes < mgp_x6_lower_bytes(M, 1)) return MGP_ERR_WORKSPACE;
  const int64_t Mp = x6_mp(M);
  const int nmb = (int)(Mp / 32), nmk = (int)(Mp / 16);
  const int64_t nfrag = (int64_t)nmb * nmk;
  void* t1 = Tfr[batch - 1];
  hipLaunchKernelGGL(split_upper2_kernel, dim3((unsigned)((nfrag + 3) / 4), (unsigned)batch), dim3(256), 0,
                     (hipStream_t)stream, LinvT, ldl, strideL, M, nmb, nmk, nfrag, (bf16x8*)Tfr[0],
                     (const float*)trailer(Tfr[0], lower_planes(M, 1)), (bf16x8*)t1,
                     (const float*)trailer(t1, lower_planes(M, 1)));
  return launch_status();
}

// Device address of the split-f16 scale bound in an image's trailer (lower /
// upper images: K = matrices in the batch; column images: K = 0, N columns).
extern "C" float* mgp_x6_bound_ptr(void* img, int64_t M, int64_t N, int32_t K) {
  if (!img || M <= 0) return nullptr;
  return trailer(img, K > 0 ? lower_planes(M, K) : cols_planes(M, N));
}

extern "C" int mgp_split_cols_f16(const float* A, int64_t lda, int64_t M, int64_t N, void* Afr,
                                  size_t afr_bytes, mgp_stream_t stream) {
  if (!A) return -1;
  if (lda < N) return -2;
  if (M < 0) return -3;
  if (N < 0) return -4;
  if (!Afr) return -5;
  if (M == 0 || N == 0) return MGP_OK;
  if (afr_bytes < mgp_x6_cols_bytes(M, N)) return MGP_ERR_WORKSPACE;
  if (!aligned16(Afr)) return MGP_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  float* bound = trailer(Afr, cols_planes(M, N));
  int st = hip_status(hipMemsetAsync(bound, 0, sizeof(float), s));
  if (st) return st;
  launch_absmax<0>(A, lda, (int64_t)0, M, N, M, bound, s);
  st = launch_status();
  if (st) return st;
  const int nmk = (int)(x6_mp(M) / 16);
  const int64_t nfrag = (x6_np(N) / 32) * nmk;
  hipLaunchKernelGGL(split_cols_kernel, dim3((unsigned)((nfrag + 3) / 4)), dim3(256), 0, s, A, lda, M, N, nmk,
                     nfrag, (bf16x8*)Afr, (const float*)bound);
  return launch_status();
}

// The C_k images of mgp_expert_conditional_f16c: one column image's planes per expert, no trailers.
extern "C" size_t mgp_c_images_bytes(int64_t M, int64_t N, int32_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 16;
  return (size_t)K * cols_planes(M, N);
}

extern "C" int mgp_colnorm_max(const float* q_sqrt, int64_t ldq, int64_t strideq, int64_t M, int32_t K,
                               float* out, mgp_stream_t stream) {
  if (!q_sqrt) return -1;
  if (ldq < M) return -2;
  if (M < 0) return -4;
  if (K < 1) return -5;
  if (!out) return -6;
  hipStream_t s = (hipStream_t)stream;
  int st = hip_status(hipMemsetAsync(out, 0, sizeof(float), s));
  if (st || M == 0) return st;
  hipLaunchKernelGGL(colnorm_max_kernel, dim3((unsigned)((M + 31) / 32), (unsigned)K), dim3(256), 0, s, q_sqrt, ldq,
                     strideq, M, (unsigned int*)out);
  return launch_status();
}
