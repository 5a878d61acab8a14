// The fragment-image layout shared by every producer and consumer of the split-bf16 ("x6") and
// split-f16 images: tile sizes, padded extents, plane and trailer sizes (host and device), and the
// host launchers of images.hip's builder kernels that other files need.
#pragma once

#include "mgp_common.hpp"

namespace mgp {

// Data layout ("fragment images", built once per step, 6 B per element):
//   Lfr[k][mb][mk][p][lane][8]  A-operand of (L_k)^T: lane (r = lane&31,
//       h = lane>>5), element j holds L_k[m][m'] with m' = 32 mb + r and
//       m = 16 mk + kperm(h, j), kperm(h, j) = (j&3) + 8 (j>>2) + 4 h; zero above
//       the diagonal (m < m') and outside M.
//   Afr[nb][mk][p][lane][8]     B-operand of A: element j holds
//       A[16 mk + kperm(h, j)][32 nb + r]; zero outside M x N.
// kperm is the row order in which a 32x32 MFMA accumulator holds its rows
// (register 8s + j of lane half h is row 16 s + kperm(h, j)), so K4's epilogue
// can emit A's image straight from its accumulators; both operands use the
// same k order, which leaves the contraction unchanged.
// Each fragment is 1 KiB contiguous per plane: a wave reads it with one
// coalesced 16-B-per-lane load (global for A, LDS for L), no transposes.
constexpr int kX6BM = 128;   // rows m' per item
constexpr int kX6BN = 256;   // columns n per item
constexpr int kFragBytes = 1024;

// (constexpr: callable from host and device code alike)
constexpr int64_t x6_mp(int64_t M) { return (M + kX6BM - 1) / kX6BM * kX6BM; }
constexpr int64_t x6_np(int64_t N) { return (N + kX6BN - 1) / kX6BN * kX6BN; }

// Image = fragment planes + a 256-byte trailer (a Kuf image keeps its reference point's
// offset in floats [32, 64), kuf_image.hpp) whose first float is the
// split-f16 scale bound (unused by split-bf16 images).
constexpr size_t kTrailer = 256;
constexpr size_t lower_planes(int64_t M, int32_t K) {
  const int64_t Mp = x6_mp(M);
  return (size_t)K * (size_t)(Mp / 32) * (size_t)(Mp / 16) * 3 * kFragBytes;
}
constexpr size_t cols_planes(int64_t M, int64_t N) {
  return (size_t)(x6_np(N) / 32) * (size_t)(x6_mp(M) / 16) * 3 * kFragBytes;
}
__host__ __device__ inline float* trailer(void* img, size_t planes) { return (float*)((char*)img + planes); }

// Host launchers of two of images.hip's kernels for the conditional backward, so that each kernel is
// compiled into one code object only (arguments as the kernels'; grids as images.hip's own launches).
// split_tri_kernel<LOWER, TRANS, FULL>, one workgroup per 4 fragments:
enum class TriImage {
  kUpperTrans,   // <false, true>: m <= m' kept, source read transposed (L_k as B-b's T operand)
  kLowerTrans,   // <true, true>: m >= m' kept, source read transposed (Linv from LinvT)
  kLowerFull,    // <true, false, true>: every entry (the full S_k)
};
void launch_split_tri(TriImage form, const float* src, int64_t ld, int64_t stride, int64_t M, int nmb, int nmk,
                      int64_t nfrag, bf16x8* img, const float* bound, hipStream_t s);
// absmax_kernel<TRI> (the values are its template argument):
enum class AbsTri { kAll = 0, kLower = 1, kUpper = 2 };
void launch_absmax_tri(AbsTri tri, const float* src, int64_t ld, int64_t stride, int64_t rows, int64_t cols,
                       int64_t nrows_total, float* out, hipStream_t s);

}  // namespace mgp
