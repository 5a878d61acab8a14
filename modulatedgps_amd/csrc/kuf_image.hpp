// K1's block body (Kuf = K(Z, X) written as a split-bf16 / split-f16 fragment image),
// shared by its own launch (rbf.hip: rbf_kuf_x6_kernel) and by the extra workgroups
// the K3 step launches carry (chol.hip: chol_step_pair's Kuf side job).
//
// Reference: MixtureGPs/models.py:139 (self.kernel.K(Z, Xnew)); GPflow 2.7
// SquaredExponential.K_r2(r2) = var * exp(-0.5 r2), r2 = square_distance(X / l, Z / l).
//
// Numerics: z' and x' are the inputs RELATIVE TO A REFERENCE POINT OF THE LAYER, scaled:
// z' = (z - ref) c, x' = (x - ref) c, c_d = sqrt(0.5 log2 e) / l_d, with
// ref = Z[0] + mean_i (Z[i M / 32] - Z[0]), i < 32 (a cheap centre of the inducing points:
// Z[0] alone doubles |z'|^2 + |x'|^2 on centred data).  Both subtractions, of Z[0] and of
// the offset from it, are done on the raw coordinates where they are loaded (block
// prologue), before the multiply by c.  The three terms of the expanded form below
// cancel, so the absolute f32 error of r2 is a few eps32 (|z'|^2 + |x'|^2): with the
// reference point taken out that is the squared spread of the data about it in
// lengthscale units, not the squared distance from the origin, and
// K(Z + c, X + c) = K(Z, X) -- bit for bit whenever the shifted coordinates and their
// differences are exact in float32 (only differences of raw coordinates are formed).
// The offset from Z[0] (kuf_centre_offset, a fixed summation order: the same bits wherever
// it is computed) lives in floats [32, 64) of the image's trailer.  The stand-alone
// launch's blocks each compute it (block 0 stores it); for K3's side job the prep launch
// computes it once per layer and the step launches' blocks read it (PRE), because the
// 31 row loads inlined into the step kernel cost that kernel 60 to 330 more spilled
// SGPRs and K3 a fifth of its time.  Either way the images are byte-identical.
// Data that spans tens of lengthscales is still out of reach of the expanded form at
// f32 class (inputs over 20 lengthscales: ~1e-6 normwise).
// D = 1 (DMAX = 1: time series, where the inputs span the most lengthscales) does not
// use the expanded form: rows carry (z', 1), columns (1, -x'), the one MFMA product is
// the difference z' - x' (products by 1 exact, one rounding) and each lane squares its
// accumulators -- the direct form sum_d (z'_d - x'_d)^2, never negative, whose error is
// that of the scaled coordinates only (eps32 |z' - x'| (|z'| + |x'|)).  That error is
// linear in the distance from the reference point, so there z' and x' are taken from Z[0]
// itself: the arithmetic of rbf.hip's rbf_kernel.
//
// r2 = |z'|^2 + |x'|^2 - 2 z'.x' (the expanded form GPflow's
// square_distance uses) is ONE [32 x (D + 2)] x [(D + 2) x 32] product on
// v_mfma_f32_32x32x2_f32 (exact f32 products): rows of Z carry (z', |z'|^2, 1),
// columns of X carry (-2 x', 1, |x'|^2).  The accumulator of that MFMA holds
// row (r & 3) + 8 (r >> 2) + 4 h of column l & 31 in register r -- exactly the
// order of an image fragment: registers 0..7 / 8..15 of a 32x32 tile are the
// lane's 8 elements of k-steps 2 mb / 2 mb + 1.  So each lane finishes its 16
// values with one exp2 and one multiply each (variance and, split-f16, the
// image's power-of-two scale folded into one per-lane multiplier that is 0 on
// padded columns), splits them and stores 16-B fragments.
// Block = 4 waves (a 256-thread group) x 32 columns x 128 rows (4 row tiles per
// wave); block `bid` is row block bid % row_blocks of column group bid / row_blocks
// (consecutive blocks walk down a column group: adjacent image windows).
// Rows >= M and columns >= N of the padded image are written as zeros.
// F16: split-f16 image (Kuf <= variance, so the image scale is 2^img_exp(variance)
// and block 0 writes the variance into the trailer `bound`).
#pragma once

#include <type_traits>

#include "frag_image.hpp"

namespace mgp {

struct KufImageArgs {
  const float* X; int64_t ldx;
  const float* Z; int64_t ldz;
  int64_t N, M; int D;
  const float* variance; const float* ls; int n_ls;
  int nmk, row_blocks;
  bf16x8* Kfr; float* bound;
  float* centre;   // the image trailer's floats [32, 64): the reference point's offset from Z[0]
};

// LDS floats a group needs: zs [128][DP] + cs [2 KS] + rf [2][2 KS]
template <int DMAX>
constexpr int kuf_block_lds_floats() {
  return 128 * (2 * ((DMAX + 1) / 2 + 1) + 1) + 6 * ((DMAX + 1) / 2);
}

// Rows of Z whose mean places the reference point (rows i M / kKufCentre, i = 0 ..)
constexpr int kKufCentre = 32;
constexpr int kKufCentreFloats = 32;   // floats [32, 64) of the image's trailer hold the offset
// The reference point's offset from Z[0] in dimension d: the mean of Z[i M / 32][d] - Z[0][d],
// i < 32, summed in this order wherever it is computed (the stand-alone launch's blocks,
// K3's prep launch for the side job): the same bits.  Only differences of raw coordinates
// are formed, so the offset does not move with the data.
__device__ __forceinline__ float kuf_centre_offset(const float* __restrict__ Z, int64_t ldz, int64_t M, int d) {
  const float z0 = Z[d];
  float dl = 0.f;
  // (all 31 loads in flight: the block waits for them before its first barrier; eight at a
  // time kept the stand-alone kernel at 50 VGPRs but cost it 5 us of 47)
#pragma unroll
  for (int i = 1; i < kKufCentre; ++i) dl += Z[(i * M / kKufCentre) * ldz + d] - z0;
  return dl * (1.f / kKufCentre);
}

// Stores of the image fragments (16 B per lane): POL 0 plain, 1 non-temporal (streaming:
// fewer dirty L2 lines left for the kernel boundary to write back -- the K3 step
// launches' side job, where every boundary is on the Cholesky chain's critical path).
template <int POL>
__device__ __forceinline__ void img_store(bf16x8* p, bf16x8 v) {
  if constexpr (POL == 0) *p = v;
  else __builtin_nontemporal_store(v, p);
}

template <bool F16, int POL>
__device__ __forceinline__ void store_fragment(bf16x8* __restrict__ dst, const float (&v)[8]) {
  if constexpr (POL == 0) {
    if constexpr (F16) store_split_f16(dst, v, 1.f);
    else store_split(dst, v);
  } else if constexpr (F16) {   // store_split_f16 (no e4m3 plane) with POL stores
    halfx8 h, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const _Float16 hi = (_Float16)v[j];
      h[j] = hi;
      l[j] = (_Float16)(v[j] - (float)hi);
    }
    img_store<POL>(dst, __builtin_bit_cast(bf16x8, h));
    img_store<POL>(dst + 64, __builtin_bit_cast(bf16x8, l));
  } else {                      // store_split with POL stores
    bf16x8 h, m, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      __bf16 a, b, c;
      split_bf16x3(v[j], a, b, c);
      h[j] = a; m[j] = b; l[j] = c;
    }
    img_store<POL>(dst, h);
    img_store<POL>(dst + 64, m);
    img_store<POL>(dst + 128, l);
  }
}

// One block by the 256 threads of a group (t = thread index within the group).  Every
// thread of the WORKGROUP must call it the same number of times: it takes three
// __syncthreads(); a group with nothing to do passes active = false (it joins the
// barriers, loads and stores nothing).  lds: kuf_block_lds_floats<DMAX>() floats of
// this group's own.
template <int DMAX, bool F16, int POL = 0, bool PRE = false>
__device__ __forceinline__ void kuf_image_block(const KufImageArgs& a, int64_t bid, int t, bool active,
                                                float* __restrict__ lds) {
  constexpr int KS = (DMAX + 1) / 2;     // MFMA k-steps over the dims (2 each) ...
  constexpr int KA = KS + 1;             // ... + one for the (|z'|^2, 1) x (1, |x'|^2) terms
  constexpr int KM = DMAX == 1 ? 1 : KA; // MFMAs per tile (D = 1: the one difference product)
  constexpr int DP = 2 * KA + 1;         // LDS row pitch (odd: spreads banks)
  float* zs = lds;
  float* cs = lds + 128 * DP;
  float* rf = cs + 2 * KS;               // reference point: rf[d] = Z[0][d], rf[2 KS + d] = offset from it
  const int lane = t & 63, w = t >> 6, h = lane >> 5, c32 = lane & 31;
  const int64_t rb = bid % a.row_blocks, cg = bid / a.row_blocks;
  const int64_t nb = cg * 4 + w;
  const int64_t n = 32 * nb + c32;
  const int64_t m0 = 128 * rb;
  const float kHalfLog2e = 0.8493218002880191f;  // sqrt(0.5 * log2(e))
  // this thread's raw coordinates, issued before the scale and the reference point are
  // fetched (their latency overlaps; the arithmetic waits for the barrier): KS elements
  // of the block's Z rows and the KS dims of its column of X this lane half carries
  float zraw[KS], xraw[KS];
#pragma unroll
  for (int q = 0; q < KS; ++q) {
    const int i = t + 256 * q, r = i / (2 * KS), d = i % (2 * KS), dx = DMAX == 1 ? 0 : 2 * q + h;
    zraw[q] = (active && m0 + r < a.M && d < a.D) ? a.Z[(m0 + r) * a.ldz + d] : 0.f;
    xraw[q] = (active && n < a.N && dx < a.D) ? a.X[n * a.ldx + dx] : 0.f;
  }
  if (active && t < 2 * KS) {
    cs[t] = (t < a.D) ? kHalfLog2e / a.ls[a.n_ls == 1 ? 0 : t] : 0.f;
    // the reference point Z[0] + offset (kuf_centre_offset): read from the image's trailer
    // where a launch before this one has put it (PRE: K3's side job), computed here otherwise
    float z0 = 0.f, dl = 0.f;
    if (t < a.D) {
      z0 = a.Z[t];
      dl = PRE ? a.centre[t] : kuf_centre_offset(a.Z, a.ldz, a.M, t);
    }
    rf[t] = z0;
    rf[2 * KS + t] = dl;
    if (!PRE && bid == 0) a.centre[t] = dl;
  }
  if (!PRE && active && bid == 0 && t >= 2 * KS && t < kKufCentreFloats) a.centre[t] = 0.f;
  __syncthreads();
  float xk[KA], xx = 0.f;
  if (active) {
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      const int i = t + 256 * q, r = i / (2 * KS), d = i % (2 * KS);
      const int64_t m = m0 + r;
      if constexpr (DMAX == 1)   // rows carry (z', 1), z' from Z[0]
        zs[r * DP + d] = d ? 1.f : (m < a.M) ? (zraw[q] - rf[0]) * cs[0] : 0.f;
      else
        zs[r * DP + d] = (m < a.M && d < a.D) ? ((zraw[q] - rf[d]) - rf[2 * KS + d]) * cs[d] : 0.f;
    }
    if constexpr (DMAX == 1) {
      // columns carry (1, -x'): the product is the difference z' - x' itself
      const float x0 = (n < a.N) ? (xraw[0] - rf[0]) * cs[0] : 0.f;
      xk[0] = h ? -x0 : 1.f;
    } else {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int d = 2 * s + h;
        const float xd = (n < a.N && d < a.D) ? ((xraw[s] - rf[d]) - rf[2 * KS + d]) * cs[d] : 0.f;
        xx = fmaf(xd, xd, xx);
        xk[s] = -2.f * xd;
      }
    }
  } else if constexpr (DMAX == 1) {
    xk[0] = 0.f;
  }
  xx += __shfl_xor(xx, 32, 64);  // the two lane halves hold the even / odd dims
  xk[KS] = h ? xx : 1.f;         // k = 2 KS: |z'|^2 * 1, k = 2 KS + 1: 1 * |x'|^2
  __syncthreads();
  if (DMAX > 1 && active && t < 128) {
    float s2 = 0.f;
#pragma unroll
    for (int d = 0; d < 2 * KS; ++d) s2 = fmaf(zs[t * DP + d], zs[t * DP + d], s2);
    zs[t * DP + 2 * KS] = s2;
    zs[t * DP + 2 * KS + 1] = 1.f;
  }
  __syncthreads();
  if (!active) return;
  const float var = a.variance[0];
  // the image scale (a power of two, split-f16) and the variance fold into one
  // per-lane multiplier; padded columns (n >= N) get 0 (their r2 is finite)
  float mult = var;
  if constexpr (F16) {
    mult = var * ldexpf(1.f, img_exp(var));
    if (bid == 0 && t == 0) *a.bound = var;
  }
  if (n >= a.N) mult = 0.f;
  auto tiles = [&](auto ragged) {
    constexpr bool RAGGED = decltype(ragged)::value;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      floatx16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
      for (int s = 0; s < KM; ++s) acc = mfma32x32x2(zs[(32 * i + c32) * DP + 2 * s + h], xk[s], acc);
      if constexpr (DMAX == 1) {
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] *= acc[e];
      }
      const int64_t mb = (m0 >> 5) + i;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          // acc = r2 >= 0 up to rounding; raw v_exp_f32 (results below 2^-126 flush)
          v[j] = __builtin_amdgcn_exp2f(-acc[8 * half + j]) * mult;
          if constexpr (RAGGED)
            if (m0 + 32 * i + acc_row(8 * half + j, lane) >= a.M) v[j] = 0.f;
          // the split below must see v as the rounded f32 value: without this the
          // compiler contracts the multiply into the hi / lo conversions
          // (v_fma_mix{lo,hi}_f16 on the unrounded product beside v_cvt_pk_f16_f32 of
          // the rounded one), which left the lo plane inconsistent with hi whenever
          // mult is not a power of two (kernel variance 0.1: Kuf image off by half an
          // f16 ulp of hi, 3e-4 of the maximum, tests/diag_f16_images.py)
          asm volatile("" : "+v"(v[j]));
        }
        store_fragment<F16, POL>(a.Kfr + ((nb * a.nmk + 2 * mb + half) * 3) * 64 + lane, v);
      }
    }
  };
  if (m0 + 128 <= a.M)   // uniform: only the last row block is ragged
    tiles(std::false_type{});
  else
    tiles(std::true_type{});
}

// The image geometry of a Kuf image (rbf.hip's launch, chol.hip's side job): row
// blocks of kKufRows rows, column groups of kKufCols columns over the padded Np = x6_np(N);
// kuf_nmk: the image's k-steps (its fragment index stride per column block).
constexpr int kKufRows = 128, kKufCols = 128;   // kuf_image_block: 4 row tiles of 32, 4 waves x 32 columns
static_assert(kX6BM % kKufRows == 0 && kX6BN % kKufCols == 0, "Kuf blocks tile the padded image");
inline int kuf_row_blocks(int64_t M) { return (int)(x6_mp(M) / kKufRows); }
inline int64_t kuf_blocks(int64_t M, int64_t N) { return (x6_np(N) / kKufCols) * kuf_row_blocks(M); }
inline int kuf_nmk(int64_t M) { return (int)(x6_mp(M) / 16); }

}  // namespace mgp
