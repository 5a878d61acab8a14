// The main loops of K4, K5 and the conditional backward on the 16-bit matrix cores at
// f32 accuracy ("split-bf16 x6"), with what those kernel families share around them.
//
// Every f32 operand x is split exactly into three bf16 planes,
//     x = hi + mid + lo (+ |x| 2^-25 at most),   hi = bf16(x), mid = bf16(x - hi),
//     lo = bf16(x - hi - mid)
// (each difference is exact in f32).  A product is formed from the six plane
// products whose weight is >= 2^-16 of the leading one,
//     a b ~ a_hi b_hi + a_hi b_mid + a_mid b_hi + a_hi b_lo + a_mid b_mid + a_lo b_hi,
// so the per-product error is a few f32 ulps and the sum is accumulated in the
// f32 MFMA accumulator -- the accuracy class of an f32 GEMM.  Six
// v_mfma_f32_32x32x16_bf16 (32 cycles each for 32x32x16) replace eight
// v_mfma_f32_32x32x2_f32 (64 cycles each for 32x32x2): 192 vs 512 cycles per
// 32x32x16 block, 2.7x the f32 matrix rate on the same silicon.
//
// Data layout: the fragment images of frag_image.hpp (built once per step by images.hip, K1 and K4).
//
// Staging (x6_mainloop; x6_mainloop16 is the same scheme per k-step pair): a 256-thread
// workgroup owns an item of 128 rows x 256 columns, wave w all 128 rows x 64 columns.
// Per k-step (16 deep) the workgroup stages the T fragments of its 4 row sub-tiles in
// LDS (double buffered, one barrier per k-step); each wave loads its B fragments
// straight from global into registers one k-step ahead.
//
// Here: ld_frag / img_rsrc (buffer loads of a fragment), col_major_item (the item map
// of the one-matrix products), x6_mainloop (32x32x16 MFMAs), x6_mainloop16 with the
// mfma16_* plane products (16x16x32 MFMAs), and the accumulator stores store_acc_f32 /
// store_acc_image.  Users: trsm_stats.hip (K4), expert_cond.hip (K5), cond_bwd.hip.
#pragma once

#include <type_traits>

#include "mgp_common.hpp"
#include "frag_image.hpp"

namespace mgp {

__device__ __forceinline__ bf16x8 ld_frag(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
  return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

// Item b -> (row tile t, column tile tn) for the one-matrix products (K4,
// gA, gKuf): the nT row tiles of a column tile are adjacent block ids on one
// XCD (b % 8), heaviest first, so the column slab of the B image they all read
// is served from that XCD's L2.
__device__ __forceinline__ void col_major_item(int b, int nT, int nTn, int& t, int& tn) {
  if (nTn % 8 == 0) {
    const int x = b & 7, j = b >> 3;
    t = nT - 1 - j % nT;
    tn = (j / nT) * 8 + x;
  } else {
    t = nT - 1 - b % nT;
    tn = b / nT;
  }
}

// Main loop shared by K4 and K5: acc[i][c] (row sub-tile i = 0..3 of the
// 128-row tile, column sub-tile c = 0..1 of this wave's 64 columns) +=
// sum over k-steps mk in [mk_begin, mk_end) (even count) of T-image blocks
// (4 t + i, mk) x B-image blocks (nb0 + c, mk).  T fragments are staged in LDS
// (shared by the 4 waves), B fragments go global -> registers one k-step ahead.
//   tbase: byte offset of T block (mb = 4 t, mk = 0) of this matrix
//   sB0:   byte offset of B block (nb0, mk = 0)
template <int V>
using ic = std::integral_constant<int, V>;

// DIAG_FIRST (K5, T lower: block (mb, mk) zero for 16 mk + 15 < 32 mb): the
// first 8 k-steps meet the diagonal and only sub-tiles i <= p of k-step pair p
// are non-zero.  Otherwise (K4, T upper: zero for 16 mk > 32 mb + 31) the last
// 8 k-steps do, with sub-tiles i >= p of pair p.  Those MFMAs are skipped
// (8% of the work), everything else is unchanged.
// DIAG: 1 = diagonal first (lower T), 2 = diagonal last (upper T), 0 = full T.
// NC: column sub-tiles (32 wide) per wave (B blocks nb0 .. nb0 + NC - 1).
// NPL: planes used (3 = x6 products; 2, 1 = K5's reduced modes, mfma_planes):
// only those planes are loaded and staged.
// F16: the images are split-f16 (mfma_fmt), NPL must be 2.
// X8 (with F16): image planes 0 (f16 hi) and 2 (e4m3 cross terms) are loaded;
// per k-step pair, two f16 hi products and one e4m3 MFMA for both pairs of
// cross terms (mfma_f8x): 2 + 2 f16-product-equivalents instead of 6.
// HOIST: all T fragment reads of a k-step issued before its MFMAs (trsm_bwd: 457 ->
// 438 us; K4 +2.5 %, K5 unchanged -- so only there).
// BH: called as bh(b, mk) on k-step mk's B fragments right before their MFMAs
// (trsm_bwd16_kernel's per-column rescale of the gA image); NoBHook: nothing.
struct NoBHook {
  template <class B>
  __device__ __forceinline__ void operator()(B&, int) const {}
};
template <int DIAG, int NC = 2, int NPL = 3, bool F16 = false, bool X8 = false, bool HOIST = false,
          typename BH = NoBHook>
__device__ __forceinline__ void x6_mainloop(floatx16 (&acc)[4][NC], bf16x8 (*sL)[4 * 3 * 64],
                                            __amdgpu_buffer_rsrc_t rT, uint32_t tbase,
                                            __amdgpu_buffer_rsrc_t rB, uint32_t sB0, int mk_begin,
                                            int mk_end, int nmk, bool init = true, BH bhook = BH{}) {
  static_assert(!X8 || (F16 && NPL == 2), "X8 reads split-f16 images");
  auto PL = [](int p) { return (X8 && p == 1) ? 2 : p; };  // LDS / register plane -> image plane
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t vB = 16u * lane;
  const uint32_t sBc = (uint32_t)nmk * 3u * kFragBytes;  // B block nb0 + c at sB0 + c sBc
  // T stage: 256 NPL 16-B units per k-step, NPL per thread: unit e = tid + 256 s ->
  //   row sub-tile i = e / (64 NPL), plane p = (e / 64) % NPL, lane e % 64
  //   byte offset tbase + ((i * nmk + mk) * 192 + p * 64 + lane) * 16; LDS unit (3 i + p) * 64 + lane
  uint32_t vT[NPL];
  int dT[NPL];
#pragma unroll
  for (int s = 0; s < NPL; ++s) {
    const int e = tid + 256 * s, i = e / (64 * NPL), p = (e / 64) % NPL;
    vT[s] = (uint32_t)((i * nmk * 192 + PL(p) * 64 + (e & 63)) * 16);
    dT[s] = (3 * i + p) * 64 + (e & 63);
  }
  if (init) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][c][e] = 0.f;
  }

  auto load_b = [&](bf16x8 (&b)[NC][3], int mk) {
    const uint32_t o = (uint32_t)mk * 3u * kFragBytes;
#pragma unroll
    for (int p = 0; p < NPL; ++p)
#pragma unroll
      for (int c = 0; c < NC; ++c) b[c][p] = ld_frag(rB, vB, sB0 + c * sBc + o + PL(p) * kFragBytes);
  };
  auto load_t = [&](u32x4v (&st)[NPL], int mk) {
    const uint32_t o = tbase + (uint32_t)mk * 192u * 16u;
#pragma unroll
    for (int s = 0; s < NPL; ++s) st[s] = __builtin_amdgcn_raw_buffer_load_b128(rT, vT[s], o, 0);
  };
  auto store_t = [&](int buf, const u32x4v (&st)[NPL]) {
#pragma unroll
    for (int s = 0; s < NPL; ++s) reinterpret_cast<u32x4v*>(sL[buf])[dT[s]] = st[s];
  };
  auto compute = [&](int buf, const bf16x8 (&b)[NC][3], auto ilo, auto ihi) {
    constexpr int ILO = decltype(ilo)::value, IHI = decltype(ihi)::value;
    if constexpr (HOIST) {  // every T fragment read of the k-step before its first MFMA
    bf16x8 a[4][3];
#pragma unroll
    for (int i = ILO; i < IHI; ++i)
#pragma unroll
      for (int p = 0; p < NPL; ++p) a[i][p] = sL[buf][(i * 3 + p) * 64 + lane];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = ILO; i < IHI; ++i)
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[i][c] = mfma_fmt<NPL, F16>(a[i], b[c], acc[i][c]);
    } else {
#pragma unroll
    for (int i = ILO; i < IHI; ++i) {
      bf16x8 a[3];
#pragma unroll
      for (int p = 0; p < NPL; ++p) a[p] = sL[buf][(i * 3 + p) * 64 + lane];
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[i][c] = mfma_fmt<NPL, F16>(a, b[c], acc[i][c]);
    }
    }
  };

  // X8: the first k-step of a pair keeps its cross-term fragments for the second
  bf16x8 ax_s[4], bx_s[NC];
  auto compute_x8 = [&](int buf, const bf16x8 (&b)[NC][3], auto ilo, auto ihi, auto second) {
    constexpr int ILO = decltype(ilo)::value, IHI = decltype(ihi)::value;
    constexpr bool SECOND = decltype(second)::value;
#pragma unroll
    for (int i = ILO; i < IHI; ++i) {
      const bf16x8 a_hi = sL[buf][(i * 3) * 64 + lane], a_x = sL[buf][(i * 3 + 1) * 64 + lane];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if constexpr (SECOND) acc[i][c] = mfma_f8x(ax_s[i], a_x, bx_s[c], b[c][1], acc[i][c]);
        acc[i][c] = mfma_f16(a_hi, b[c][0], acc[i][c]);
      }
      if constexpr (!SECOND) ax_s[i] = a_x;
    }
    if constexpr (!SECOND) {
#pragma unroll
      for (int c = 0; c < NC; ++c) bx_s[c] = b[c][1];
    }
  };

  bf16x8 b0[NC][3], b1[NC][3];
  u32x4v st[NPL];
  load_t(st, mk_begin);
  load_b(b0, mk_begin);
  store_t(0, st);
  __syncthreads();
  // two k-steps per iteration: LDS buffers and fragment sets alternate
  // one pair of k-steps (mk, mk + 1) on sub-tiles [ilo, ihi); sched_barrier(0)
  // pins the prefetch loads ahead of the MFMA block
  auto pair = [&](int mk, auto ilo, auto ihi) {
    load_t(st, mk + 1);
    load_b(b1, mk + 1);
    __builtin_amdgcn_sched_barrier(0);
    bhook(b0, mk);
    if constexpr (X8)
      compute_x8(0, b0, ilo, ihi, std::false_type{});
    else
      compute(0, b0, ilo, ihi);
    __builtin_amdgcn_sched_barrier(0);
    store_t(1, st);
    __syncthreads();
    const int m2 = mk + 2 < nmk ? mk + 2 : nmk - 1;  // after the last pair: harmless reload
    load_t(st, m2);
    load_b(b0, m2);
    __builtin_amdgcn_sched_barrier(0);
    bhook(b1, mk + 1);
    if constexpr (X8)
      compute_x8(1, b1, ilo, ihi, std::true_type{});
    else
      compute(1, b1, ilo, ihi);
    __builtin_amdgcn_sched_barrier(0);
    store_t(0, st);
    __syncthreads();
  };
  if constexpr (DIAG == 1) {
    pair(mk_begin, ic<0>{}, ic<1>{});
    pair(mk_begin + 2, ic<0>{}, ic<2>{});
    pair(mk_begin + 4, ic<0>{}, ic<3>{});
    pair(mk_begin + 6, ic<0>{}, ic<4>{});
#pragma nounroll
    for (int mk = mk_begin + 8; mk < mk_end; mk += 2) pair(mk, ic<0>{}, ic<4>{});
  } else if constexpr (DIAG == 0) {
#pragma nounroll
    for (int mk = mk_begin; mk < mk_end; mk += 2) pair(mk, ic<0>{}, ic<4>{});
  } else {
#pragma nounroll
    for (int mk = mk_begin; mk < mk_end - 8; mk += 2) pair(mk, ic<0>{}, ic<4>{});
    pair(mk_end - 8, ic<0>{}, ic<4>{});
    pair(mk_end - 6, ic<1>{}, ic<4>{});
    pair(mk_end - 4, ic<2>{}, ic<4>{});
    pair(mk_end - 2, ic<3>{}, ic<4>{});
  }
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t img_rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, (int)bytes, 0x00020000);
}

// ------------------------------------------------------------------ K5 (split-f16) on 16x16x32 MFMAs
// The same contraction, items and split-f16 images as expert_cond_x6_kernel<2, true>,
// on v_mfma_f32_16x16x32_f16 (16 cycles per 16x16x32 block: the same cycles per flop
// as 32x32x16; the chip can hold a different clock per shape under load,
// MI355X_MICROARCH.md, DVFS give-back item 7).  No new image format: one k-step PAIR
// (32 deep) of the existing fragments is one MFMA k-step; lane l (i = l % 16,
// q = l / 16) takes the 16 bytes of fragment k-step 2 ks + q / 2 at lane position
// 16 (row block % 2) + i + 32 (q % 2) -- its 8 elements are 8 of the 32 m of the pair,
// the same 8 for the A operand (L_k^T, rows m') and the B operand (A, columns n), so
// the contraction is unchanged.  Wave w: 128 rows x 64 columns = 8 x 4 blocks of
// 16 x 16; per pair the L fragments of the item's 4 row sub-tiles (16 KiB) are staged
// in LDS (double buffered, one barrier per pair), the wave's B fragments go global ->
// registers one pair ahead; 96 MFMAs per wave and pair.
typedef float floatx4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ floatx4v mfma16_f16(bf16x8 a, bf16x8 b, floatx4v c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(halfx8, a), __builtin_bit_cast(halfx8, b), c,
                                                0, 0, 0);
}
__device__ __forceinline__ floatx4v mfma16_bf16(bf16x8 a, bf16x8 b, floatx4v c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// one 16x16 block: the plane products of mfma_fmt (x6: six bf16, split-f16: three f16)
template <int NPL, bool F16>
__device__ __forceinline__ floatx4v mfma16_fmt(const bf16x8 (&a)[3], const bf16x8 (&b)[3], floatx4v acc) {
  if constexpr (F16) {
    acc = mfma16_f16(a[1], b[0], acc);
    acc = mfma16_f16(a[0], b[1], acc);
    return mfma16_f16(a[0], b[0], acc);
  } else if constexpr (NPL == 3) {
    acc = mfma16_bf16(a[2], b[0], acc);
    acc = mfma16_bf16(a[1], b[1], acc);
    acc = mfma16_bf16(a[0], b[2], acc);
    acc = mfma16_bf16(a[1], b[0], acc);
    acc = mfma16_bf16(a[0], b[1], acc);
    return mfma16_bf16(a[0], b[0], acc);
  } else if constexpr (NPL == 2) {
    acc = mfma16_bf16(a[1], b[0], acc);
    acc = mfma16_bf16(a[0], b[1], acc);
    return mfma16_bf16(a[0], b[0], acc);
  } else {
    return mfma16_bf16(a[0], b[0], acc);
  }
}

// Main loop of the 16x16x32 kernels: acc[ib][cb] (16-row block ib = 0..7 of the 128-row
// item, 16-column block cb = 0..3 of this wave's 64 columns) += sum over k-step PAIRS
// ks in [ks_begin, ks_end) (even count) of T-image rows x B-image columns.  T fragments
// of the item's 4 row sub-tiles, both k-steps of a pair and NPL planes are staged in LDS
// (double buffered, one barrier per pair); B fragments go global -> registers one pair
// ahead.  DIAG = 1: T lower (K5): the first 4 pairs meet the diagonal, pair p has row
// blocks ib <= 2 p + 1; DIAG = 2: T upper (K4): the last 4 pairs do, pair p of them has
// ib >= 2 p; 0: full.  (The zero sub-blocks inside come from the images' zero fill.)
//   tbase: byte offset of T fragment (mb = 4 t, mk = 0); sB0: of B fragment (nb0, mk = 0)
template <int DIAG, int NPL, bool F16>
__device__ __forceinline__ void x6_mainloop16(floatx4v (&acc)[8][4], bf16x8 (*sL)[4 * 2 * 3 * 64],
                                              __amdgpu_buffer_rsrc_t rT, uint32_t tbase, __amdgpu_buffer_rsrc_t rB,
                                              uint32_t sB0, int ks_begin, int ks_end, int nmk) {
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, q = lane >> 4;
  // T staging: unit e = tid + 256 s (NPL 2: 4 units, 3: 6 units per thread): sub-tile
  // i = e / (128 NPL), k-step kk = (e / (64 NPL)) % 2, plane p = (e / 64) % NPL, position e % 64
  constexpr int NU = 2 * NPL;
  uint32_t vT[NU];
#pragma unroll
  for (int s = 0; s < NU; ++s) {
    const int e = tid + 256 * s, i = e / (128 * NPL), kk = (e / (64 * NPL)) % 2, p = (e / 64) % NPL;
    vT[s] = (uint32_t)((((i * nmk + kk) * 3 + p) * 64 + (e & 63)) * 16);
  }
  // B: column block cb, plane p, pair ks: fragment nb0 + cb / 2, k-step 2 ks + q / 2,
  // position 16 (cb % 2) + li + 32 (q % 2)
  const uint32_t vB = (uint32_t)((((q >> 1) * 3) * 64 + li + 32 * (q & 1)) * 16);
  auto boff = [&](int cb, int p, int ks) {
    return sB0 + (uint32_t)(cb >> 1) * (uint32_t)nmk * 3u * kFragBytes + (uint32_t)((2 * ks) * 3 + p) * kFragBytes +
           (uint32_t)(16 * (cb & 1)) * 16u;
  };
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[i][c] = floatx4v{0.f, 0.f, 0.f, 0.f};
  auto load_b = [&](bf16x8 (&b)[4][3], int ks) {
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int p = 0; p < NPL; ++p) b[cb][p] = ld_frag(rB, vB, boff(cb, p, ks));
  };
  auto load_t = [&](u32x4v (&st)[NU], int ks) {
    const uint32_t o = tbase + (uint32_t)(2 * ks) * 3u * kFragBytes;
#pragma unroll
    for (int s = 0; s < NU; ++s) st[s] = __builtin_amdgcn_raw_buffer_load_b128(rT, vT[s], o, 0);
  };
  auto store_t = [&](int buf, const u32x4v (&st)[NU]) {
#pragma unroll
    for (int s = 0; s < NU; ++s) reinterpret_cast<u32x4v*>(sL[buf])[tid + 256 * s] = st[s];
  };
  // A operand of row block ib, plane p: sub-tile ib / 2, k-step q / 2, position 16 (ib % 2) + li + 32 (q % 2)
  const int aoff = (q >> 1) * 64 * NPL + li + 32 * (q & 1);
  auto compute = [&](int buf, const bf16x8 (&b)[4][3], auto ilo, auto ihi) {
    constexpr int ILO = decltype(ilo)::value, IHI = decltype(ihi)::value;
#pragma unroll
    for (int ib = ILO; ib < IHI; ++ib) {
      const int base = (ib >> 1) * 128 * NPL + 16 * (ib & 1) + aoff;
      bf16x8 a[3];
#pragma unroll
      for (int p = 0; p < NPL; ++p) a[p] = sL[buf][base + 64 * p];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) acc[ib][cb] = mfma16_fmt<NPL, F16>(a, b[cb], acc[ib][cb]);
    }
  };
  bf16x8 b0[4][3], b1[4][3];
  u32x4v st[NU];
  load_t(st, ks_begin);
  load_b(b0, ks_begin);
  store_t(0, st);
  __syncthreads();
  auto two = [&](int ks, auto ilo0, auto ihi0, auto ilo1, auto ihi1) {
    load_t(st, ks + 1);
    load_b(b1, ks + 1);
    __builtin_amdgcn_sched_barrier(0);
    compute(0, b0, ilo0, ihi0);
    __builtin_amdgcn_sched_barrier(0);
    store_t(1, st);
    __syncthreads();
    const int k2 = ks + 2 < ks_end ? ks + 2 : ks_end - 1;  // after the last pair: harmless reload
    load_t(st, k2);
    load_b(b0, k2);
    __builtin_amdgcn_sched_barrier(0);
    compute(1, b1, ilo1, ihi1);
    __builtin_amdgcn_sched_barrier(0);
    store_t(0, st);
    __syncthreads();
  };
  if constexpr (DIAG == 1) {
    two(ks_begin, ic<0>{}, ic<2>{}, ic<0>{}, ic<4>{});
    two(ks_begin + 2, ic<0>{}, ic<6>{}, ic<0>{}, ic<8>{});
#pragma nounroll
    for (int ks = ks_begin + 4; ks < ks_end; ks += 2) two(ks, ic<0>{}, ic<8>{}, ic<0>{}, ic<8>{});
  } else if constexpr (DIAG == 0) {
#pragma nounroll
    for (int ks = ks_begin; ks < ks_end; ks += 2) two(ks, ic<0>{}, ic<8>{}, ic<0>{}, ic<8>{});
  } else {
#pragma nounroll
    for (int ks = ks_begin; ks < ks_end - 4; ks += 2) two(ks, ic<0>{}, ic<8>{}, ic<0>{}, ic<8>{});
    two(ks_end - 4, ic<0>{}, ic<8>{}, ic<2>{}, ic<8>{});
    two(ks_end - 2, ic<4>{}, ic<8>{}, ic<6>{}, ic<8>{});
  }
}

// Store a 128 x 256 item's accumulators (wave w: 128 rows x 64 columns) as f32
// rows [i0 + .][n0 + .] of out (M rows, leading dimension ld), each column n
// scaled by colscale[n] (if given).  Buffer stores with 32-bit offsets: rows
// beyond M fall outside the resource and are dropped.
__device__ __forceinline__ void store_acc_f32(const floatx16 (&acc)[4][2], float* __restrict__ out, int64_t ld,
                                              int64_t i0, int64_t n0, int64_t M, int64_t N,
                                              const float* __restrict__ colscale) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc((void*)out, (short)0, (int)(uint32_t)(M * ld * 4), 0x00020000);
  const uint32_t soff = (uint32_t)((i0 * ld + n0) * 4);
  const uint32_t ld32 = (uint32_t)ld;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int nl = 64 * w + 32 * c + (lane & 31);
    const int64_t n = n0 + nl;
    if (n < N) {
      const float cs = colscale ? colscale[n] : 1.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const uint32_t rl = (uint32_t)(32 * i + acc_row(e, lane));
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, acc[i][c][e] * cs), r,
                                                (rl * ld32 + (uint32_t)nl) * 4u, soff, 0);
        }
    }
  }
}

// Store the accumulators as the split image [nb][mk] of the item's 128 x 256
// block (as K4 does for A), columns scaled by colscale[n] (0 beyond N).
__device__ __forceinline__ void store_acc_image(const floatx16 (&acc)[4][2], bf16x8* __restrict__ img, int nmk,
                                                int t, int tn, int64_t N, const float* __restrict__ colscale) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int64_t nb = 8 * (int64_t)tn + 2 * w + c;
    const int64_t n = 32 * nb + (lane & 31);
    const float cs = colscale ? (n < N ? colscale[n] : 0.f) : 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t mk = 8 * (int64_t)t + 2 * i;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = acc[i][c][8 * s + j] * cs;
        store_split(img + ((nb * nmk + mk + s) * 3) * 64 + lane, v);
      }
    }
  }
}

}  // namespace mgp
