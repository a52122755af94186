// Compressed points on the device: k_compress (affine wire points -> x and a flag byte) and k_decompress (x and flag -> affine wire
// points and a report), include/mnt753_hip.h "compressed points".  libff: operator<< / operator>> under #ifndef NO_PT_COMPRESSION,
// depends/libff/libff/algebra/curves/mnt753/mnt4753/mnt4753_g1.cpp:389-450, mnt4753_g2.cpp:419-460 and the two mnt6753 files.
//
// Mapping as in k_check_points and k_g2_subgroup: one lane per G1 point, one lane group (two / three lanes, the lane-split fields of
// curve753.hip.h) per G2 point, 256-thread workgroups.  Every element of the arrays has its own stride, so that the verifier
// decompresses A, B and C of a batch of proofs straight into the A | B | C rows of its staging buffer (mnt753_pairing.hip).
//
// k_decompress per point, the first rule that applies:
//   1. a flag bit 2-7 is set, or a component of x is >= q           -> MNT753_BAD_NONCANONICAL
//   2. the identity flag (bit 1) is set                              -> zero words, good, whatever x holds
//   3. rhs = x^3 + a x + b (twist: a', b') is not a square, or = 0   -> MNT753_BAD_OFF_CURVE (rhs = 0: the only point has y = 0, which
//                                                                       the wire form reads as the identity and which is in neither group)
//   4. y = the root whose parity (of y.c0 as an integer, out of Montgomery form) is bit 0 of the flag; fp_sqrt.hip.h on y.c0 = 0.
// A bad point's output is all-zero words.  A point that rule 1 or 2 stops runs the square root on the stand-in x (the generator's),
// as a malformed proof steps the generator in the verifier: every lane of a wave executes the same instructions, nothing is saved
// by leaving, and the neighbours in the wave see nothing of it.  The square root itself has no data-dependent control flow
// (fp_sqrt.hip.h), so a non-square costs what a square costs and cannot hang its wave; its closing r^2 == rhs IS the curve check.
#pragma once
#include "pairing_kernels.hip.h"
#include "fp_sqrt.hip.h"

namespace mnt753 {

#if defined(__HIPCC__)
// the report record: as SubgroupReport (pairing_kernels.hip.h), key = index << 3 | reason, all ones = good
using CompressReport = SubgroupReport;

// the coefficient b (G1) / b' (twist), this lane's share
template <class C>
__device__ __forceinline__ void compress_curve_b(typename C::F::E& r) {
  using F = typename C::F;
  constexpr int curve = F::MOD == MOD_B ? CURVE_MNT4753 : CURVE_MNT6753;
  if constexpr (F::DEG == 1) {
    fp_const_limbs(r, CURVE_B[curve].g1);
  } else if constexpr (F::LANES == 1) {
#pragma unroll
    for (int k = 0; k < F::DEG; ++k) fp_const_limbs(F::comp(r, k), CURVE_B[curve].g2[k]);
  } else {
    const int comp = tw_lane_comp<F>();
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      uint32_t v = CURVE_B[curve].g2[0][i];
      if (comp == 1) v = CURVE_B[curve].g2[1][i];
      if (comp == 2) v = CURVE_B[curve].g2[2][i];
      r.l[i] = v;
    }
  }
}

// affine[t] (2 Wx words at stride a_stride) -> x[t] (Wx words at x_stride), flags[t * f_stride].  Validates nothing.
template <class C>
__global__ void __launch_bounds__(256) k_compress(const uint32_t* __restrict__ affine, size_t a_stride, uint32_t* __restrict__ x, size_t x_stride,
                                                  uint8_t* __restrict__ flags, size_t f_stride, uint32_t n) {
  using F = typename C::F;
  constexpr int M = F::MOD;
  constexpr int WX = wire_coord_words<C>();
  const uint32_t t = logical_lane<F>();
  if (t == 0xffffffffu || t >= n) return;          // (all lanes of a group leave together)
  const uint32_t* src = affine + (size_t)t * a_stride;
  const uint32_t comp = lane_comp<F>();
  const bool ident = wire_y_is_zero<F>(src + WX);
  uint32_t w[24];
  load_wire24(w, src + 24 * comp);
  if (ident) {
#pragma unroll
    for (int i = 0; i < 24; ++i) w[i] = 0u;
  }
  store_wire24(x + (size_t)t * x_stride + 24 * comp, w);
  if (comp == 0) {
    uint32_t yi[24];
    load_wire24(w, src + WX);                      // y.c0
    fp_wire_to_integer<M>(yi, w);
    flags[(size_t)t * f_stride] = ident ? (uint8_t)2 : (uint8_t)(yi[0] & 1u);
  }
}

template <class C>
__global__ void __launch_bounds__(256, 1) k_decompress(const uint32_t* __restrict__ x, size_t x_stride, const uint8_t* __restrict__ flags, size_t f_stride,
                                                       const uint32_t* __restrict__ stand_x, uint32_t* __restrict__ out, size_t out_stride, uint32_t n,
                                                       unsigned long long base, CompressReport* __restrict__ rec) {
  using F = typename C::F;
  using E = typename F::E;
  using S = Sqrt<F>;
  constexpr int M = F::MOD;
  constexpr int WX = wire_coord_words<C>();
  const uint32_t t = logical_lane<F>();
  if (t == 0xffffffffu || t >= n) return;          // (all lanes of a group leave together)
  const uint32_t comp = lane_comp<F>();
  const uint32_t* px = x + (size_t)t * x_stride;
  const uint32_t flag = flags[(size_t)t * f_stride];
  const bool noncanon = (flag & 0xfcu) != 0u || !group_all<F>(!wire_noncanonical<M>(px + 24 * comp));
  const bool ident = (flag & 2u) != 0u;
  const uint32_t* src = (noncanon || ident) ? stand_x : px;
  E X, xx, rhs, ax, cb, y;
  wire_load<F>(X, src);
  S::sqr(xx, X);
  S::mul(rhs, xx, X);
  C::mul_by_a(ax, X);
  compress_curve_b<C>(cb);
  F::add(rhs, rhs, ax);
  F::add(rhs, rhs, cb);
  const bool rhs_zero = F::is_zero(rhs);
  bool square = false;
  S::sqrt(y, square, rhs);
  sqrt_fix_sign<F>(y, flag & 1u);
  uint32_t reason = 0;                             // MNT753_BAD_NONE
  if (noncanon) reason = 1;                        // MNT753_BAD_NONCANONICAL
  else if (!ident && (!square || rhs_zero)) reason = 2;   // MNT753_BAD_OFF_CURVE
  const bool good = reason == 0 && !ident;
  uint32_t wx[24], wy[24];
  load_wire24(wx, src + 24 * comp);
  fp_to_wire(wy, y);
  if (!good) {
#pragma unroll
    for (int i = 0; i < 24; ++i) { wx[i] = 0u; wy[i] = 0u; }
  }
  uint32_t* dst = out + (size_t)t * out_stride;
  store_wire24(dst + 24 * comp, wx);
  store_wire24(dst + WX + 24 * comp, wy);
  const bool bad = comp == 0 && reason != 0;
  const unsigned long long mask = __ballot(bad);
  if (mask && (int)(threadIdx.x & 63u) == __ffsll(mask) - 1) {
    atomicAdd(&rec->n_bad, (unsigned long long)__popcll(mask));
    atomicMin(&rec->key, ((base + t) << 3) | reason);
  }
}

// sqrt on raw field elements (test hook): in / out n elements in wire form, is_square n bytes; the lane mapping of k_decompress
template <class F, int W>
__global__ void __launch_bounds__(256, 1) k_field_sqrt(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint8_t* __restrict__ is_square, uint32_t n) {
  using E = typename F::E;
  const uint32_t t = logical_lane<F>();
  if (t == 0xffffffffu || t >= n) return;
  E a, r;
  wire_load<F>(a, in + (size_t)t * 24 * F::DEG);
  bool square = false;
  Sqrt<F>::template sqrt<W>(r, square, a);
  if (!square) F::zero(r);
  wire_store<F>(out + (size_t)t * 24 * F::DEG, r);
  if (lane_comp<F>() == 0) is_square[t] = square ? 1 : 0;
}
#endif  // __HIPCC__

}  // namespace mnt753
