// Folded Groth16 verification with one tail per segment: the fold's equation (fold_kernels.hip.h) on every
// run of FoldGroups::GROUPS proofs, so that a rejected batch names the segments that hold a wrong proof.
//
// k_fold_scale and k_fold_miller run unchanged: a chunk starts on a segment boundary, so partials[b] of k_fold_miller is F_b of
// segment b.  The kernels here -- the first two per chunk, the last two once per call over all its segments:
//   k_fold_segment_point_sum   one workgroup per segment: T_s = sum rho_i C_i through the halving tree of k_fold_point_sum, then the
//                              affine wire form (one inversion per segment)
//   k_fold_segment_dots        one lane per (segment, scalar): rho_s as handed in, c_{j,s} = sum_i rho_i x_ij in Fr, as integers
//   k_fold_segment_s           one lane per segment (a key that is not prepared): S_s = rho_s ABC[0] + sum_j c_{j,s} ABC[j + 1], the joint
//                              ladder of k_vk_accumulate over num_inputs + 1 scalars
//   k_fold_segment_tail        one lane group per segment: k_fold_tail's body on (F_s, S_s, T_s, rho_s)
// F and tower operations are the out-of-line ones: no kernel here holds a second instance of a multiplier.
#pragma once
#include "fold_kernels.hip.h"
#include "reduce_kernels.hip.h"

namespace mnt753 {
#if defined(__HIPCC__)

// Workgroup b: out_wire[b] = the sum of pts[b seg + k], k < min(seg, n - b seg), in affine wire form (the identity: zero words).
// IN PLACE as k_fold_point_sum: lane k keeps its running sum in its own point.  seg <= 256; the host launches no workgroup without
// a proof.
template <class C1>
__global__ void __launch_bounds__(256, 1) k_fold_segment_point_sum(uint32_t* __restrict__ pts, uint32_t n, uint32_t seg, uint32_t* __restrict__ out_wire) {
  using F = typename C1::F;
  constexpr int PW = proj_words<C1>();
  const uint32_t first = blockIdx.x * seg;
  const uint32_t cnt = n - first < seg ? n - first : seg;
  uint32_t* mine = pts + (size_t)(first + threadIdx.x) * PW;
  Proj<C1> acc, Q;
#pragma unroll 1
  for (uint32_t s = 128u; s > 0u; s >>= 1) {
    if (threadIdx.x < s && threadIdx.x + s < cnt) {
      proj_load<C1>(acc, mine);
      proj_load<C1>(Q, mine + (size_t)s * PW);
      g1_sum_step<C1>(acc, Q);
      proj_store<C1>(mine, acc);
    }
    __threadfence_block();
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  proj_load<C1>(acc, mine);
  uint32_t wx[24], wy[24];
  if (pt_is_zero(acc)) {
#pragma unroll
    for (int i = 0; i < 24; ++i) wx[i] = wy[i] = 0u;
  } else {
    typename F::E zi, x, y;
    F::inv(zi, acc.Z);
    F::mul(x, acc.X, zi);
    F::mul(y, acc.Y, zi);
    fp_to_wire(wx, x);
    fp_to_wire(wy, y);
  }
  store_wire24(out_wire + (size_t)blockIdx.x * 48, wx);
  store_wire24(out_wire + (size_t)blockIdx.x * 48 + 24, wy);
}

// Lane (s, jj), s < segments, jj <= k: ints[s (k + 1) + jj] = the integer of scalar jj of segment s -- jj == 0: rho_s (rho_ints[s], an
// integer already), jj >= 1: c_{jj-1,s} = sum_i rho[i] x[i k + jj - 1] over the segment's proofs i in Fr (rho, x: wire form; the sum
// as k_vk_input_dots forms it, then red_finish and the integer).  A segment is at most 256 proofs: one lane runs its sum.
template <int M>
__global__ void __launch_bounds__(256) k_fold_segment_dots(const uint32_t* __restrict__ rho, const uint32_t* __restrict__ x, const uint32_t* __restrict__ rho_ints,
                                                          uint32_t n, uint32_t k, uint32_t seg, uint32_t segments, uint32_t* __restrict__ ints) {
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t s = lane / (k + 1u), jj = lane % (k + 1u);
  if (s >= segments) return;
  uint32_t w[24], out[24];
  if (jj == 0u) {
    load_wire24(out, rho_ints + (size_t)s * 24);
  } else {
    const uint32_t first = s * seg, last = n - first < seg ? n : first + seg;
    Fp<M> acc;
    fp_zero(acc);
    uint32_t pending = 0;
#pragma unroll 1
    for (uint32_t i = first; i < last; ++i) {
      Fp<M> y;
      load_wire24(w, rho + (size_t)i * 24);
      fp_unpack(y, w);
      dot_term<M>(acc, pending, x + ((size_t)i * k + (jj - 1u)) * 24, y);
    }
    red_flush(acc, pending);
    red_finish(w, acc);
    fp_wire_to_integer<M>(out, w);
  }
  store_wire24(ints + (size_t)lane * 24, out);
}

// out[s] = sum_{jj < scalars} ints[s scalars + jj] ABC[jj] for s < segments, affine wire form (the identity: zero words), one lane per
// segment: k_vk_accumulate's joint double-and-add with ABC[0] as one more scaled base instead of the summand of its last step.
// The doubling of a bit is the VM's doubling; an addition is g1_sum_step's, spelled out so that the kernel holds ONE instance of the
// VM: two ABC points of a key may be equal (or meet the running sum), and the VM's addition is not the doubling.  bits: the scalars
// are below 2^bits.
template <class C1>
__global__ void __launch_bounds__(256, 1) k_fold_segment_s(const uint32_t* __restrict__ abc, const uint32_t* __restrict__ ints, uint32_t* __restrict__ out,
                                                          uint32_t segments, uint32_t scalars, uint32_t bits) {
  using F = typename C1::F;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= segments) return;
  Proj<C1> acc, Q;
  pt_set_zero(acc);
  F::zero(Q.X); F::zero(Q.Y); F::one(Q.Z);
  const uint32_t per_bit = scalars + 1u;
  const uint32_t steps = bits * per_bit;
#pragma unroll 1
  for (uint32_t s = 0; s < steps; ++s) {
    const uint32_t bit = bits - 1u - s / per_bit, j = s % per_bit;   // j == 0: the doubling of this bit; j >= 1: scalar j - 1
    int pc = PC_END;
    if (j == 0u) {
      if (!pt_is_zero(acc)) pc = PC_DBL;
    } else if ((ints[((size_t)t * scalars + (j - 1u)) * 24 + (bit >> 5)] >> (bit & 31u)) & 1u) {
      const uint32_t* src = abc + (size_t)(j - 1u) * 48;
      uint32_t w[24];
      load_wire24(w, src); fp_from_wire(Q.X, w);
      load_wire24(w, src + 24); fp_from_wire(Q.Y, w);
      pc = add_pc<C1>(acc, Q);                                       // (Q is never the identity; an empty acc takes it over)
      if (pc == PC_ADD && g1_same_point<C1>(acc, Q)) pc = PC_DBL;
    }
    pt_vm<C1, true>(acc, Q, pc);
  }
  uint32_t* dst = out + (size_t)t * 48;
  uint32_t wx[24], wy[24];
  if (pt_is_zero(acc)) {
#pragma unroll
    for (int i = 0; i < 24; ++i) wx[i] = wy[i] = 0u;
  } else {
    typename F::E zi, x, y;
    F::inv(zi, acc.Z);
    F::mul(x, acc.X, zi);
    F::mul(y, acc.Y, zi);
    fp_to_wire(wx, x);
    fp_to_wire(wy, y);
  }
  store_wire24(dst, wx);
  store_wire24(dst + 24, wy);
}

// tower elements in storage form -> wire words c0 | c1, lane group t < m for element t
template <class C>
__global__ void __launch_bounds__(256, 1) k_fold_segment_export(const uint32_t* __restrict__ partials, uint32_t m, uint32_t* __restrict__ out_wire) {
  using F = typename C::F;
  using G = FoldGroups<F>;
  constexpr int W2 = wire_coord_words<C>();
  const uint32_t t = logical_lane<F>();
  if (t == 0xffffffffu || t >= m) return;
  typename Tower<F>::E f;
  tower_load<F>(f, partials + (size_t)t * G::TW);
  wire_store<F>(out_wire + (size_t)t * 2 * W2, f.c0);
  wire_store<F>(out_wire + (size_t)t * 2 * W2 + W2, f.c1);
}

// Lane group t < segments: accepted[t] = no proof of segment t has a status and FE(F_t ML(-S_t, G2::one()) ML(-T_t, delta)) ==
// e(alpha, beta)^rho_t -- k_fold_tail's body on element t of partials (storage form), s_wire, t_wire (48 words each) and rho.
// Lane groups of one wave run different segments, so every loop has the same trip count in all of them: the power runs over
// max_bits, the bit length of the largest rho_t of the launch, from ONE (leading zero bits square one), and a group multiplies where
// its own bit is set.  use_s, use_t and the bits are per-group predicates: whole groups are switched off, and a lane only fetches from
// lanes of its own group.  A segment with a flagged proof sits out as a whole group and is rejected: the per-proof verifier names its
// proofs.  status: k_fold_miller's bytes of the n proofs; seg proofs per segment.
template <class C, class C1>
__global__ void __launch_bounds__(256, 1) k_fold_segment_tail(const uint32_t* __restrict__ partials, const uint32_t* __restrict__ s_all, const uint32_t* __restrict__ t_all,
                                                             const uint32_t* __restrict__ key, const uint32_t* __restrict__ coeffs, const FoldExp* __restrict__ rho,
                                                             int max_bits, const uint8_t* __restrict__ status, uint32_t n, uint32_t seg, uint32_t segments,
                                                             uint32_t* __restrict__ accepted) {
  using A = Ate<C>;
  using F = typename C::F;
  using F1 = FieldFp<F::MOD>;
  using T = Tower<F>;
  using G = FoldGroups<F>;
  constexpr int W2 = wire_coord_words<C>();
  const uint32_t t = logical_lane<F>();
  if (t == 0xffffffffu || t >= segments) return;     // (all lanes of a group leave together)
  {
    const uint32_t first = t * seg, last = n - first < seg ? n : first + seg;
    bool flagged = false;
    for (uint32_t i = first; i < last; ++i) flagged |= status[i] != 0;
    if (flagged) {
      if (lane_comp<F>() == 0) accepted[t] = 0u;
      return;
    }
  }
  const uint32_t *s_wire = s_all + (size_t)t * 48, *t_wire = t_all + (size_t)t * 48;
  const uint32_t *stand1 = key, *gen2 = key + 48, *delta = gen2 + 2 * W2, *gt = delta + 2 * W2;
  const bool use_s = !wire_y_is_zero<F1>(s_wire + 24), use_t = !wire_y_is_zero<F1>(t_wire + 24);
  typename A::B sx, sy, tx, ty;
  wire_load<F1>(sx, use_s ? s_wire : stand1); wire_load<F1>(sy, (use_s ? s_wire : stand1) + 24);
  wire_load<F1>(tx, use_t ? t_wire : stand1); wire_load<F1>(ty, (use_t ? t_wire : stand1) + 24);
  fp_neg(sy, sy);
  fp_neg(ty, ty);
  StoredPair<C> s1, s2;
  typename A::FE qx, qy;
  wire_load<F>(qx, gen2); wire_load<F>(qy, gen2 + W2);
  stored_setup<C>(s1, sx, sy, qx, qy);
  wire_load<F>(qx, delta); wire_load<F>(qy, delta + W2);
  stored_setup<C>(s2, tx, ty, qx, qy);
  const uint32_t *c1 = coeffs, *c2 = coeffs + ate_coeff_words<C>();
  typename T::E f, r, want;
  T::one(f);
#pragma unroll 1
  for (int i = PAIRC[A::CURVE].loop_bits - 2; i >= 0; --i) {
    const bool bit = (PAIRC[A::CURVE].loop_count[i >> 5] >> (i & 31)) & 1u;
    T::sqr(f, f);
    if (use_s) stored_line_dbl<C>(f, s1, c1);
    if (use_t) stored_line_dbl<C>(f, s2, c2);
    if (bit) {
      if (use_s) stored_line_add<C>(f, s1, c1);
      if (use_t) stored_line_add<C>(f, s2, c2);
    }
  }
  if (PAIRC[A::CURVE].loop_neg) {
    if (use_s) stored_line_add<C>(f, s1, c1);
    if (use_t) stored_line_add<C>(f, s2, c2);
    T::inv(f, f);
  }
  tower_load<F>(r, partials + (size_t)t * G::TW);
  T::mul(f, f, r);
  A::final_exponentiation(r, f);
  // (a stored e(alpha, beta) that is not canonical accepts nothing, as in k_fold_tail)
  bool nc = false;
  if constexpr (F::LANES == 1) {
    for (int k = 0; k < 2 * F::DEG; ++k) nc |= wire_noncanonical<F::MOD>(gt + 24 * k);
  } else {
    const int comp = (int)lane_comp<F>();
    nc = wire_noncanonical<F::MOD>(gt + 24 * comp) || wire_noncanonical<F::MOD>(gt + W2 + 24 * comp);
  }
  const bool canonical = group_all<F>(!nc);
  wire_load<F>(f.c0, gt); wire_load<F>(f.c1, gt + W2);
  const uint32_t* e = rho[t].w;
  T::one(want);
#pragma unroll 1
  for (int i = max_bits - 1; i >= 0; --i) {
    T::sqr(want, want);
    if ((e[i >> 5] >> (i & 31)) & 1u) T::mul(want, want, f);
  }
  const bool same = A::f_equal(r.c0, want.c0) && A::f_equal(r.c1, want.c1) && canonical;
  if (lane_comp<F>() == 0) accepted[t] = same ? 1u : 0u;
}
#endif  // __HIPCC__

}  // namespace mnt753
