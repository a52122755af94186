// Folded Groth16 verification: n proofs, one final exponentiation.
//
// With coefficients 0 < rho_i < 2^128 the batch (A_i, B_i, C_i), x_i is accepted iff
//     FE( prod_i ML(rho_i A_i, B_i) * ML(-S, G2::one()) * ML(-T, delta) ) == e(alpha, beta)^rho,
//     T = sum rho_i C_i,  rho = sum rho_i,  S = rho ABC[0] + sum_j (sum_i rho_i x_ij) ABC[j + 1].
// The kernels, in the order of a chunk of the batch:
//   k_fold_scale       one lane per proof on the point VM: the checks of A and C, U_i = rho_i A_i (affine wire form) and rho_i C_i
//                      (projective), two 128-bit double-and-add ladders through one instance of the VM
//   k_fold_point_sum   the sum of the rho_i C_i: a strided run per lane, then a tree over the lanes of a workgroup; a second launch
//                      of one workgroup sums the workgroups' results and the sum carried over from the chunks before
//   k_fold_miller      one lane group (2 / 3 lanes) per proof: the checks of B, the Miller loop of the ONE stepped pair (U_i, B_i)
//                      with the subgroup test of B on its running point, the status byte, and the product of the workgroup's
//                      Miller values through LDS -- one partial product per workgroup
//   k_fold_reduce      one workgroup: the product of the partial products and of the product carried over
// and once per call, on one lane group, k_fold_tail: the two stored pairs of the key, the final exponentiation, the power of
// e(alpha, beta) and the comparison.  F and tower operations are the out-of-line ones of tower753.hip.h / pairing_kernels.hip.h: no
// kernel here holds a second instance of a multiplier.
#pragma once
#include "pairing_kernels.hip.h"

namespace mnt753 {
#if defined(__HIPCC__)

// the exponent of e(alpha, beta): rho = sum rho_i < 2^128 n <= 2^152 (a batch has at most 2^24 proofs)
struct FoldExp {
  uint32_t w[8];
};

// ---- G1 side ------------------------------------------------------------------------------------------------------------------------
// P == Q as points (both not the identity): X1 Z2 == X2 Z1 and Y1 Z2 == Y2 Z1, four products through one instance of the multiplier
template <class C1>
__device__ __attribute__((noinline)) bool g1_same_point(const Proj<C1>& P, const Proj<C1>& Q) {
  using B = Fp<C1::F::MOD>;
  B a, b, r, keep, d;
  bool same = true;
#pragma nounroll
  for (int step = 0; step < 4; ++step) {
    switch (step) {
      case 0: a = P.X; b = Q.Z; break;
      case 1: a = Q.X; b = P.Z; break;
      case 2: a = P.Y; b = Q.Z; break;
      default: a = Q.Y; b = P.Z; break;
    }
    fp_mul(r, a, b);
    if (step & 1) {
      fp_sub(d, keep, r);
      same = same && fp_is_zero(d);
    } else {
      keep = r;
    }
  }
  return same;
}
// acc += Q for any two points: the identities are resolved first (add_pc), equal points double (proofs of a batch may repeat, and
// the VM's addition is not the doubling); P + -P leaves Z = 0, which is the identity to every reader
template <class C1>
__device__ __attribute__((noinline)) void g1_sum_step(Proj<C1>& acc, const Proj<C1>& Q) {
  int pc = add_pc<C1>(acc, Q);
  if (pc == PC_ADD && g1_same_point<C1>(acc, Q)) pc = PC_DBL;
  pt_vm<C1, true>(acc, Q, pc);
}

// Per proof t < n (one lane each): bad[t] |= 1 where A or C is malformed -- a non-canonical coordinate, the identity, a point off
// the curve (bad[t] on entry: an input of the proof is >= r, k_inputs_to_integer) -- then u_out[t] = rho_t A_t in affine wire form and
// c_out[t] = rho_t C_t projective, in storage form.  rho_t: the 128 bits coef[4 t .. 4 t + 3], not zero (the host has checked).  A
// joint schedule as in k_vk_accumulate: per bit one doubling and, if the bit is set, one mixed addition, through ONE instance of the
// VM for both ladders.  rho_t < 2^128 < r and A, C have order r (G1 has cofactor 1), so no step meets the identity or acc = +-Q
// after the first set bit.  A malformed proof steps the stand-in (the generator) and contributes the identity to the sum.
template <class C1>
__global__ void __launch_bounds__(256, 1) k_fold_scale(const uint32_t* __restrict__ proofs, uint32_t proof_words, const uint32_t* __restrict__ coef,
                                                      const uint32_t* __restrict__ stand1, uint8_t* __restrict__ bad, uint32_t* __restrict__ u_out,
                                                      uint32_t* __restrict__ c_out, uint32_t n) {
  using F = typename C1::F;
  constexpr int M = F::MOD;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t* pa = proofs + (size_t)t * proof_words;
  const uint32_t* pc_ = pa + proof_words - 48;
  bool malformed = bad[t] != 0;
  malformed |= wire_noncanonical<M>(pa) || wire_noncanonical<M>(pa + 24) || wire_noncanonical<M>(pc_) || wire_noncanonical<M>(pc_ + 24);
  malformed |= wire_y_is_zero<F>(pa + 24) || wire_y_is_zero<F>(pc_ + 24);
  Fp<M> ax, ay, cx, cy;
  wire_load<F>(ax, pa); wire_load<F>(ay, pa + 24);
  wire_load<F>(cx, pc_); wire_load<F>(cy, pc_ + 24);
  if (!malformed) malformed = !(g1_on_curve<C1>(ax, ay) && g1_on_curve<C1>(cx, cy));
  if (malformed) {
    wire_load<F>(ax, stand1); wire_load<F>(ay, stand1 + 24);
    cx = ax; cy = ay;
  }
  bad[t] = malformed ? 1 : 0;
  Proj<C1> acc, Q;
  F::one(Q.Z);
#pragma unroll 1
  for (int which = 0; which < 2; ++which) {
    Q.X = which ? cx : ax;
    Q.Y = which ? cy : ay;
    pt_set_zero(acc);
#pragma unroll 1
    for (uint32_t s = 0; s < 256u; ++s) {
      const uint32_t bit = 127u - (s >> 1);
      int pc = PC_END;
      if ((s & 1u) == 0u) {
        if (!pt_is_zero(acc)) pc = PC_DBL;
      } else if ((coef[(size_t)t * 4 + (bit >> 5)] >> (bit & 31u)) & 1u) {
        if (pt_is_zero(acc)) { acc.X = Q.X; acc.Y = Q.Y; F::one(acc.Z); }
        else pc = PC_MADD;
      }
      pt_vm<C1, false>(acc, Q, pc);
    }
    if (which == 0) {
      typename F::E zi, x, y;
      uint32_t wx[24], wy[24];
      F::inv(zi, acc.Z);
      F::mul(x, acc.X, zi);
      F::mul(y, acc.Y, zi);
      fp_to_wire(wx, x);
      fp_to_wire(wy, y);
      store_wire24(u_out + (size_t)t * 48, wx);
      store_wire24(u_out + (size_t)t * 48 + 24, wy);
    } else {
      if (malformed) pt_set_zero(acc);
      proj_store<C1>(c_out + (size_t)t * proj_words<C1>(), acc);
    }
  }
}

// out[b] = the sum of the points pts[i], i < n, i = (b, lane) mod (blocks, 256), and in a launch of ONE workgroup out[0] = that sum
// plus *carry where carry is given (out may be carry).  IN PLACE: lane k of the grid keeps its running sum in pts[k], which no
// other lane reads in the strided run; the tree over the workgroup's lanes then halves 256 slots in eight steps.  n >= 1.
template <class C1>
__global__ void __launch_bounds__(256, 1) k_fold_point_sum(uint32_t* __restrict__ pts, uint32_t n, const uint32_t* carry, uint32_t* out) {
  constexpr int PW = proj_words<C1>();
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  Proj<C1> acc, Q;
  if (k < n) {
    proj_load<C1>(acc, pts + (size_t)k * PW);
    for (uint32_t i = k + stride; i < n; i += stride) {
      proj_load<C1>(Q, pts + (size_t)i * PW);
      g1_sum_step<C1>(acc, Q);
    }
    proj_store<C1>(pts + (size_t)k * PW, acc);
  }
  __threadfence_block();
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = 128u; s > 0u; s >>= 1) {
    if (threadIdx.x < s && k + s < n) {
      proj_load<C1>(acc, pts + (size_t)k * PW);
      proj_load<C1>(Q, pts + (size_t)(k + s) * PW);
      g1_sum_step<C1>(acc, Q);
      proj_store<C1>(pts + (size_t)k * PW, acc);
    }
    __threadfence_block();
    __syncthreads();
  }
  if (threadIdx.x == 0 && k < n) {
    proj_load<C1>(acc, pts + (size_t)k * PW);
    if (carry) {
      proj_load<C1>(Q, carry);
      g1_sum_step<C1>(acc, Q);
    }
    proj_store<C1>(out + (size_t)blockIdx.x * PW, acc);
  }
}

// one projective point in storage form -> affine wire words, the identity as zero words (one lane)
template <class C1>
__global__ void __launch_bounds__(256, 1) k_fold_point_affine(const uint32_t* __restrict__ pt, uint32_t* __restrict__ out) {
  using F = typename C1::F;
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  Proj<C1> P;
  proj_load<C1>(P, pt);
  uint32_t wx[24], wy[24];
  if (pt_is_zero(P)) {
#pragma unroll
    for (int i = 0; i < 24; ++i) wx[i] = wy[i] = 0u;
  } else {
    typename F::E zi, x, y;
    F::inv(zi, P.Z);
    F::mul(x, P.X, zi);
    F::mul(y, P.Y, zi);
    fp_to_wire(wx, x);
    fp_to_wire(wy, y);
  }
  store_wire24(out, wx);
  store_wire24(out + 24, wy);
}

// ---- the lane groups of a workgroup --------------------------------------------------------------------------------------------------
// 256 threads hold 128 groups of two lanes (MNT4753) or 84 of three (MNT6753: 21 per wave, lane 63 of every wave belongs to none).
// Group g of workgroup b is logical lane b GROUPS + g (logical_lane).
template <class F>
struct FoldGroups {
  static_assert(F::LANES == 2 || F::LANES == 3, "the fold runs on the lane-split fields");
  static constexpr int GROUPS = F::LANES == 3 ? 84 : 128;
  static constexpr int TW = 2 * F::DEG * FPS_WORDS;                // storage words of a tower element
  static constexpr int LDS_WORDS = 64 * F::LANES * 2 * FPS_WORDS;  // the upper half of a tree step: at most 64 groups write
  static __device__ __forceinline__ bool lane_used() { return F::LANES == 2 || (threadIdx.x & 63u) != 63u; }
  static __device__ __forceinline__ int group() {
    if constexpr (F::LANES == 2) return (int)(threadIdx.x >> 1);
    else return (int)((threadIdx.x >> 6) * 21u + (threadIdx.x & 63u) / 3u);
  }
};
template <class F>
__device__ __forceinline__ void tower_load(typename Tower<F>::E& f, const uint32_t* p) {
  e_load<F>(f.c0, p);
  e_load<F>(f.c1, p + F::DEG * FPS_WORDS);
}
template <class F>
__device__ __forceinline__ void tower_store(uint32_t* p, const typename Tower<F>::E& f) {
  e_store<F>(p, f.c0);
  e_store<F>(p + F::DEG * FPS_WORDS, f.c1);
}
// The product of the tower elements f of the groups g < cnt of this workgroup (1 <= cnt <= GROUPS), left in group 0.  Seven halving
// steps: the groups [s, 2 s) below cnt write their element to LDS -- every lane its own component of both halves, so the reader's
// lanes find theirs at the same place -- and group g < s with g + s < cnt multiplies the element of group g + s into its own.  Every
// thread of the workgroup calls this (`used` false for the lanes that belong to no group); the products run with whole groups
// switched off, which the cross-lane exchange of the fields allows: a lane only ever fetches from lanes of its own group.
template <class C>
__device__ __forceinline__ void fold_workgroup_product(typename Tower<typename C::F>::E& f, bool used, int g, int cnt, uint32_t* lds) {
  using F = typename C::F;
  using T = Tower<F>;
  const int comp = (int)lane_comp<F>();
#pragma unroll 1
  for (int s = 64; s > 0; s >>= 1) {
    if (used && g >= s && g < 2 * s && g < cnt) {
      uint32_t* dst = lds + (size_t)(((g - s) * F::LANES + comp) * 2) * FPS_WORDS;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        dst[i] = f.c0.l[i];
        dst[FPS_WORDS + i] = f.c1.l[i];
      }
    }
    __syncthreads();
    if (used && g < s && g + s < cnt) {
      typename T::E o;
      const uint32_t* src = lds + (size_t)((g * F::LANES + comp) * 2) * FPS_WORDS;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        o.c0.l[i] = src[i];
        o.c1.l[i] = src[FPS_WORDS + i];
      }
      T::mul(f, f, o);
    }
    __syncthreads();
  }
}

// The Miller loop of ONE stepped pair with the subgroup test of its G2 point on the running point (miller_loop_verify's SUB path
// without the stored pairs): f = ML(P, Q) as Ate<C>::miller_loop<1> gives it, and whether Q lies in G2.
template <class C>
__device__ __forceinline__ bool miller_loop_fold(typename Tower<typename C::F>::E& f, typename Ate<C>::Pair& p) {
  using A = Ate<C>;
  using T = Tower<typename C::F>;
  bool member;
  T::one(f);
#pragma unroll 1
  for (int i = PAIRC[A::CURVE].loop_bits - 2; i >= 0; --i) {
    const bool bit = (PAIRC[A::CURVE].loop_count[i >> 5] >> (i & 31)) & 1u;
    T::sqr(f, f);
    A::line_dbl(f, p);
    if (bit) A::line_add(f, p, p.qx, p.qy, p.qy2);
  }
  typename A::FE sx, sy;
  A::endo(sx, sy, p.qx, p.qy);
  if (PAIRC[A::CURVE].loop_neg) {
    typename A::FE mx, my, my2;
    A::minus_r_affine(mx, my, my2, p.R);
    member = A::affine_equals(p.R.Z, mx, my, sx, sy);
    A::line_add(f, p, mx, my, my2);              // line_close, with -R affine in hand
    T::inv(f, f);
  } else {
    member = A::run_equals(p.R, sx, sy);
  }
  return member;
}

// Per proof t < n (one lane group each): status[t] = 1 (malformed: bad[t] from k_fold_scale, or B with a non-canonical component,
// the identity, off the twist), 3 (B on the twist and not in G2) or 0, and the proof's factor ML(U_t, B_t) -- ONE for a proof with a
// status, which steps the generators so that its neighbours in the wave see nothing of it.  partials[b] = the product of the
// factors of workgroup b, in storage form.  u: k_fold_scale's rho_t A_t.  key: as for k_groth16_verify.
template <class C, class C1>
__global__ void __launch_bounds__(256, 1) k_fold_miller(const uint32_t* __restrict__ proofs, const uint32_t* __restrict__ u, const uint32_t* __restrict__ key,
                                                       const uint8_t* __restrict__ bad, uint8_t* __restrict__ status, uint32_t* __restrict__ partials, uint32_t n) {
  using A = Ate<C>;
  using F = typename C::F;
  using F1 = FieldFp<F::MOD>;
  using G = FoldGroups<F>;
  constexpr int M = F::MOD;
  constexpr int W2 = wire_coord_words<C>();
  __shared__ __attribute__((aligned(16))) uint32_t lds[G::LDS_WORDS];
  const bool used = G::lane_used();
  const int g = G::group();
  const uint32_t first = blockIdx.x * (uint32_t)G::GROUPS;           // (the host launches no workgroup without a proof)
  const int cnt = n - first < (uint32_t)G::GROUPS ? (int)(n - first) : G::GROUPS;
  typename A::TE f;
  if (used && g < cnt) {
    const uint32_t t = first + (uint32_t)g;
    const uint32_t* pb = proofs + (size_t)t * (96 + 2 * W2) + 48;
    const uint32_t *stand1 = key, *gen2 = key + 48;
    bool malformed = bad[t] != 0;
    {
      const int comp = (int)lane_comp<F>();
      const bool nc = wire_noncanonical<M>(pb + 24 * comp) || wire_noncanonical<M>(pb + W2 + 24 * comp);
      malformed |= !group_all<F>(!nc);
    }
    malformed |= wire_y_is_zero<F>(pb + W2);
    typename A::B ux, uy;
    typename A::FE bx, by;
    wire_load<F>(bx, pb); wire_load<F>(by, pb + W2);
    if (!malformed) malformed = !g2_on_curve<C>(bx, by);
    if (malformed) {
      wire_load<F1>(ux, stand1); wire_load<F1>(uy, stand1 + 24);
      wire_load<F>(bx, gen2); wire_load<F>(by, gen2 + W2);
    } else {
      wire_load<F1>(ux, u + (size_t)t * 48); wire_load<F1>(uy, u + (size_t)t * 48 + 24);
    }
    typename A::Pair p;
    A::setup(p, ux, uy, bx, by);
    const bool member = miller_loop_fold<C>(f, p);
    const uint8_t st = malformed ? 1 : (!member ? 3 : 0);
    if (st) A::T::one(f);
    if (lane_comp<F>() == 0) status[t] = st;
  }
  fold_workgroup_product<C>(f, used, g, cnt, lds);
  if (used && g == 0) tower_store<F>(partials + (size_t)blockIdx.x * G::TW, f);
}

// *acc = the product of partials[0 .. m) and, unless `first`, of *acc: ONE workgroup; group g multiplies the elements g, g + GROUPS,
// .., then the tree of fold_workgroup_product.  m >= 1.
template <class C>
__global__ void __launch_bounds__(256, 1) k_fold_reduce(const uint32_t* __restrict__ partials, uint32_t m, uint32_t* acc, int first) {
  using F = typename C::F;
  using T = Tower<F>;
  using G = FoldGroups<F>;
  __shared__ __attribute__((aligned(16))) uint32_t lds[G::LDS_WORDS];
  const bool used = G::lane_used();
  const int g = G::group();
  const uint32_t total = m + (first ? 0u : 1u);                      // element m: the product carried over
  const int cnt = total < (uint32_t)G::GROUPS ? (int)total : G::GROUPS;
  typename T::E f;
  if (used && g < cnt) {
    tower_load<F>(f, (uint32_t)g < m ? partials + (size_t)g * G::TW : acc);
#pragma unroll 1
    for (uint32_t i = (uint32_t)g + (uint32_t)G::GROUPS; i < total; i += (uint32_t)G::GROUPS) {
      typename T::E o;
      tower_load<F>(o, i < m ? partials + (size_t)i * G::TW : acc);
      T::mul(f, f, o);
    }
  }
  fold_workgroup_product<C>(f, used, g, cnt, lds);                   // (its barriers stand between the reads of *acc and the write)
  if (used && g == 0) tower_store<F>(acc, f);
}

// a tower element in storage form -> wire words c0 | c1 (lane group 0 of one workgroup)
template <class C>
__global__ void __launch_bounds__(256, 1) k_fold_export(const uint32_t* __restrict__ acc, uint32_t* __restrict__ out_wire) {
  using F = typename C::F;
  if (logical_lane<F>() != 0u) return;
  typename Tower<F>::E f;
  tower_load<F>(f, acc);
  wire_store<F>(out_wire, f.c0);
  wire_store<F>(out_wire + wire_coord_words<C>(), f.c1);
}

// The tail of a call, on lane group 0 of one workgroup: *accepted = FE(F ML(-S, G2::one()) ML(-T, delta)) == e(alpha, beta)^rho.
// facc: F in storage form.  s_wire, t_wire: S and T, affine wire form; the identity (zero words) pairs to one, its lines are left
// out.  Both pairs read the key's stored coefficients (coeffs: of G2::one(), then of delta, as for k_groth16_verify) and share the
// squaring.  rho > 0 of `bits` bits.
template <class C, class C1>
__global__ void __launch_bounds__(256, 1) k_fold_tail(const uint32_t* __restrict__ facc, const uint32_t* __restrict__ s_wire, const uint32_t* __restrict__ t_wire,
                                                     const uint32_t* __restrict__ key, const uint32_t* __restrict__ coeffs, FoldExp rho, int bits,
                                                     uint32_t* __restrict__ accepted) {
  using A = Ate<C>;
  using F = typename C::F;
  using F1 = FieldFp<F::MOD>;
  using T = Tower<F>;
  constexpr int W2 = wire_coord_words<C>();
  if (logical_lane<F>() != 0u) return;
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
  tower_load<F>(r, facc);
  T::mul(f, f, r);
  A::final_exponentiation(r, f);
  // wire_load keeps 756 bits of a component and reduces what it keeps: a stored e(alpha, beta) that is not canonical would be compared
  // as another element's words, so it accepts nothing (k_groth16_verify compares the words themselves)
  bool nc = false;
  if constexpr (F::LANES == 1) {
    for (int k = 0; k < 2 * F::DEG; ++k) nc |= wire_noncanonical<F::MOD>(gt + 24 * k);
  } else {
    const int comp = (int)lane_comp<F>();
    nc = wire_noncanonical<F::MOD>(gt + 24 * comp) || wire_noncanonical<F::MOD>(gt + W2 + 24 * comp);
  }
  const bool canonical = group_all<F>(!nc);
  wire_load<F>(f.c0, gt); wire_load<F>(f.c1, gt + W2);
  T::pow(want, f, rho.w, bits);
  const bool same = A::f_equal(r.c0, want.c0) && A::f_equal(r.c1, want.c1) && canonical;
  if (lane_comp<F>() == 0) *accepted = same ? 1u : 0u;
}
#endif  // __HIPCC__

}  // namespace mnt753
