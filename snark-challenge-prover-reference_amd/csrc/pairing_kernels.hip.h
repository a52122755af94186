// The flipped ate pairing of MNT4753 / MNT6753 on the tower of tower753.hip.h.
//
// Replaces, for a batch, libff's mnt{4,6}753_ate_precompute_G2 / ate_miller_loop / final_exponentiation
// (depends/libff/libff/algebra/curves/mnt753/mnt4753/mnt4753_pairing.cpp:180-223, :405-593 and the same lines of mnt6753_pairing.cpp).
// Same formulas, so the same field elements:
//   dbl_step / add_step   doubling_step_for_flipped_miller_loop (:405-431), mixed_addition_step_for_flipped_miller_loop (:433-459) on
//                         R = (X, Y, Z, T = Z^2) over the twist;
//   miller_loop           f <- f^2 g_RR(P), and on a set bit of the loop count f <- f g_RQ(P) (:539-593), for K pairs that share
//                         the squaring (libff's double_miller_loop is K = 2); with a negative loop count (MNT4753) the closing step
//                         with -R made affine (:522-533) and the inversion of f (:582-588);
//   final_exponentiation  :213-223: the first chunk q^2 - 1 (MNT4753) or (q^3 - 1)(q + 1) (MNT6753) on f and on 1 / f, then
//                         Frobenius(1) of the first times the |w0| power of the one the sign of w0 names.
// The schedule is the device's.  libff stores the coefficients H, 4C, J, L / L1, RZ of every step of a G2 point (0.4 MB per point on
// MNT4753, 0.6 MB on MNT6753) and reads them back in the Miller loop.  For a point that comes with the call (the Q of a pairing, the B
// of a proof) every step's coefficients go into its line value at once and are never stored: no workspace whatever the batch.  For
// the points of a verification key that never change (G2::one(), delta_g2) they are stored ONCE, by k_g2_precompute into the key
// object, and every lane group of every proof reads them from there (k_groth16_verify): all lanes of a wave read the same step at
// the same time, one address per component.
//
// Everything above the kernels is __host__ __device__ and compiles with a host compiler through the one-lane fields
// (tools/host_pairing_check.cpp).  The kernels run one lane group per pairing on the lane-split fields: 2 lanes (MNT4753, 32 pairings
// per wave) or 3 lanes (MNT6753, 21 per wave, lane 63 idle).
#pragma once
#include "tower753.hip.h"
#if defined(__HIPCC__)
#include "msm_kernels.hip.h"
#endif

namespace mnt753 {

// C: a G2 configuration of curve753.hip.h (Mnt4G2 / Mnt6G2, or Mnt4G2S / Mnt6G2S on the device)
template <class C>
struct Ate {
  using F = typename C::F;
  using X = FX<F>;
  using FE = typename F::E;
  using B = Fp<F::MOD>;
  using T = Tower<F>;
  using TE = typename T::E;
  static constexpr int CURVE = X::CURVE;

  struct Run {
    FE X, Y, Z, T;
  };
  // one (P, Q) pair of a Miller loop: PX twist, PY twist, L1_coeff = PX - QX / twist, QY / twist, Q and the running point
  struct Pair {
    FE px_t, py_t, l1c, qyt, qx, qy, qy2;
    Run R;
  };

  static TW_FN void setup(Pair& p, const B& px, const B& py, const FE& qx, const FE& qy) {
    B ni;
    FE tinv, t;
    fp_const_limbs(ni, PAIRC[CURVE].nr_inv);
    X::embed(tinv, ni, F::DEG - 1);              // 1 / twist = u^(deg - 1) / NR
    X::embed(p.px_t, px, 1);                     // twist = u
    X::embed(p.py_t, py, 1);
    X::mul(t, qx, tinv);
    X::embed(p.l1c, px, 0);
    X::sub(p.l1c, p.l1c, t);
    X::mul(p.qyt, qy, tinv);
    p.qx = qx;
    p.qy = qy;
    X::sqr(p.qy2, qy);
    p.R.X = qx;
    p.R.Y = qy;
    X::one(p.R.Z);
    X::one(p.R.T);
  }

  static TW_FN void dbl_step(Run& R, FE& H, FE& C4, FE& J, FE& L) {
    FE A, Bq, Cq, D, E, Fv, G, t, u;
    X::sqr(A, R.T);
    X::sqr(Bq, R.X);
    X::sqr(Cq, R.Y);
    X::sqr(D, Cq);
    X::add(t, R.X, Cq); X::sqr(t, t); X::sub(t, t, Bq); X::sub(E, t, D);           // E = (X + C)^2 - B - D
    C::mul_by_a(t, A); X::dbl(u, Bq); X::add(u, u, Bq); X::add(Fv, u, t);          // F = 3 B + a' A
    X::sqr(G, Fv);
    X::add(t, Fv, R.T); X::sqr(t, t); X::sub(t, t, G); X::sub(J, t, A);            // J = (F + T)^2 - G - A
    X::add(t, Fv, R.X); X::sqr(t, t); X::sub(t, t, G); X::sub(L, t, Bq);           // L = (F + X)^2 - G - B
    X::dbl(E, E);                                                                  // 2 E
    X::dbl(t, E); X::sub(R.X, G, t);                                               // X3 = G - 4 E
    X::sub(t, E, R.X); X::mul(t, Fv, t);
    X::dbl(D, D); X::dbl(D, D); X::dbl(D, D);
    X::add(u, R.Y, R.Z);                                                           // (before Y changes)
    X::sub(R.Y, t, D);                                                             // Y3 = F (2 E - X3) - 8 D
    X::sqr(u, u); X::sub(u, u, Cq); X::sqr(t, R.Z); X::sub(R.Z, u, t);             // Z3 = (Y + Z)^2 - C - Z^2
    X::add(u, R.Z, R.T);                                                           // Z3 + T1
    X::sqr(R.T, R.Z);                                                              // T3
    X::sqr(u, u); X::sub(u, u, R.T); X::sub(H, u, A);                              // H = (Z3 + T1)^2 - T3 - A
    X::dbl(C4, Cq); X::dbl(C4, C4);
  }

  // RZ is R.Z afterwards
  static TW_FN void add_step(const FE& bx, const FE& by, const FE& by2, Run& R, FE& L1) {
    FE Bq, D, H, I, E, J, V, Y2, t;
    X::mul(Bq, bx, R.T);
    X::add(t, by, R.Z); X::sqr(t, t); X::sub(t, t, by2); X::sub(t, t, R.T); X::mul(D, t, R.T);
    X::sub(H, Bq, R.X);
    X::sqr(I, H);
    X::dbl(E, I); X::dbl(E, E);
    X::mul(J, H, E);
    X::mul(V, R.X, E);
    X::dbl(Y2, R.Y);
    X::sub(L1, D, Y2);
    X::sqr(t, L1); X::sub(t, t, J); X::sub(t, t, V); X::sub(R.X, t, V);            // X3 = L1^2 - J - 2 V
    X::sub(t, V, R.X); X::mul(t, L1, t); X::mul(J, Y2, J); X::sub(R.Y, t, J);      // Y3 = L1 (V - X3) - 2 Y1 J
    X::add(t, R.Z, H); X::sqr(t, t); X::sub(t, t, R.T); X::sub(R.Z, t, I);         // Z3 = (Z1 + H)^2 - T1 - I
    X::sqr(R.T, R.Z);
  }

  // f <- f g_RR(P) after R <- 2 R
  static TW_FN void line_dbl(TE& f, Pair& p) {
    FE H, C4, J, L, t;
    TE g;
    dbl_step(p.R, H, C4, J, L);
    X::mul(t, J, p.px_t);
    X::sub(t, L, t);
    X::sub(g.c0, t, C4);                         // -4C - J PX twist + L
    X::mul(g.c1, H, p.py_t);
    T::mul(f, f, g);
  }
  // f <- f g_RQ(P) after R <- R + (bx, by)
  static TW_FN void line_add(TE& f, Pair& p, const FE& bx, const FE& by, const FE& by2) {
    FE L1, t, u;
    TE g;
    add_step(bx, by, by2, p.R, L1);
    X::mul(g.c0, p.R.Z, p.py_t);
    X::mul(t, p.qyt, p.R.Z);
    X::mul(u, p.l1c, L1);
    X::add(t, t, u);
    X::neg(g.c1, t);
    T::mul(f, f, g);
  }
  // -R made affine, with its y squared: the base of the closing step of a negative loop count
  static TW_FN void minus_r_affine(FE& mx, FE& my, FE& my2, const Run& R) {
    FE zi, zi2, zi3;
    X::inv(zi, R.Z);
    X::sqr(zi2, zi);
    X::mul(zi3, zi2, zi);
    X::mul(mx, R.X, zi2);
    X::mul(my, R.Y, zi3);
    X::neg(my, my);
    X::sqr(my2, my);
  }
  // the closing step: R + (-R)
  static TW_FN void line_close(TE& f, Pair& p) {
    FE mx, my, my2;
    minus_r_affine(mx, my, my2, p.R);
    line_add(f, p, mx, my, my2);
  }

  // ---- subgroup membership on the twist ----------------------------------------------------------------
  // psi = twist^-1 o Frobenius_q o twist on E'(F): psi(x, y) = (x^q gamma_1^-2, y^q gamma_1^-3).  x^q in F is component c times
  // gamma_1^(2 c), the frob[1][2 c] the tower's Frobenius already uses; the two constants lie in Fq (tools/gen_constants.py asserts
  // it, and psi(G2::one()) = [q - r] G2::one(), which fixes the sign of the y constant).  The product by the constant is a product
  // of F with the embedded constant: no further instance of the multiplier.
  static TW_FN void endo(FE& sx, FE& sy, const FE& qx, const FE& qy) {
    B k;
    FE c, t;
    X::template frob_scale<1, 0>(t, qx);
    fp_const_limbs(k, PAIRC[CURVE].psi_x);
    X::embed(c, k, 0);
    X::mul(sx, t, c);
    X::template frob_scale<1, 0>(t, qy);
    fp_const_limbs(k, PAIRC[CURVE].psi_y);
    X::embed(c, k, 0);
    X::mul(sy, t, c);
  }
  static TW_FN bool f_equal(const FE& a, const FE& b) {
    FE d;
    X::sub(d, a, b);
    return F::is_zero(d);
  }
  // Q in G2  <=>  psi(Q) = [t - 1] Q, t - 1 = q - r the signed loop count: psi satisfies X^2 - t X + q, so psi(Q) = [t - 1] Q gives
  // [(t - 1)^2 - t (t - 1) + q] Q = [r] Q = O, and G2 is the eigenspace of Frobenius with eigenvalue q = t - 1 (mod r).  Exact, per
  // point, with the 377-bit multiplier the Miller loop steps anyway.  The two predicates take the running point R = [|t - 1|] Q as
  // the bit loop of the Miller loop leaves it, and (sx, sy) = psi(Q).
  // Z = 0 is tested explicitly and means NOT in the subgroup.  dbl_step / add_step are incomplete formulas: a Q with a component of
  // small order in the cofactor group can meet R = O, or R = +-Q at an addition, in mid-loop, and then Z becomes 0.  Z = 0 is a
  // sink of both steps (doubling: Z3 = 2 Y Z; addition: T = 0 gives H = -X, I = X^2 and Z3 = (Z + H)^2 - T - I = 0), every later
  // coordinate is then without meaning, and an all-zero R would satisfy 0 == 0 below.  A member of G2 never meets the exceptional
  // cases: they need m Q in {O, +-Q} for a prefix m of the loop count, 1 < m < 2^377, and Q has prime order r > 2^752.
  // Positive loop count (MNT6753): R = [t - 1] Q projectively against psi(Q): X == sx T and Y == sy Z T with T = Z^2.  No inversion.
  static TW_FN bool run_equals(const Run& R, const FE& sx, const FE& sy) {
    FE a, b;
    const bool z0 = F::is_zero(R.Z);
    X::mul(a, sx, R.T);
    const bool ex = f_equal(R.X, a);
    X::mul(b, R.Z, R.T);
    X::mul(a, sy, b);
    const bool ey = f_equal(R.Y, a);
    return !z0 && ex && ey;
  }
  // Negative loop count (MNT4753): [t - 1] Q = -R, which minus_r_affine has made affine for the closing step: (mx, my).  Taken BEFORE
  // the closing addition (after it R is O).  rz: R.Z as the bit loop left it.
  static TW_FN bool affine_equals(const FE& rz, const FE& mx, const FE& my, const FE& sx, const FE& sy) {
    const bool z0 = F::is_zero(rz);
    const bool ex = f_equal(mx, sx);
    const bool ey = f_equal(my, sy);
    return !z0 && ex && ey;
  }
  // R <- [|t - 1|] Q from R = Q: the point stepping of the Miller loop alone (no G1 side, no tower, no line values).  dbl_step's H, J
  // and L -- three squarings the point does not need -- are computed and dropped: the loop stays the one the pairing runs.
  static HD void step_loop(Run& R, const FE& qx, const FE& qy) {
    FE qy2, H, C4, J, L, L1;
    X::sqr(qy2, qy);
    R.X = qx; R.Y = qy; X::one(R.Z); X::one(R.T);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = PAIRC[CURVE].loop_bits - 2; i >= 0; --i) {
      dbl_step(R, H, C4, J, L);
      if ((PAIRC[CURVE].loop_count[i >> 5] >> (i & 31)) & 1u) add_step(qx, qy, qy2, R, L1);
    }
  }
  // the whole test of one point (not the identity, on the twist)
  static HD bool in_subgroup(const FE& qx, const FE& qy) {
    Run R;
    FE sx, sy;
    step_loop(R, qx, qy);
    endo(sx, sy, qx, qy);
    if (PAIRC[CURVE].loop_neg) {
      FE mx, my, my2;
      minus_r_affine(mx, my, my2, R);
      return affine_equals(R.Z, mx, my, sx, sy);
    }
    return run_equals(R, sx, sy);
  }

  template <int K>
  static HD void miller_loop(TE& f, Pair (&p)[K]) {
    T::one(f);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = PAIRC[CURVE].loop_bits - 2; i >= 0; --i) {
      const bool bit = (PAIRC[CURVE].loop_count[i >> 5] >> (i & 31)) & 1u;
      T::sqr(f, f);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
      for (int j = 0; j < K; ++j) line_dbl(f, p[j]);
      if (bit) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (int j = 0; j < K; ++j) line_add(f, p[j], p[j].qx, p[j].qy, p[j].qy2);
      }
    }
    if (PAIRC[CURVE].loop_neg) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
      for (int j = 0; j < K; ++j) line_close(f, p[j]);
      T::inv(f, f);
    }
  }

  static HD void first_chunk(TE& r, const TE& e, const TE& e_inv) {
    TE t;
    if constexpr (T::K == 4) {
      T::template frobenius<2>(t, e);
      T::mul(r, t, e_inv);
    } else {
      TE a;
      T::template frobenius<3>(t, e);
      T::mul(t, t, e_inv);                       // e^(q^3 - 1)
      T::template frobenius<1>(a, t);
      T::mul(r, a, t);                           // ^(q + 1)
    }
  }
  static TW_FN void final_exponentiation(TE& r, const TE& f) {
    TE fi, a, b, w1, w0;
    T::inv(fi, f);
    first_chunk(a, f, fi);
    first_chunk(b, fi, f);
    T::template frobenius<1>(w1, a);
    T::pow(w0, PAIRC[CURVE].w0_neg ? b : a, PAIRC[CURVE].w0_abs, PAIRC[CURVE].w0_bits);
    T::mul(r, w1, w0);
  }

  static HD void reduced_pairing(TE& r, const B& px, const B& py, const FE& qx, const FE& qy) {
    Pair p[1];
    TE f;
    setup(p[0], px, py, qx, qy);
    miller_loop<1>(f, p);
    final_exponentiation(r, f);
  }
};

#if defined(__HIPCC__)
// ---- wire words <-> this lane's share of an F element ---------------------------------------------------------------------------
template <class F>
__device__ __forceinline__ void wire_load(typename F::E& r, const uint32_t* p) {
  uint32_t w[24];
  if constexpr (F::LANES == 1) {
#pragma unroll 1
    for (int k = 0; k < F::DEG; ++k) {
      load_wire24(w, p + 24 * k);
      fp_from_wire(F::comp(r, k), w);
    }
  } else {
    load_wire24(w, p + 24 * lane_comp<F>());
    fp_from_wire(r, w);
  }
}
template <class F>
__device__ __forceinline__ void wire_store(uint32_t* p, const typename F::E& a) {
  uint32_t w[24];
  if constexpr (F::LANES == 1) {
#pragma unroll 1
    for (int k = 0; k < F::DEG; ++k) {
      fp_to_wire(w, F::comp(a, k));
      store_wire24(p + 24 * k, w);
    }
  } else {
    fp_to_wire(w, a);
    store_wire24(p + 24 * lane_comp<F>(), w);
  }
}
// all y words of a wire-format affine point are zero: the identity (serialization.hpp:84-111).  One answer per lane group.
template <class F>
__device__ __forceinline__ bool wire_y_is_zero(const uint32_t* y) {
  uint32_t o = 0;
  if constexpr (F::LANES == 1) {
    for (int k = 0; k < 24 * F::DEG; ++k) o |= y[k];
    return o == 0;
  } else {
    const uint32_t* mine = y + 24 * lane_comp<F>();
    for (int k = 0; k < 24; ++k) o |= mine[k];
    Fp<F::MOD> z;
    fp_zero(z);
    z.l[0] = o != 0 ? 1u : 0u;
    return F::is_zero(z);
  }
}

// out_gt[t] = e(g1[t], g2[t]), t < n: wire-format affine points in, GT as c0 | c1 in wire form out.  The identity in either argument
// gives one: its lane group runs the arithmetic on the stand-in pair (the generators; every lane of a wave executes the same
// instructions, so nothing is saved by leaving) and writes one instead of the result.  Inputs are canonical and on their curves
// (the caller has checked).
template <class C>
__global__ void __launch_bounds__(256, 1) k_pairing(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ g2, const uint32_t* __restrict__ stand_g1,
                                                   const uint32_t* __restrict__ stand_g2, uint32_t* __restrict__ out_gt, uint32_t n, int unreduced) {
  using A = Ate<C>;
  using F = typename C::F;
  const uint32_t t = logical_lane<F>();
  if (t == 0xffffffffu || t >= n) return;        // (all lanes of a group leave together)
  const uint32_t* p1 = g1 + (size_t)t * 48;
  const uint32_t* p2 = g2 + (size_t)t * 2 * wire_coord_words<C>();
  const bool ident = wire_y_is_zero<FieldFp<F::MOD>>(p1 + 24) || wire_y_is_zero<F>(p2 + wire_coord_words<C>());
  if (ident) { p1 = stand_g1; p2 = stand_g2; }
  typename A::B px, py;
  typename A::FE qx, qy;
  wire_load<FieldFp<F::MOD>>(px, p1);
  wire_load<FieldFp<F::MOD>>(py, p1 + 24);
  wire_load<F>(qx, p2);
  wire_load<F>(qy, p2 + wire_coord_words<C>());
  typename A::TE r;
  if (unreduced) {
    typename A::Pair p[1];
    A::setup(p[0], px, py, qx, qy);
    A::template miller_loop<1>(r, p);
  } else {
    A::reduced_pairing(r, px, py, qx, qy);
  }
  if (ident) A::T::one(r);
  uint32_t* dst = out_gt + (size_t)t * 2 * wire_coord_words<C>();
  wire_store<F>(dst, r.c0);
  wire_store<F>(dst + wire_coord_words<C>(), r.c1);
}

// ---- stored coefficients of a fixed G2 point ----------------------------------------------------------------------------------------
// Layout of one point's coefficients (device form, e_store): for every bit of the loop count below the top one, high to low, the
// doubling step's H | 4C | J | L, then, if the bit is set, the addition step's L1 | RZ; after the last bit the closing step's L1 | RZ
// where the loop count is negative (MNT4753).  ate_coeff_elems = 4 (bits - 1) + 2 (set bits - 1 + closing) elements of F.
template <class C>
constexpr int ate_coeff_elems() {
  constexpr int curve = C::F::DEG == 2 ? CURVE_MNT4753 : CURVE_MNT6753;
  int adds = PAIRC[curve].loop_neg ? 1 : 0;
  for (int i = PAIRC[curve].loop_bits - 2; i >= 0; --i) adds += (PAIRC[curve].loop_count[i >> 5] >> (i & 31)) & 1u;
  return 4 * (PAIRC[curve].loop_bits - 1) + 2 * adds;
}
template <class C>
constexpr int ate_coeff_words() { return ate_coeff_elems<C>() * C::F::DEG * FPS_WORDS; }

// ate_precompute_G2 of ONE point (wire form, not the identity) by one lane group: the launch is one workgroup, lane group 0 works
template <class C>
__global__ void __launch_bounds__(256, 1) k_g2_precompute(const uint32_t* __restrict__ q_wire, uint32_t* __restrict__ coeffs) {
  using A = Ate<C>;
  using F = typename C::F;
  using X = FX<F>;
  constexpr int EW = F::DEG * FPS_WORDS;
  if (logical_lane<F>() != 0u) return;
  typename A::FE qx, qy, qy2, H, C4, J, L, L1;
  wire_load<F>(qx, q_wire);
  wire_load<F>(qy, q_wire + wire_coord_words<C>());
  X::sqr(qy2, qy);
  typename A::Run R;
  R.X = qx; R.Y = qy; X::one(R.Z); X::one(R.T);
  uint32_t* out = coeffs;
#pragma unroll 1
  for (int i = PAIRC[A::CURVE].loop_bits - 2; i >= 0; --i) {
    A::dbl_step(R, H, C4, J, L);
    e_store<F>(out, H); e_store<F>(out + EW, C4); e_store<F>(out + 2 * EW, J); e_store<F>(out + 3 * EW, L);
    out += 4 * EW;
    if ((PAIRC[A::CURVE].loop_count[i >> 5] >> (i & 31)) & 1u) {
      A::add_step(qx, qy, qy2, R, L1);
      e_store<F>(out, L1); e_store<F>(out + EW, R.Z);
      out += 2 * EW;
    }
  }
  if (PAIRC[A::CURVE].loop_neg) {
    typename A::FE mx, my, my2;
    A::minus_r_affine(mx, my, my2, R);
    A::add_step(mx, my, my2, R, L1);
    e_store<F>(out, L1); e_store<F>(out + EW, R.Z);
  }
}

// the G1 side of a pair whose G2 point's coefficients are stored: PX twist, PY twist, L1_coeff, QY / twist
template <class C>
struct StoredPair {
  typename C::F::E px_t, py_t, l1c, qyt;
};
template <class C>
__device__ __attribute__((noinline)) void stored_setup(StoredPair<C>& s, const Fp<C::F::MOD>& px, const Fp<C::F::MOD>& py, const typename C::F::E& qx,
                                                       const typename C::F::E& qy) {
  using F = typename C::F;
  using X = FX<F>;
  Fp<F::MOD> ni;
  typename F::E tinv, t;
  fp_const_limbs(ni, PAIRC[X::CURVE].nr_inv);
  X::embed(tinv, ni, F::DEG - 1);
  X::embed(s.px_t, px, 1);
  X::embed(s.py_t, py, 1);
  X::mul(t, qx, tinv);
  X::embed(s.l1c, px, 0);
  X::sub(s.l1c, s.l1c, t);
  X::mul(s.qyt, qy, tinv);
}
// f <- f g_RR(P) / f <- f g_RQ(P) from stored coefficients; `at` moves past what was read
template <class C>
__device__ __attribute__((noinline)) void stored_line_dbl(typename Tower<typename C::F>::E& f, const StoredPair<C>& s, const uint32_t*& at) {
  using F = typename C::F;
  using X = FX<F>;
  constexpr int EW = F::DEG * FPS_WORDS;
  typename F::E H, C4, J, L, t;
  typename Tower<F>::E g;
  e_load<F>(H, at); e_load<F>(C4, at + EW); e_load<F>(J, at + 2 * EW); e_load<F>(L, at + 3 * EW);
  at += 4 * EW;
  X::mul(t, J, s.px_t);
  X::sub(t, L, t);
  X::sub(g.c0, t, C4);
  X::mul(g.c1, H, s.py_t);
  Tower<F>::mul(f, f, g);
}
template <class C>
__device__ __attribute__((noinline)) void stored_line_add(typename Tower<typename C::F>::E& f, const StoredPair<C>& s, const uint32_t*& at) {
  using F = typename C::F;
  using X = FX<F>;
  constexpr int EW = F::DEG * FPS_WORDS;
  typename F::E L1, RZ, t, u;
  typename Tower<F>::E g;
  e_load<F>(L1, at); e_load<F>(RZ, at + EW);
  at += 2 * EW;
  X::mul(g.c0, RZ, s.py_t);
  X::mul(t, s.qyt, RZ);
  X::mul(u, s.l1c, L1);
  X::add(t, t, u);
  X::neg(g.c1, t);
  Tower<F>::mul(f, f, g);
}
// The verifier's Miller loop: one pair stepped as it goes (p) and two pairs read from a key's stored coefficients, one squaring.
// SUB: also the subgroup test of the stepped pair's G2 point, on the running point the loop holds anyway (Ate<C>::run_equals /
// affine_equals); returns its answer (true without SUB).
template <class C, bool SUB = false>
__device__ __forceinline__ bool miller_loop_verify(typename Tower<typename C::F>::E& f, typename Ate<C>::Pair& p, const StoredPair<C>& s1, const uint32_t* c1,
                                                   const StoredPair<C>& s2, const uint32_t* c2) {
  using A = Ate<C>;
  using T = Tower<typename C::F>;
  bool member = true;
  T::one(f);
#pragma unroll 1
  for (int i = PAIRC[A::CURVE].loop_bits - 2; i >= 0; --i) {
    const bool bit = (PAIRC[A::CURVE].loop_count[i >> 5] >> (i & 31)) & 1u;
    T::sqr(f, f);
    A::line_dbl(f, p);
    stored_line_dbl<C>(f, s1, c1);
    stored_line_dbl<C>(f, s2, c2);
    if (bit) {
      A::line_add(f, p, p.qx, p.qy, p.qy2);
      stored_line_add<C>(f, s1, c1);
      stored_line_add<C>(f, s2, c2);
    }
  }
  if (PAIRC[A::CURVE].loop_neg) {
    if constexpr (SUB) {
      typename A::FE sx, sy, mx, my, my2;
      A::endo(sx, sy, p.qx, p.qy);
      A::minus_r_affine(mx, my, my2, p.R);
      member = A::affine_equals(p.R.Z, mx, my, sx, sy);
      A::line_add(f, p, mx, my, my2);            // line_close, with -R affine in hand
    } else {
      A::line_close(f, p);
    }
    stored_line_add<C>(f, s1, c1);
    stored_line_add<C>(f, s2, c2);
    T::inv(f, f);
  } else if constexpr (SUB) {
    typename A::FE sx, sy;
    A::endo(sx, sy, p.qx, p.qy);
    member = A::run_equals(p.R, sx, sy);
  }
  return member;
}

// ---- Groth16 verification ---------------------------------------------------------------------------------------------------------
// the 768-bit integer of the wire words is >= the modulus
template <int M>
__device__ __forceinline__ bool wire_noncanonical(const uint32_t* p) {
  uint32_t borrow = 0;
  for (int j = 0; j < 24; ++j) {
    const uint32_t pj = (uint32_t)(FPC[M].p64[j >> 1] >> (32 * (j & 1)));
    const uint64_t t = (uint64_t)p[j] - pj - borrow;
    borrow = (uint32_t)(t >> 63);
  }
  return borrow == 0;
}
// one answer for the lane group: every lane's flag is set
template <class F>
__device__ __forceinline__ bool group_all(bool mine) {
  if constexpr (F::LANES == 1) return mine;
  else {
    Fp<F::MOD> z;
    fp_zero(z);
    z.l[0] = mine ? 0u : 1u;
    return F::is_zero(z);
  }
}
// y^2 == x^3 + a x + b on G1 (C1: Mnt4G1 / Mnt6G1), one multiplier instance
template <class C1>
__device__ __attribute__((noinline)) bool g1_on_curve(const Fp<C1::F::MOD>& x, const Fp<C1::F::MOD>& y) {
  using B = Fp<C1::F::MOD>;
  constexpr int curve = C1::F::MOD == MOD_B ? CURVE_MNT4753 : CURVE_MNT6753;
  B a, b, r, xx, x3;
#pragma nounroll
  for (int step = 0; step < 3; ++step) {
    switch (step) {
      case 0: a = x; b = x; break;
      case 1: a = xx; b = x; break;
      default: a = y; b = y; break;
    }
    fp_mul(r, a, b);
    if (step == 0) xx = r;
    if (step == 1) x3 = r;
  }
  B ax, cb;
  C1::mul_by_a(ax, x);
  fp_const_limbs(cb, CURVE_B[curve].g1);
  fp_add(x3, x3, ax);
  fp_add(x3, x3, cb);
  fp_sub(x3, r, x3);
  return fp_is_zero(x3);
}
// the same on the twist, in the field form of C
template <class C>
__device__ __attribute__((noinline)) bool g2_on_curve(const typename C::F::E& x, const typename C::F::E& y) {
  using F = typename C::F;
  using X = FX<F>;
  typename F::E xx, x3, yy, ax, cb;
  X::sqr(xx, x);
  X::mul(x3, xx, x);
  X::sqr(yy, y);
  C::mul_by_a(ax, x);
  if constexpr (F::LANES == 1) {
#pragma unroll
    for (int k = 0; k < F::DEG; ++k) fp_const_limbs(F::comp(cb, k), CURVE_B[X::CURVE].g2[k]);
  } else {
    const int comp = tw_lane_comp<F>();
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      uint32_t v = CURVE_B[X::CURVE].g2[0][i];
      if (comp == 1) v = CURVE_B[X::CURVE].g2[1][i];
      if (comp == 2) v = CURVE_B[X::CURVE].g2[2][i];
      cb.l[i] = v;
    }
  }
  X::add(x3, x3, ax);
  X::add(x3, x3, cb);
  X::sub(x3, yy, x3);
  return F::is_zero(x3);
}

// inputs (n x num_inputs Fr, wire form) -> their integers (as_bigint), and bad[t] |= 1 where one of proof t's inputs is >= r
template <int FR>
__global__ void __launch_bounds__(256) k_inputs_to_integer(const uint32_t* __restrict__ inputs, uint32_t* __restrict__ ints, uint8_t* __restrict__ bad,
                                                          uint32_t n, uint32_t num_inputs) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  uint8_t b = 0;
#pragma unroll 1
  for (uint32_t j = 0; j < num_inputs; ++j) {
    const size_t at = ((size_t)t * num_inputs + j) * 24;
    uint32_t w[24], s[24];
    load_wire24(w, inputs + at);
    if (wire_noncanonical<FR>(inputs + at)) b = 1;
    fp_wire_to_integer<FR>(s, w);
    store_wire24(ints + at, s);
  }
  bad[t] = b;
}

// acc[t] = ABC[0] + sum_j input[t][j] ABC[j + 1], affine wire form (the identity: all words zero), one lane per proof: a joint
// double-and-add over the 753 bits of all inputs -- per bit one doubling and one mixed addition for every input whose bit is set,
// through one instance of the point VM -- then one inversion.  753 (1 + num_inputs / 2) group operations per proof on average in one
// lane: right for a handful of public inputs.  A key with tens to thousands of them is prepared (mnt753_vk_prepare_inputs) and then
// runs k_vk_walk / k_vk_segment_sum over window tables instead (vk_input_kernels.hip.h), which write the same words.
template <class C1>
__global__ void __launch_bounds__(256, 1) k_vk_accumulate(const uint32_t* __restrict__ abc, const uint32_t* __restrict__ ints, uint32_t* __restrict__ out,
                                                         uint32_t n, uint32_t num_inputs) {
  using F = typename C1::F;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Proj<C1> acc, Q;
  pt_set_zero(acc);
  F::zero(Q.X); F::zero(Q.Y); F::one(Q.Z);
  const uint32_t per_bit = num_inputs + 1;
  const uint32_t steps = num_inputs ? 753u * per_bit + 1u : 1u;
#pragma unroll 1
  for (uint32_t s = 0; s < steps; ++s) {
    const bool last = s + 1 == steps;
    const uint32_t bit = 752u - s / per_bit, j = s % per_bit;      // j == 0: the doubling of this bit; j >= 1: input j - 1
    int pc = PC_END;
    if (!last && j == 0) {
      if (!pt_is_zero(acc)) pc = PC_DBL;
    } else {
      bool take = last;
      if (!last) take = (ints[((size_t)t * num_inputs + (j - 1)) * 24 + (bit >> 5)] >> (bit & 31)) & 1u;
      if (take) {
        const uint32_t* src = abc + (size_t)(last ? 0u : j) * 48;
        uint32_t w[24];
        load_wire24(w, src); fp_from_wire(Q.X, w);
        load_wire24(w, src + 24); fp_from_wire(Q.Y, w);
        if (pt_is_zero(acc)) { acc.X = Q.X; acc.Y = Q.Y; F::one(acc.Z); }
        else pc = PC_MADD;
      }
    }
    pt_vm<C1, false>(acc, Q, pc);
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

// verdicts[t] for proof t = (A | B | C) against the key: 0 accepted, 1 malformed, 2 the pairing check failed.
//   FE(ML(A, B) ML(-acc, G2::one()) ML(-C, delta)) == e(alpha, beta): one Miller loop over three pairs that share the squaring and
//   one final exponentiation.  Only B is stepped; the line coefficients of G2::one() and delta are read from the key (coeffs:
//   ate_coeff_words words for G2::one(), then as many for delta, written by k_g2_precompute).  (The reference's form multiplies ML(A, B) by the unitary inverse of the other two's product; the two
//   differ by a factor in the subfield, which the final exponentiation kills.)
// key: stand-in G1 | G2::one() | delta_g2 | e(alpha, beta), wire words.  acc: mnt753_vk_accumulate's output for these proofs.
// bad[t] != 0 on entry: an input of proof t is >= r.  A malformed proof -- a non-canonical coordinate, a point off its curve, an
// identity among A, B, C or acc, such an input -- runs the arithmetic on the stand-in points (the generators), so that its neighbours
// in the wave see nothing of it, and its verdict is 1.  No subgroup test of B unless SUB: then a well-formed
// proof whose B is not in the order-r subgroup of the twist gets verdict 3, before the pairing check is looked at (the pairing is
// bilinear on G2 only); a malformed proof steps the generator, which is in G2, and stays 1.
template <class C, class C1, bool SUB = false>
__global__ void __launch_bounds__(256, 1) k_groth16_verify(const uint32_t* __restrict__ proofs, const uint32_t* __restrict__ acc, const uint32_t* __restrict__ key,
                                                          const uint32_t* __restrict__ coeffs, const uint8_t* __restrict__ bad, uint8_t* __restrict__ verdicts, uint32_t n) {
  using A = Ate<C>;
  using F = typename C::F;
  using F1 = FieldFp<F::MOD>;
  constexpr int M = F::MOD;
  constexpr int W2 = wire_coord_words<C>();      // words of one G2 coordinate
  const uint32_t t = logical_lane<F>();
  if (t == 0xffffffffu || t >= n) return;
  const uint32_t* pa = proofs + (size_t)t * (96 + 2 * W2);
  const uint32_t* pb = pa + 48;
  const uint32_t* pc = pb + 2 * W2;
  const uint32_t* pacc = acc + (size_t)t * 48;
  const uint32_t *stand1 = key, *gen2 = key + 48, *delta = gen2 + 2 * W2, *gt = delta + 2 * W2;
  bool malformed = bad[t] != 0;
  malformed |= wire_noncanonical<M>(pa) || wire_noncanonical<M>(pa + 24) || wire_noncanonical<M>(pc) || wire_noncanonical<M>(pc + 24);
  {
    const int comp = (int)lane_comp<F>();
    bool nc = false;
    if constexpr (F::LANES == 1) {
      for (int k = 0; k < 2 * F::DEG; ++k) nc |= wire_noncanonical<M>(pb + 24 * k);
    } else {
      nc = wire_noncanonical<M>(pb + 24 * comp) || wire_noncanonical<M>(pb + W2 + 24 * comp);
    }
    malformed |= !group_all<F>(!nc);
  }
  malformed |= wire_y_is_zero<F1>(pa + 24) || wire_y_is_zero<F1>(pc + 24) || wire_y_is_zero<F1>(pacc + 24) || wire_y_is_zero<F>(pb + W2);
  typename A::B ax, ay, cx, cy, sx, sy;
  typename A::FE bx, by;
  wire_load<F1>(ax, pa); wire_load<F1>(ay, pa + 24);
  wire_load<F1>(cx, pc); wire_load<F1>(cy, pc + 24);
  wire_load<F>(bx, pb); wire_load<F>(by, pb + W2);
  if (!malformed) malformed = !(g1_on_curve<C1>(ax, ay) && g1_on_curve<C1>(cx, cy) && g2_on_curve<C>(bx, by));
  if (malformed) {
    wire_load<F1>(ax, stand1); wire_load<F1>(ay, stand1 + 24);
    cx = ax; cy = ay; sx = ax; sy = ay;
    wire_load<F>(bx, gen2); wire_load<F>(by, gen2 + W2);
  } else {
    wire_load<F1>(sx, pacc); wire_load<F1>(sy, pacc + 24);
  }
  fp_neg(sy, sy);
  fp_neg(cy, cy);
  typename A::Pair p;
  StoredPair<C> s1, s2;
  typename A::FE qx, qy;
  A::setup(p, ax, ay, bx, by);
  wire_load<F>(qx, gen2); wire_load<F>(qy, gen2 + W2);
  stored_setup<C>(s1, sx, sy, qx, qy);
  wire_load<F>(qx, delta); wire_load<F>(qy, delta + W2);
  stored_setup<C>(s2, cx, cy, qx, qy);
  typename A::TE f, r;
  constexpr int CW = ate_coeff_words<C>();
  const bool member = miller_loop_verify<C, SUB>(f, p, s1, coeffs, s2, coeffs + CW);
  A::final_exponentiation(r, f);
  bool same = true;
#pragma unroll 1
  for (int h = 0; h < 2; ++h) {
    const uint32_t* want = gt + h * W2;
    if constexpr (F::LANES == 1) {
      for (int k = 0; k < F::DEG; ++k) {
        uint32_t w[24];
        fp_to_wire(w, F::comp(h == 0 ? r.c0 : r.c1, k));
        for (int i = 0; i < 24; ++i) same &= w[i] == want[24 * k + i];
      }
    } else {
      uint32_t w[24];
      fp_to_wire(w, h == 0 ? r.c0 : r.c1);
      for (int i = 0; i < 24; ++i) same &= w[i] == want[24 * lane_comp<F>() + i];
    }
  }
  same = group_all<F>(same);
  if (lane_comp<F>() == 0) verdicts[t] = malformed ? 1 : (!member ? 3 : (same ? 0 : 2));
}

// ---- subgroup membership of a point set ----------------------------------------------------------------------------------------------
// The report record of k_g2_subgroup: number of bad points and the lowest key, key = index << 3 | reason (the reasons of
// include/mnt753_hip.h go up to MNT753_BAD_NOT_IN_SUBGROUP = 4; mnt753_validate.hip's own record keeps two bits), all ones = good.
struct SubgroupReport {
  unsigned long long n_bad, key;
};
static __global__ void k_subgroup_report_init(SubgroupReport* rec) {   // (static: the header serves more than one unit of the library)
  rec->n_bad = 0;
  rec->key = ~0ull;
}
// Per point (n affine wire-format points of the twist, point base + t by lane group t, lane mapping as k_pairing), the first that
// applies: a coordinate component >= q -> 1 (non-canonical); all y words zero -> the identity, good; off the twist -> 2; psi(Q) !=
// [t - 1] Q -> 4 (Ate<C>::in_subgroup).  A point that fails an earlier test, and the identity, steps the stand-in (stand_g2: the
// generator), as a malformed proof does in the verifier.  The record does not depend on scheduling: one lane per group holds the
// point's key, a wave's count and lowest key come from a ballot (indices grow with the lane, so the lowest flagged lane holds the
// wave's minimum), and a wave that found something issues one 64-bit atomic add and one 64-bit atomic min.
template <class C>
__global__ void __launch_bounds__(256, 1) k_g2_subgroup(const uint32_t* __restrict__ g2, const uint32_t* __restrict__ stand_g2, uint32_t n,
                                                       unsigned long long base, SubgroupReport* __restrict__ rec) {
  using A = Ate<C>;
  using F = typename C::F;
  constexpr int M = F::MOD;
  constexpr int W2 = wire_coord_words<C>();
  const uint32_t t = logical_lane<F>();
  if (t == 0xffffffffu || t >= n) return;        // (all lanes of a group leave together)
  const uint32_t* p2 = g2 + (size_t)t * 2 * W2;
  const int comp = (int)lane_comp<F>();
  bool nc = false;
  if constexpr (F::LANES == 1) {
    for (int k = 0; k < 2 * F::DEG; ++k) nc |= wire_noncanonical<M>(p2 + 24 * k);
  } else {
    nc = wire_noncanonical<M>(p2 + 24 * comp) || wire_noncanonical<M>(p2 + W2 + 24 * comp);
  }
  const bool noncanon = !group_all<F>(!nc);
  const bool ident = wire_y_is_zero<F>(p2 + W2);
  typename A::FE qx, qy;
  wire_load<F>(qx, p2);
  wire_load<F>(qy, p2 + W2);
  uint32_t reason = 0;                           // MNT753_BAD_NONE
  if (noncanon) reason = 1;                      // MNT753_BAD_NONCANONICAL
  else if (!ident && !g2_on_curve<C>(qx, qy)) reason = 2;   // MNT753_BAD_OFF_CURVE
  if (reason != 0 || ident) {
    wire_load<F>(qx, stand_g2);
    wire_load<F>(qy, stand_g2 + W2);
  }
  const bool member = A::in_subgroup(qx, qy);
  if (reason == 0 && !ident && !member) reason = 4;   // MNT753_BAD_NOT_IN_SUBGROUP
  const bool flag = comp == 0 && reason != 0;
  const unsigned long long bad = __ballot(flag);
  if (bad && (int)(threadIdx.x & 63u) == __ffsll(bad) - 1) {
    atomicAdd(&rec->n_bad, (unsigned long long)__popcll(bad));
    atomicMin(&rec->key, ((base + t) << 3) | reason);
  }
}

// The two halves of the test for n points each (test hooks): what == 0: psi(P); what == 1: [t - 1] P, affine wire words, the identity
// (the stepping ended with Z = 0) as zero words.  Points on the twist, not the identity.
template <class C>
__global__ void __launch_bounds__(256, 1) k_g2_subgroup_half(int what, const uint32_t* __restrict__ g2, uint32_t* __restrict__ out, uint32_t n) {
  using A = Ate<C>;
  using F = typename C::F;
  using X = FX<F>;
  constexpr int W2 = wire_coord_words<C>();
  const uint32_t t = logical_lane<F>();
  if (t == 0xffffffffu || t >= n) return;
  typename A::FE qx, qy, rx, ry;
  wire_load<F>(qx, g2 + (size_t)t * 2 * W2);
  wire_load<F>(qy, g2 + (size_t)t * 2 * W2 + W2);
  if (what == 0) {
    A::endo(rx, ry, qx, qy);
  } else {
    typename A::Run R;
    typename A::FE my2;
    A::step_loop(R, qx, qy);
    const bool z0 = F::is_zero(R.Z);
    A::minus_r_affine(rx, ry, my2, R);           // -R affine: [t - 1] P where the loop count is negative
    if (!PAIRC[A::CURVE].loop_neg) X::neg(ry, ry);
    if (z0) { X::zero(rx); X::zero(ry); }
  }
  uint32_t* dst = out + (size_t)t * 2 * W2;
  wire_store<F>(dst, rx);
  wire_store<F>(dst + W2, ry);
}
#endif  // __HIPCC__

}  // namespace mnt753
