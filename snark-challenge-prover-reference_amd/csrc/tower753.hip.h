// The quadratic tower over the coordinate field F of G2: Fq4 = Fq2[v]/(v^2 - u) on MNT4753, Fq6 = Fq3[v]/(v^2 - u) on MNT6753 -- the
// target field of the pairing (libff: depends/libff/libff/algebra/fields/fp4.tcc, fp6_2over3.tcc).
//
// One template for both curves and for both forms of F (curve753.hip.h): the one-lane FieldFp2 / FieldFp3, which a host compiler
// takes as well (tools/host_pairing_check.cpp), and the lane-split FieldFp2S / FieldFp3S, two or three lanes per element, which
// the device runs.  An element is a pair (c0, c1) of F elements; in the split forms every lane of the group holds its component of
// both halves, 54 words per lane.
//
// Code size: a product of F is one inlined instance of the 1458-MAD multiplier or of its fused two- / three-product forms (14 to
// 40 KB of code).  The pairing has some fifty product sites, so everything here is an out-of-line function (TW_FN): one instance of
// each F operation per kernel, operands passed by reference (they live in scratch; a product's 2200 to 4400 multiply-adds dwarf
// the 81 words it moves).
#pragma once
#include "curve753.hip.h"
#include "mnt753_pairing_constants.h"

#if defined(__HIPCC__)
#define TW_FN __host__ __device__ __attribute__((noinline))
#else
#define TW_FN inline
#endif

namespace mnt753 {

// this lane's component index of a lane-split element (0 for one-lane fields)
template <class F>
HD int tw_lane_comp() {
  if constexpr (F::LANES == 2) return lane_is_odd() ? 1 : 0;
  else if constexpr (F::LANES == 3) return wave_lane() % 3;
  else return 0;
}

// ---- F with the operations the tower and the Miller loop need beyond curve753.hip.h's --------------------------------------------
template <class F>
struct FX {
  using E = typename F::E;
  using B = Fp<F::MOD>;
  static constexpr int M = F::MOD;
  static constexpr int DEG = F::DEG;
  static constexpr int CURVE = F::DEG == 2 ? CURVE_MNT4753 : CURVE_MNT6753;
  static constexpr unsigned NR = F::DEG == 2 ? 13u : 11u;

  static TW_FN void mul(E& r, const E& a, const E& b) { E t; F::mul(t, a, b); r = t; }
  static TW_FN void sqr(E& r, const E& a) { E t; F::mul(t, a, a); r = t; }
  static TW_FN void add(E& r, const E& a, const E& b) { F::add(r, a, b); }
  static TW_FN void sub(E& r, const E& a, const E& b) { F::sub(r, a, b); }
  static TW_FN void neg(E& r, const E& a) { F::neg(r, a); }
  static TW_FN void dbl(E& r, const E& a) { F::add(r, a, a); }
  static HD void zero(E& r) { F::zero(r); }
  static HD void one(E& r) { F::one(r); }

  // fp2.tcc:129-142, fp3.tcc:126-143; the split fields bring their own
  static TW_FN void inv(E& r, const E& x) {
    if constexpr (has_inv<F>::value) {
      E t; F::inv(t, x); r = t;
    } else if constexpr (DEG == 2) {
      B t0, t1, n, ni;
      fp_sqr(t0, x.c0); fp_sqr(t1, x.c1);
      fp_mul_small(n, t1, NR);
      fp_sub(n, t0, n);
      fp_inv(ni, n);
      fp_mul(t0, x.c0, ni);
      fp_mul(t1, x.c1, ni);
      r.c0 = t0; fp_neg(r.c1, t1);
    } else {
      B c0, c1, c2, t, u, ti;
      fp_sqr(c0, x.c0); fp_mul(t, x.c1, x.c2); fp_mul_small(u, t, NR); fp_sub(c0, c0, u);      // x0^2 - NR x1 x2
      fp_sqr(t, x.c2); fp_mul_small(c1, t, NR); fp_mul(t, x.c0, x.c1); fp_sub(c1, c1, t);      // NR x2^2 - x0 x1
      fp_sqr(c2, x.c1); fp_mul(t, x.c0, x.c2); fp_sub(c2, c2, t);                              // x1^2 - x0 x2
      fp_mul(t, x.c2, c1); fp_mul(u, x.c1, c2); fp_add(t, t, u); fp_mul_small(u, t, NR);
      fp_mul(t, x.c0, c0); fp_add(t, t, u);                                                    // x0 c0 + NR (x2 c1 + x1 c2)
      fp_inv(ti, t);
      fp_mul(r.c0, c0, ti); fp_mul(r.c1, c1, ti); fp_mul(r.c2, c2, ti);
    }
  }

  // x u: (c0, c1) -> (13 c1, c0) on Fq2, (c0, c1, c2) -> (11 c2, c0, c1) on Fq3; a lane rotation in the split forms
  static TW_FN void mul_by_u(E& r, const E& x) {
    if constexpr (F::LANES == 1 && DEG == 2) {
      B t; fp_mul_small(t, x.c1, NR); r.c1 = x.c0; r.c0 = t;
    } else if constexpr (F::LANES == 1) {
      B t; fp_mul_small(t, x.c2, NR); r.c2 = x.c1; r.c1 = x.c0; r.c0 = t;
    } else {
      E xo, nx;
      if constexpr (F::LANES == 2) {
#pragma unroll
        for (int i = 0; i < NL; ++i) xo.l[i] = pair_swap_u32(x.l[i]);
      } else {
        const int lane = wave_lane(), k = lane % 3, src = lane - k + (k + 2) % 3;
#pragma unroll
        for (int i = 0; i < NL; ++i) xo.l[i] = lane_fetch_u32(x.l[i], src);
      }
      fp_mul_small(nx, xo, NR);
      const bool first = tw_lane_comp<F>() == 0;
#pragma unroll
      for (int i = 0; i < NL; ++i) r.l[i] = first ? nx.l[i] : xo.l[i];
    }
  }

  // component c of x times frob[I][H + 2 c]: half H of a tower element under the q^I-th power map
  template <int I, int H>
  static TW_FN void frob_scale(E& r, const E& x) {
    if constexpr (F::LANES == 1) {
      B k, t;
      fp_const_limbs(k, PAIRC[CURVE].frob[I][H]);
      fp_mul(t, x.c0, k); r.c0 = t;
      fp_const_limbs(k, PAIRC[CURVE].frob[I][H + 2]);
      fp_mul(t, x.c1, k); r.c1 = t;
      if constexpr (DEG == 3) {
        fp_const_limbs(k, PAIRC[CURVE].frob[I][H + 4]);
        fp_mul(t, x.c2, k); r.c2 = t;
      }
    } else {
      const int comp = tw_lane_comp<F>();
      B k, t;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        uint32_t v = PAIRC[CURVE].frob[I][H][i];
        if (comp == 1) v = PAIRC[CURVE].frob[I][H + 2][i];
        if constexpr (DEG == 3) {
          if (comp == 2) v = PAIRC[CURVE].frob[I][H + 4][i];
        }
        k.l[i] = v;
      }
      fp_mul(t, x, k);
      r = t;
    }
  }

  // the element with the base-field value c in component `comp` and zero elsewhere
  static HD void embed(E& r, const B& c, int comp) {
    if constexpr (F::LANES == 1) {
      F::zero(r);
      F::comp(r, comp) = c;
    } else {
      const bool mine = tw_lane_comp<F>() == comp;
#pragma unroll
      for (int i = 0; i < NL; ++i) r.l[i] = mine ? c.l[i] : 0u;
    }
  }
};

// ---- the tower ------------------------------------------------------------------------------------------------------------------
template <class F>
struct Tower {
  using X = FX<F>;
  using FE = typename F::E;
  struct E {
    FE c0, c1;
  };
  static constexpr int K = 2 * F::DEG;   // the embedding degree

  static HD void one(E& r) { F::one(r.c0); F::zero(r.c1); }
  static HD void zero(E& r) { F::zero(r.c0); F::zero(r.c1); }

  // Karatsuba over F: three F products
  static TW_FN void mul(E& r, const E& a, const E& b) {
    FE v0, v1, s, t;
    X::mul(v0, a.c0, b.c0);
    X::mul(v1, a.c1, b.c1);
    X::add(s, a.c0, a.c1);
    X::add(t, b.c0, b.c1);
    X::mul(s, s, t);
    X::sub(s, s, v0);
    X::sub(r.c1, s, v1);
    X::mul_by_u(t, v1);
    X::add(r.c0, v0, t);
  }
  // complex squaring (fp4.tcc / fp6_2over3.tcc squared()): c0 = (a + b)(a + u b) - ab - u ab, c1 = 2 ab; two F products
  static TW_FN void sqr(E& r, const E& a) {
    FE ab, s, t, ub;
    X::mul(ab, a.c0, a.c1);
    X::add(s, a.c0, a.c1);
    X::mul_by_u(ub, a.c1);
    X::add(t, a.c0, ub);
    X::mul(s, s, t);
    X::sub(s, s, ab);
    X::mul_by_u(t, ab);
    X::sub(r.c0, s, t);
    X::dbl(r.c1, ab);
  }
  // (c0 - c1 v) / (c0^2 - u c1^2)
  static TW_FN void inv(E& r, const E& a) {
    FE t0, t1, n;
    X::sqr(t0, a.c0);
    X::sqr(t1, a.c1);
    X::mul_by_u(t1, t1);
    X::sub(n, t0, t1);
    X::inv(n, n);
    X::mul(r.c0, a.c0, n);
    X::mul(t1, a.c1, n);
    X::neg(r.c1, t1);
  }
  // the inverse of an element of norm one over F (whatever the first chunk of the final exponent leaves): conjugation
  static HD void unitary_inverse(E& r, const E& a) { r.c0 = a.c0; X::neg(r.c1, a.c1); }

  // a^(q^I)
  template <int I>
  static HD void frobenius(E& r, const E& a) {
    X::template frob_scale<I % K, 0>(r.c0, a.c0);
    X::template frob_scale<I % K, 1>(r.c1, a.c1);
  }

  // a^e for e of `bits` bits in 32-bit words, e > 0: plain square-and-multiply from the top bit (libff's cyclotomic_exp gives the
  // same element)
  static TW_FN void pow(E& r, const E& a, const uint32_t* e, int bits) {
    E acc = a;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = bits - 2; i >= 0; --i) {
      sqr(acc, acc);
      if ((e[i >> 5] >> (i & 31)) & 1u) mul(acc, acc, a);
    }
    r = acc;
  }
};

}  // namespace mnt753
