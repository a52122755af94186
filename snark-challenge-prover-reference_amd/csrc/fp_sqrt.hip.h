// Square roots in the four coordinate fields: Fq of MNT4753 (2-adicity of q - 1: s = 15) and of MNT6753 (s = 30), Fq2 of MNT4753
// (s = 16), Fq3 of MNT6753 (s = 30) -- what decompressing a point needs (libff: sqrt() in depends/libff/libff/algebra/fields/fp.tcc,
// fp2.tcc, fp3.tcc:154-206, all three the same Tonelli-Shanks).
//
// One template over the field classes of curve753.hip.h: FieldFp<MOD>, the one-lane FieldFp2 / FieldFp3, which a host compiler takes
// as well (tools/host_sqrt_check.cpp), and the lane-split FieldFp2S / FieldFp3S the device runs, in the style of tower753.hip.h: every
// product is an out-of-line function (TW_FN), one instance of the field's multiplier per kernel.
//
// Algorithm, with |F| - 1 = 2^s t, t odd, z a non-square, c = z^t of order 2^s (mnt753_sqrt_constants.h, generated):
//     w = a^((t - 1) / 2),  x = a w,  b = x w = a^t                                      invariant: x^2 = a b
//     for i = s .. 2:   if b^(2^(i - 2)) != 1:  x <- x c, b <- b c^2;     c <- c^2       b's order divides 2^(i - 1) on entry
//     is_square = (x^2 == a)
// CONTROL FLOW IS THE SAME FOR EVERY ELEMENT.  libff's loop searches the order of b and "does not terminate if not a square"; here
// the trip counts are fixed -- (s - 1)(s - 2) / 2 squarings for the tests, s - 1 of c, 2 (s - 1) products whose results are taken or
// dropped by a limb-wise select -- and the exponent (t - 1) / 2 is a constant of the field, so its window schedule is one for all
// lanes.  The test "= 1" is F::is_zero of a difference: in the lane-split fields that is one answer for the lane group (an exchange
// over the group's lanes), so all lanes of a group select alike and every cross-lane operation of the split multiplier is executed
// by all of them.  A non-square falls through the same instructions (its b = a^t has order 2^s, the loop leaves some x) and is
// detected by the closing x^2 == a; zero gives w = x = b = 0, x stays 0, and 0^2 == 0: the root 0, a square.
// Which of the two roots comes out is not specified; callers fix the sign (mnt753_compress.hip).
//
// Window of the fixed exponent: W bits at a time from the top, table a^1 .. a^(2^W - 1) in the lane's private memory (2^W - 1
// entries of 108 B per lane and component), L squarings and about (L / W)(1 - 2^-W) products for an exponent of L bits: L = 737 /
// 722 / 1489 / 2228.  W = 1 keeps no table.  The choice is SQRT_WINDOW, by measurement: DESIGN.md 4.16.
#pragma once
#include "tower753.hip.h"
#include "mnt753_sqrt_constants.h"

#ifndef MNT753_SQRT_WINDOW
#define MNT753_SQRT_WINDOW 4
#endif

namespace mnt753 {

constexpr int SQRT_WINDOW = MNT753_SQRT_WINDOW;

template <class F>
struct Sqrt {
  using E = typename F::E;
  using B = Fp<F::MOD>;
  static constexpr int DEG = F::DEG;
  static constexpr int IDX = DEG == 1 ? (F::MOD == MOD_B ? 0 : 1) : (DEG == 2 ? 2 : 3);   // SQRTC
  static constexpr int S = SQRTC[IDX].s;

  static TW_FN void mul(E& r, const E& a, const E& b) { E t; F::mul(t, a, b); r = t; }
  static TW_FN void sqr(E& r, const E& a) {
    E t;
    if constexpr (has_sqr<F>::value) F::sqr(t, a); else F::mul(t, a, a);
    r = t;
  }
  // a == b, one answer per element (per lane group in the split fields)
  static TW_FN bool equal(const E& a, const E& b) {
    E d;
    F::sub(d, a, b);
    return F::is_zero(d);
  }
  // r = take ? a : r, limb by limb: no branch
  static HD void select(E& r, bool take, const E& a) {
    if constexpr (F::LANES == 1 && DEG > 1) {
      for (int k = 0; k < DEG; ++k) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < NL; ++i) F::comp(r, k).l[i] = take ? F::comp(a, k).l[i] : F::comp(r, k).l[i];
      }
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int i = 0; i < NL; ++i) r.l[i] = take ? a.l[i] : r.l[i];
    }
  }
  // z^t, an element of order 2^s
  static HD void root_of_unity(E& r) {
    if constexpr (F::LANES == 1) {
      for (int k = 0; k < DEG; ++k) fp_const_limbs(F::comp(r, k), SQRTC[IDX].zt[k]);
    } else {
      const int comp = tw_lane_comp<F>();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int i = 0; i < NL; ++i) {
        uint32_t v = SQRTC[IDX].zt[0][i];
        if (comp == 1) v = SQRTC[IDX].zt[1][i];
        if constexpr (DEG == 3) {
          if (comp == 2) v = SQRTC[IDX].zt[2][i];
        }
        r.l[i] = v;
      }
    }
  }

  // a^((t - 1) / 2): fixed windows of W bits from the top of the constant exponent
  template <int W>
  static TW_FN void pow_half_t(E& r, const E& a) {
    constexpr int BITS = SQRTC[IDX].e_bits;
    constexpr int NWIN = (BITS + W - 1) / W;
    auto digit = [](int win) -> unsigned {
      unsigned d = 0;
      for (int k = W - 1; k >= 0; --k) {
        const int bit = win * W + k;
        d = (d << 1) | (bit < BITS ? (SQRTC[IDX].e[bit >> 5] >> (bit & 31)) & 1u : 0u);
      }
      return d;
    };
    E acc;
    if constexpr (W == 1) {
      acc = a;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
      for (int i = BITS - 2; i >= 0; --i) {
        sqr(acc, acc);
        if ((SQRTC[IDX].e[i >> 5] >> (i & 31)) & 1u) mul(acc, acc, a);
      }
    } else {
      E tab[(1 << W) - 1];                       // tab[d - 1] = a^d
      tab[0] = a;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
      for (int d = 2; d < (1 << W); ++d) mul(tab[d - 1], tab[d - 2], a);
      acc = tab[digit(NWIN - 1) - 1];            // the top window holds the top bit: never zero
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
      for (int win = NWIN - 2; win >= 0; --win) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (int k = 0; k < W; ++k) sqr(acc, acc);
        const unsigned d = digit(win);           // a constant of the field: the same for every lane
        if (d) mul(acc, acc, tab[d - 1]);
      }
    }
    r = acc;
  }

  // a square: r^2 = a, is_square = true (a = 0: r = 0); otherwise is_square = false and r is unspecified
  template <int W = SQRT_WINDOW>
  static TW_FN void sqrt(E& r, bool& is_square, const E& a) {
    E w, x, b, c, one, t, u;
    F::one(one);
    pow_half_t<W>(w, a);
    mul(x, a, w);
    mul(b, x, w);
    root_of_unity(c);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = S; i >= 2; --i) {
      t = b;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
      for (int k = 0; k < i - 2; ++k) sqr(t, t);
      const bool step = !equal(t, one);          // one answer per element
      mul(u, x, c);
      select(x, step, u);
      sqr(c, c);
      mul(u, b, c);
      select(b, step, u);
    }
    sqr(t, x);
    is_square = equal(t, a);
    r = x;
  }
};

// ---- the sign of a root ----------------------------------------------------------------------------------------------------------
// libff's flag of a compressed point is Y.as_bigint().data[0] & 1 (for G2: of Y.c0): the parity of the INTEGER in [0, q), out of
// Montgomery form.  sqrt_parity: that bit of this lane's component; sqrt_fix_sign makes y the root with the wanted flag.  Where
// y.c0 = 0 both roots carry flag 0 and libff's format cannot tell them apart: the root whose first non-zero higher component is
// even is taken then, whatever the flag says (a departure).
template <int M>
HD uint32_t sqrt_parity(const Fp<M>& y) {
  Fp<M> raw_one, t, c;
  fp_zero(raw_one);
  raw_one.l[0] = 1u;
  fp_mul(t, y, raw_one);                         // y R' / R' = the integer, in [0, 2q)
  fp_canon(c, t);
  return c.l[0] & 1u;
}
template <class F>
TW_FN void sqrt_fix_sign(typename F::E& y, uint32_t want_odd) {
  using E = typename F::E;
  bool flip;
  if constexpr (F::DEG == 1) {
    flip = sqrt_parity(y) != (want_odd & 1u);
  } else if constexpr (F::LANES == 1) {
    uint32_t par = 0, want = want_odd & 1u;
    bool found = false;
    for (int k = 0; k < F::DEG; ++k) {
      const bool z = fp_is_zero(F::comp(y, k));
      const uint32_t p = sqrt_parity(F::comp(y, k));
      if (!found && !z) { par = p; found = true; if (k > 0) want = 0u; }
    }
    flip = found && par != want;
  } else {
    // each lane looks at its own component; the group's lanes exchange (non-zero, parity) and decide alike
    const uint32_t mine = (fp_is_zero(y) ? 0u : 2u) | sqrt_parity(y);
    uint32_t v[3] = {0u, 0u, 0u};
    if constexpr (F::LANES == 2) {
      const uint32_t other = pair_swap_u32(mine);
      const bool odd = lane_is_odd();
      v[0] = odd ? other : mine;
      v[1] = odd ? mine : other;
    } else {
      const int lane = wave_lane(), g = lane - lane % 3;
      v[0] = lane_fetch_u32(mine, g);
      v[1] = lane_fetch_u32(mine, g + 1);
      v[2] = lane_fetch_u32(mine, g + 2);
    }
    if (v[0] & 2u) flip = (v[0] & 1u) != (want_odd & 1u);
    else if (v[1] & 2u) flip = (v[1] & 1u) != 0u;
    else flip = (v[2] & 2u) != 0u && (v[2] & 1u) != 0u;
  }
  E n;
  F::neg(n, y);
  Sqrt<F>::select(y, flip, n);
}

}  // namespace mnt753
