// Modular inversion without exponentiation: Bernstein-Yang "safegcd" division steps, 28 at a time.
//
// Replaces libff's Fp_model::invert (fields/fp.tcc:641-685, mpn_gcdext) on the device.  The Fermat chain a^(p-2) costs
// ~950 Montgomery products (about 3 ms of wave time for ONE inversion on gfx950); this costs 78 batches of
//     28 division steps on the low words of (f, g)              -- 32-bit ALU only, builds a 2x2 transition matrix
//     (f, g) <- M (f, g) / 2^28 ,  (d, e) <- M (d, e) / 2^28 mod p -- 27 x 6 multiply-adds (v_mad_i64_i32)
// i.e. ~90 k simple instructions = ~55 product-equivalents.  Every lane runs the same instruction sequence (the division
// steps are the constant-time formulation: masks, no branches), so a wave inverts 64 different elements at full rate.
//
// Number of steps: the original divstep (delta starts at 1) needs at most floor((49 d + 57) / 17) steps for inputs below
// 2^d (Bernstein-Yang 2019, Theorem 11.2); d = 754 gives 2176 <= 78 * 28 = 2184.
// Measured and NOT adopted (round 3; the build switch left the source in round 5): the half-delta variant (delta starts at 1/2, as in libsecp256k1's
// modinv) run UNTIL g = 0 IN EVERY LANE OF THE WAVE -- once g is 0 a batch is the identity (transition matrix 2^28 I), so lanes
// that are done early are unharmed and correctness rests on no step bound.  Random 753-bit inputs need 1520 steps on average and
// 1536 as the maximum over the 64 lanes of a wave (simulation over 2560 inputs: at most 1544): 55-56 batches instead of 78.  Same
// registers, bit-identical results (131 GPU tests) -- and no gain: same box, alternating, G1 2^20 24.96 / 25.25 ms fixed against
// 25.14 / 25.05 early, G2 2^20 65.98 / 65.79 against 69.36 / 69.76 (profiles/r03/ab_inversion_early_exit.txt).  The inversion is
// the low-power phase of a pairing level (32-bit ALU work, no multiplies); shortening it shortens the time the chip spends below
// its power limit, and the multiplier phases around it pay that back in clock.
//
// Representation inside the routine: 27 limbs of 28 bits, limbs 0..25 in [0, 2^28), limb 26 signed -- the same limb width
// as fp753.hip.h, so a 28-step batch divides by exactly one limb.  d and e stay in (-2p, p), f and g in [-p, p].
#pragma once
#include "fp753.hip.h"

namespace mnt753 {

struct InvMat { int32_t u, v, q, r; };

// 28 division steps on the low limbs; returns the new eta = -(delta + 1/2) (delta > 0 <=> eta < 0) and the transition matrix t with
//   (f', g') = t (f, g) / 2^28
HD int32_t inv_divsteps28(int32_t eta, uint32_t f0, uint32_t g0, InvMat& t) {
  uint32_t u = 1, v = 0, q = 0, r = 1;
  uint32_t f = f0, g = g0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
  for (int i = 0; i < 28; ++i) {
    uint32_t c1 = (uint32_t)(eta >> 31);          // delta > 0
    const uint32_t c2 = 0u - (g & 1u);            // g odd
    const uint32_t x = (f ^ c1) - c1, y = (u ^ c1) - c1, z = (v ^ c1) - c1;   // -f, -u, -v when delta > 0
    g += x & c2; q += y & c2; r += z & c2;
    c1 &= c2;                                     // swap case: delta > 0 and g odd
    eta = (int32_t)(((uint32_t)eta ^ c1) - (c1 + 1u));   // eta = -delta: delta <- 1 - delta (swap) or 1 + delta
    f += g & c1; u += q & c1; v += r & c1;
    g >>= 1; u <<= 1; v <<= 1;
  }
  t.u = (int32_t)u; t.v = (int32_t)v; t.q = (int32_t)q; t.r = (int32_t)r;
  return eta;
}

// (f, g) <- t (f, g) / 2^28  (exact: the low 28 bits vanish by construction)
HD void inv_update_fg(int32_t f[NL], int32_t g[NL], const InvMat& t) {
  int64_t cf = (int64_t)t.u * f[0] + (int64_t)t.v * g[0];
  int64_t cg = (int64_t)t.q * f[0] + (int64_t)t.r * g[0];
  cf >>= LB; cg >>= LB;
#pragma unroll
  for (int i = 1; i < NL; ++i) {
    cf += (int64_t)t.u * f[i] + (int64_t)t.v * g[i];
    cg += (int64_t)t.q * f[i] + (int64_t)t.r * g[i];
    f[i - 1] = (int32_t)((uint32_t)cf & LMASK); cf >>= LB;
    g[i - 1] = (int32_t)((uint32_t)cg & LMASK); cg >>= LB;
  }
  f[NL - 1] = (int32_t)cf;
  g[NL - 1] = (int32_t)cg;
}

// (d, e) <- t (d, e) / 2^28 mod p, keeping both in (-2p, p): a multiple of p is added that clears the low limb
template <int M>
HD void inv_update_de(int32_t d[NL], int32_t e[NL], const InvMat& t) {
  const uint32_t pinv = (0u - FPC[M].inv) & LMASK;        // p^-1 mod 2^28 (the table holds -p^-1)
  const int32_t sd = d[NL - 1] >> 31, se = e[NL - 1] >> 31;   // sign masks
  int32_t md = (t.u & sd) + (t.v & se);                   // start from +p for every negative input
  int32_t me = (t.q & sd) + (t.r & se);
  int64_t cd = (int64_t)t.u * d[0] + (int64_t)t.v * e[0];
  int64_t ce = (int64_t)t.q * d[0] + (int64_t)t.r * e[0];
  md -= (int32_t)((pinv * (uint32_t)cd + (uint32_t)md) & LMASK);
  me -= (int32_t)((pinv * (uint32_t)ce + (uint32_t)me) & LMASK);
  cd += (int64_t)FPC[M].p[0] * md;
  ce += (int64_t)FPC[M].p[0] * me;
  cd >>= LB; ce >>= LB;
#pragma unroll
  for (int i = 1; i < NL; ++i) {
    cd += (int64_t)t.u * d[i] + (int64_t)t.v * e[i] + (int64_t)FPC[M].p[i] * md;
    ce += (int64_t)t.q * d[i] + (int64_t)t.r * e[i] + (int64_t)FPC[M].p[i] * me;
    d[i - 1] = (int32_t)((uint32_t)cd & LMASK); cd >>= LB;
    e[i - 1] = (int32_t)((uint32_t)ce & LMASK); ce >>= LB;
  }
  d[NL - 1] = (int32_t)cd;
  e[NL - 1] = (int32_t)ce;
}

// r = a^-1 as plain integers mod p: a canonical in [0, p) (limbs as in Fp), r canonical; a = 0 gives r = 0.
template <int M>
HD void fp_inv_integer(uint32_t r[NL], const uint32_t a[NL]) {
  int32_t d[NL], e[NL], f[NL], g[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) { d[i] = 0; e[i] = 0; f[i] = (int32_t)FPC[M].p[i]; g[i] = (int32_t)a[i]; }
  e[0] = 1;
  int32_t eta = -1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int it = 0; it < 78; ++it) {
    InvMat t;
    eta = inv_divsteps28(eta, (uint32_t)f[0], (uint32_t)g[0], t);
    inv_update_de<M>(d, e, t);
    inv_update_fg(f, g, t);
  }
  // g = 0 and f = +-1 now (f = +-p when a = 0); d * a = f (mod p).  Negate d when f < 0, then bring it into [0, p).
  const int32_t sf = f[NL - 1] >> 31;
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) {            // d <- (d ^ sf) - sf, limb-wise with borrow
    int32_t v = (d[i] ^ sf) - sf + c;
    if (i < NL - 1) { c = v >> LB; v &= (int32_t)LMASK; }
    d[i] = v;
  }
  // limbs 0..25 of the negated value: (x ^ -1) - (-1) = -x per limb needs the carry chain above because inner limbs are
  // unsigned; after it d is again "inner limbs in [0, 2^28), top limb signed", value in (-2p, 2p)
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {     // add p while negative (at most twice)
    const int32_t neg = d[NL - 1] >> 31;
    c = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      int32_t v = d[i] + ((int32_t)FPC[M].p[i] & neg) + c;
      if (i < NL - 1) { c = v >> LB; v &= (int32_t)LMASK; }
      d[i] = v;
    }
  }
  {                                          // subtract p once if d >= p
    int32_t s[NL];
    c = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      int32_t v = d[i] - (int32_t)FPC[M].p[i] + c;
      if (i < NL - 1) { c = v >> LB; v &= (int32_t)LMASK; }
      s[i] = v;
    }
    const int32_t ge = ~(s[NL - 1] >> 31);   // all ones when d - p >= 0
#pragma unroll
    for (int i = 0; i < NL; ++i) d[i] = (s[i] & ge) | (d[i] & ~ge);
  }
#pragma unroll
  for (int i = 0; i < NL; ++i) r[i] = (uint32_t)d[i];
}

// Montgomery-form inverse in the device representation (radix R' = 2^756, values lazily in [0, 2p)):
// x = a R'  ->  r = a^-1 R'.  The integer inverse of x is a^-1 R'^-1; two products by R'^2 restore the radix:
// mul(mul(y, R'^2), R'^2) = y R'^2.  Zero maps to zero.
template <int M>
HD void fp_inv(Fp<M>& r, const Fp<M>& x) {
  Fp<M> c, y, r2, t;
  fp_canon(c, x);
  fp_inv_integer<M>(y.l, c.l);
  fp_const_limbs(r2, FPC[M].r2p);
  fp_mul(t, y, r2);
  fp_mul(r, t, r2);
}


// ---- one inversion by a group of G lanes (the pairing levels of the base fields, msm_kernels.hip.h) --------------------------------
// Under SIMT a wave pays fp_inv's ~90 k instructions whether one lane or all 64 need an inverse.  fp_inv_group<M, G> computes ONE
// inverse with the G consecutive lanes of a group, limb-parallel: lane j holds limbs LPL j .. LPL j + LPL - 1 of f, g, d and e
// (LPL = 32 / G limb slots per lane, slots 27..31 hold zero), every lane runs the 28 division steps of a batch on the low limbs
// (broadcast from the group's lane 0), and each lane applies the transition matrix to its own limbs only.  Same 78 batches, same 28
// steps, same matrices as fp_inv_integer; the result is its canonical integer inverse, bit for bit.
//
// Limb ranges (asserted after every batch by tools/host_inv_group_check.cpp).  A batch forms, per limb i, the 64-bit column
//   c_i = m0 a_i + m1 b_i (+ p_i mp),   |m0| + |m1| <= 2^28, |mp| < 2^29, |a_i|, |b_i| < 2^28 + 2^4:   |c_i| < 2^58
// and splits it into lo(c_i) in [0, 2^28) and hi(c_i) = c_i >> 28 in (-2^30, 2^30).  The quotient by 2^28 has the limbs
//   v_i = lo(c_{i+1}) + hi(c_i)                   in (-2^30, 2^30 + 2^28)      (one hand-over: lo of the next lane's first limb)
// and a second, small carry brings them back:
//   limb_i = (v_i & mask) + (v_{i-1} >> 28)       in [-4, 2^28 + 4)            (one hand-over: the previous lane's last carry)
// Nothing comes into limb 0, so limb 0 is EXACT in [0, 2^28) -- the division steps and the multiple of p that clears the low limb of
// (d, e) read it -- limbs 1..25 are redundant within [-4, 2^28 + 4), limb 26 is signed and keeps whatever is above (never masked,
// no carry out of it).  The values are exact throughout; only their limbs are not unique.  The sign of d and e (fp_inv_integer adds p
// to a negative input of the matrix) is taken from limb 26, which is the sign of the value unless |value| < 2^709; adding p or not to a
// value that small keeps d and e in (-2p - 2^709, p + 2^709) instead of (-2p, p).  The carries are resolved once, at the end, in every
// lane (inv_grp_finish: three conditional additions of p and one subtraction cover that range).
//
// The per-lane arithmetic below is __host__ __device__; only the exchange between lanes is device code.  The host model
// (tools/host_inv_group_check.cpp) runs the same functions with the lanes as an array index.
template <int G>
struct InvGrp {
  static_assert(G == 8 || G == 16 || G == 32, "group sizes: 8, 16 or 32 lanes");
  static constexpr int LPL = 32 / G;                         // limb slots per lane
  static constexpr int TOP_LANE = (NL - 1) / LPL, TOP_SLOT = (NL - 1) % LPL;
};

// this lane's limbs of a 27-limb value: slot k of lane j is limb LPL j + k (zero beyond limb 26)
template <int LPL>
HD void inv_grp_take(int32_t out[LPL], const uint32_t a[NL], int j) {
#pragma unroll
  for (int k = 0; k < LPL; ++k) out[k] = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i)
    if (i / LPL == j) out[i % LPL] = (int32_t)a[i];
}
// the mask of the second carry per slot: 28 bits, all 32 for limb 26 (and nothing is carried out of it)
template <int LPL>
HD void inv_grp_masks(uint32_t keep[LPL], int j) {
#pragma unroll
  for (int k = 0; k < LPL; ++k) keep[k] = LPL * j + k == NL - 1 ? 0xffffffffu : LMASK;
}
// columns of this lane's limbs, split: c = m0 a + m1 b (+ pl mp)
template <int LPL, bool WITH_P>
HD void inv_grp_columns(int32_t lo[LPL], int32_t hi[LPL], const int32_t a[LPL], const int32_t b[LPL], int32_t m0, int32_t m1,
                        const int32_t pl[LPL], int32_t mp) {
#pragma unroll
  for (int k = 0; k < LPL; ++k) {
    int64_t c = (int64_t)m0 * a[k] + (int64_t)m1 * b[k];
    if (WITH_P) c += (int64_t)pl[k] * mp;
    lo[k] = (int32_t)((uint32_t)c & LMASK);
    hi[k] = (int32_t)(c >> LB);
  }
}
// v_i = lo(c_{i+1}) + hi(c_i); lo_next = lo of the next lane's slot 0 (0 behind the group's last lane)
template <int LPL>
HD void inv_grp_shift(int32_t v[LPL], const int32_t lo[LPL], const int32_t hi[LPL], int32_t lo_next) {
#pragma unroll
  for (int k = 0; k < LPL; ++k) v[k] = (k + 1 < LPL ? lo[k + 1] : lo_next) + hi[k];
}
// the small carry out of a slot: v >> 28, nothing out of limb 26
HD int32_t inv_grp_carry(int32_t v, uint32_t keep) { return (int32_t)((uint32_t)v & ~keep) >> LB; }
// limb = (v & mask) + carry of the slot below; carry_in = the previous lane's inv_grp_carry of its last slot (0 for the group's lane 0)
template <int LPL>
HD void inv_grp_settle(int32_t out[LPL], const int32_t v[LPL], const uint32_t keep[LPL], int32_t carry_in) {
#pragma unroll
  for (int k = 0; k < LPL; ++k) out[k] = (int32_t)((uint32_t)v[k] & keep[k]) + (k ? inv_grp_carry(v[k - 1], keep[k - 1]) : carry_in);
}
// the multiples of p that (d, e) <- t (d, e) / 2^28 takes (inv_update_de): +p for every input judged negative (sd, se = sign masks
// of limb 26), then whatever clears the low 28 bits.  d0, e0 = the exact low limbs.
template <int M>
HD void inv_grp_pmult(int32_t& md, int32_t& me, const InvMat& t, int32_t sd, int32_t se, uint32_t d0, uint32_t e0) {
  const uint32_t pinv = (0u - FPC[M].inv) & LMASK;
  md = (t.u & sd) + (t.v & se);
  me = (t.q & sd) + (t.r & se);
  const uint32_t cd = (uint32_t)t.u * d0 + (uint32_t)t.v * e0;
  const uint32_t ce = (uint32_t)t.q * d0 + (uint32_t)t.r * e0;
  md -= (int32_t)((pinv * cd + (uint32_t)md) & LMASK);
  me -= (int32_t)((pinv * ce + (uint32_t)me) & LMASK);
}
// The end, in every lane: d = all 27 limbs (redundant as above), f0 = the exact low limb of f (f = +-1: 1 or 2^28 - 1; f = p for the
// input 0, whose d is 0 mod p).  r = the canonical residue of d (carries resolved, p added while negative -- at most three times --
// and subtracted once), negated mod p when f = -1.
template <int M>
HD void inv_grp_finish(uint32_t r[NL], int32_t d[NL], uint32_t f0) {
  int32_t c;
#pragma unroll 1
  for (int pass = 0; pass < 4; ++pass) {
    const int32_t neg = pass == 0 ? 0 : d[NL - 1] >> 31;      // pass 0 only resolves the carries (the sign is exact behind it)
    c = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      int32_t v = d[i] + ((int32_t)FPC[M].p[i] & neg) + c;
      if (i < NL - 1) { c = v >> LB; v &= (int32_t)LMASK; }
      d[i] = v;
    }
  }
  // d in [0, p + 2^709) now.  s = d - p and n = p - d = -s; pick d, s or their negatives
  int32_t s[NL], n[NL];
  c = 0;
  int32_t cn = 0, nz = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    int32_t v = d[i] - (int32_t)FPC[M].p[i] + c;
    int32_t w = (int32_t)FPC[M].p[i] - d[i] + cn;
    if (i < NL - 1) { c = v >> LB; v &= (int32_t)LMASK; cn = w >> LB; w &= (int32_t)LMASK; }
    s[i] = v; n[i] = w;
    nz |= d[i];
  }
  const int32_t ge = ~(s[NL - 1] >> 31);                      // d >= p: take d - p (its negative, 2p - d, is then p - (d - p): below)
  const int32_t sf = f0 == LMASK ? -1 : 0;                    // f = -1: the inverse is -d
  // canonical e = ge ? s : d;  result = sf ? (e == 0 ? 0 : p - e) : e.   p - e for ge: p - (d - p) -- d >= p happens only within 2^709
  // of p, and p - s is then formed from s the same way n is from d
  int32_t ns[NL];
  cn = 0;
  int32_t nzs = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    int32_t w = (int32_t)FPC[M].p[i] - s[i] + cn;
    if (i < NL - 1) { cn = w >> LB; w &= (int32_t)LMASK; }
    ns[i] = w;
    nzs |= s[i];
  }
  const int32_t e_nz = (ge ? nzs : nz) != 0 ? -1 : 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int32_t e = (s[i] & ge) | (d[i] & ~ge);
    const int32_t ne = ((ns[i] & ge) | (n[i] & ~ge)) & e_nz;
    r[i] = (uint32_t)((ne & sf) | (e & ~sf));
  }
}

#if defined(__HIPCC__)
// ---- the exchange between the lanes of a group (device only) ----
// G = 16 is one DPP row: neighbours by row_shl / row_shr with bound_ctrl (0 comes in at the ends), broadcasts by row_newbcast; the
// other sizes go through ds_bpermute
template <int G> __device__ __forceinline__ int32_t inv_grp_from_next(int32_t x) {          // lane + 1's value, 0 in the last lane
  if constexpr (G == 16) return __builtin_amdgcn_update_dpp(0, x, 0x101, 0xf, 0xf, true);  // row_shl:1
  else { const int l = (int)(threadIdx.x & 63u); const int y = __builtin_amdgcn_ds_bpermute(((l + 1) & 63) << 2, x); return (l & (G - 1)) == G - 1 ? 0 : y; }
}
template <int G> __device__ __forceinline__ int32_t inv_grp_from_prev(int32_t x) {          // lane - 1's value, 0 in the first lane
  if constexpr (G == 16) return __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);  // row_shr:1
  else { const int l = (int)(threadIdx.x & 63u); const int y = __builtin_amdgcn_ds_bpermute(((l - 1) & 63) << 2, x); return (l & (G - 1)) == 0 ? 0 : y; }
}
template <int G, int SRC> __device__ __forceinline__ int32_t inv_grp_bcast(int32_t x) {      // the value of the group's lane SRC
  if constexpr (G == 16) return __builtin_amdgcn_update_dpp(0, x, 0x150 + SRC, 0xf, 0xf, false);   // row_newbcast:SRC
  else { const int l = (int)(threadIdx.x & 63u); return __builtin_amdgcn_ds_bpermute(((l & ~(G - 1)) + SRC) << 2, x); }
}

// limb I of a value spread over the group, into every lane
template <int G, int I>
struct InvGrpGather {
  static __device__ __forceinline__ void run(int32_t D[NL], const int32_t d[InvGrp<G>::LPL]) {
    D[I] = inv_grp_bcast<G, I / InvGrp<G>::LPL>(d[I % InvGrp<G>::LPL]);
    if constexpr (I + 1 < NL) InvGrpGather<G, I + 1>::run(D, d);
  }
};

// r = a^-1 as plain integers mod p, computed by the G lanes of a group together: every lane of the group passes the SAME canonical a
// and gets the same r = fp_inv_integer(a).  All 64 lanes of the wave must be active.
template <int M, int G>
__device__ __forceinline__ void fp_inv_integer_group(uint32_t r[NL], const uint32_t a[NL]) {
  constexpr int LPL = InvGrp<G>::LPL;
  const int j = (int)(threadIdx.x & (unsigned)(G - 1));
  int32_t d[LPL], e[LPL], f[LPL], g[LPL], pl[LPL];
  uint32_t keep[LPL];
  inv_grp_take<LPL>(pl, FPC[M].p, j);
  inv_grp_take<LPL>(g, a, j);
  inv_grp_masks<LPL>(keep, j);
#pragma unroll
  for (int k = 0; k < LPL; ++k) { d[k] = 0; e[k] = 0; f[k] = pl[k]; }
  if (j == 0) e[0] = 1;
  int32_t eta = -1;
#pragma unroll 1
  for (int it = 0; it < 78; ++it) {
    InvMat t;
    const uint32_t f0 = (uint32_t)inv_grp_bcast<G, 0>(f[0]), g0 = (uint32_t)inv_grp_bcast<G, 0>(g[0]);
    const uint32_t d0 = (uint32_t)inv_grp_bcast<G, 0>(d[0]), e0 = (uint32_t)inv_grp_bcast<G, 0>(e[0]);
    const int32_t sd = inv_grp_bcast<G, InvGrp<G>::TOP_LANE>(d[InvGrp<G>::TOP_SLOT]) >> 31;
    const int32_t se = inv_grp_bcast<G, InvGrp<G>::TOP_LANE>(e[InvGrp<G>::TOP_SLOT]) >> 31;
    eta = inv_divsteps28(eta, f0, g0, t);
    int32_t md, me;
    inv_grp_pmult<M>(md, me, t, sd, se, d0, e0);
    int32_t lo[LPL], hi[LPL], v[4][LPL];
    inv_grp_columns<LPL, true>(lo, hi, d, e, t.u, t.v, pl, md);
    inv_grp_shift<LPL>(v[0], lo, hi, inv_grp_from_next<G>(lo[0]));
    inv_grp_columns<LPL, true>(lo, hi, d, e, t.q, t.r, pl, me);
    inv_grp_shift<LPL>(v[1], lo, hi, inv_grp_from_next<G>(lo[0]));
    inv_grp_columns<LPL, false>(lo, hi, f, g, t.u, t.v, pl, 0);
    inv_grp_shift<LPL>(v[2], lo, hi, inv_grp_from_next<G>(lo[0]));
    inv_grp_columns<LPL, false>(lo, hi, f, g, t.q, t.r, pl, 0);
    inv_grp_shift<LPL>(v[3], lo, hi, inv_grp_from_next<G>(lo[0]));
    inv_grp_settle<LPL>(d, v[0], keep, inv_grp_from_prev<G>(inv_grp_carry(v[0][LPL - 1], keep[LPL - 1])));
    inv_grp_settle<LPL>(e, v[1], keep, inv_grp_from_prev<G>(inv_grp_carry(v[1][LPL - 1], keep[LPL - 1])));
    inv_grp_settle<LPL>(f, v[2], keep, inv_grp_from_prev<G>(inv_grp_carry(v[2][LPL - 1], keep[LPL - 1])));
    inv_grp_settle<LPL>(g, v[3], keep, inv_grp_from_prev<G>(inv_grp_carry(v[3][LPL - 1], keep[LPL - 1])));
  }
  // all limbs of d into every lane, then the same end in each
  int32_t D[NL];
  InvGrpGather<G, 0>::run(D, d);
  inv_grp_finish<M>(r, D, (uint32_t)inv_grp_bcast<G, 0>(f[0]));
}

// fp_inv by a group: every lane of the group passes the same x in [0, 2p) and gets fp_inv(x), bit for bit
template <int M, int G>
__device__ __forceinline__ void fp_inv_group(Fp<M>& r, const Fp<M>& x) {
  Fp<M> c, y, r2, t;
  fp_canon(c, x);
  fp_inv_integer_group<M, G>(y.l, c.l);
  fp_const_limbs(r2, FPC[M].r2p);
  fp_mul(t, y, r2);
  fp_mul(r, t, r2);
}
// Every lane its OWN inverse for the price of one group inversion: Montgomery's trick across the G lanes of a group.
//   up, log2 G products:   level s multiplies the products of the two halves of a block of 2^(s+1) lanes (the partner's value by
//                          ds_bpermute; fp_mul's columns are symmetric in its operands, so both partners hold the same limbs);
//   fp_inv_group on the group's product (every lane of the group holds it);
//   down, log2 G products: inverse of the own half = inverse of the block x product of the sibling half (kept from the way up).
// r = x^-1 mod p in [0, 2p) -- the residue of fp_inv(x), not necessarily its limbs (p may lie between them); zero maps to zero and
// takes part as 1.  All 64 lanes of the wave must be active.  2 log2 G + 2 products and one shared inversion per lane: about 45 k
// instructions at G = 16 against fp_inv's 93 k.
// P: the product over this lane's block of 2^S lanes (the same limbs in every lane of the block) -> its inverse
template <int M, int G, int S>
struct InvLanesLevel {
  static __device__ __forceinline__ void run(Fp<M>& P) {
    if constexpr ((1 << S) == G) {
      const Fp<M> x = P;
      fp_inv_group<M, G>(P, x);
    } else {
      const int src4 = (int)(((threadIdx.x & 63u) ^ (1u << S)) << 2);
      Fp<M> sib, up;
#pragma unroll
      for (int i = 0; i < NL; ++i) sib.l[i] = (uint32_t)__builtin_amdgcn_ds_bpermute(src4, (int)P.l[i]);
      fp_mul(up, P, sib);
      InvLanesLevel<M, G, S + 1>::run(up);
      fp_mul(P, up, sib);
    }
  }
};
template <int M, int G>
__device__ __forceinline__ void fp_inv_lanes(Fp<M>& r, const Fp<M>& x) {
  const bool zero = fp_is_zero(x);
  Fp<M> P;
#pragma unroll
  for (int i = 0; i < NL; ++i) P.l[i] = zero ? FPC[M].one[i] : x.l[i];
  InvLanesLevel<M, G, 0>::run(P);
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = zero ? 0u : P.l[i];
}
#endif  // __HIPCC__

}  // namespace mnt753
