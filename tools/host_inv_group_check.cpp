// CPU-suite harness: a host model of fp_inv_integer_group (fp_inv.hip.h) -- one Bernstein-Yang inversion computed limb-parallel by a
// group of G lanes.  The lanes are an array index here and the exchange between them (DPP / ds_bpermute on the device) is an array
// read; the per-lane arithmetic is the SAME __host__ __device__ code the device runs (inv_grp_*).  For G = 8, 16, 32 and both moduli:
//   * the result equals fp_inv_integer's, bit for bit, and a * a^-1 = 1 in the host field (host_field.hpp, an independent inversion);
//   * inputs: 0, 1, 2, p - 1, p - 2, (p +- 1) / 2, R' mod p, 2^k for every k < 753, values whose low 28, 56 and 84 bits are zero,
//     and 10^5 seeded random values (G = 16; 2 * 10^4 for the other two sizes);
//   * after EVERY batch the limb ranges stated above the routine are asserted: limb 0 exact in [0, 2^28), limbs 1..25 in
//     [-4, 2^28 + 4), slots beyond limb 26 zero, the columns inside int64 by the stated margin, and the values of d, e inside
//     (-2p - 2^709, p + 2^709) (checked on the top limbs).
//   g++ -O2 -std=c++17 tools/host_inv_group_check.cpp -o build/host_inv_group_check && build/host_inv_group_check   (from the repo root)
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <cstdlib>
#include <vector>
#include "../snark-challenge-prover-reference_amd/csrc/fp_inv.hip.h"
#include "../snark-challenge-prover-reference_amd/csrc/host_field.hpp"
using namespace mnt753;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static long g_range_bad = 0;

template <int G>
struct Model {
  static constexpr int LPL = InvGrp<G>::LPL;
  int32_t d[G][LPL], e[G][LPL], f[G][LPL], g[G][LPL], pl[G][LPL];
  uint32_t keep[G][LPL];

  static void check_limbs(const int32_t x[G][LPL], const char* what, int it) {
    for (int j = 0; j < G; ++j)
      for (int k = 0; k < LPL; ++k) {
        const int i = LPL * j + k;
        const int64_t v = x[j][k];
        bool ok;
        if (i == 0) ok = v >= 0 && v < (1 << LB);
        else if (i < NL - 1) ok = v >= -4 && v < (1 << LB) + 4;
        else if (i == NL - 1) ok = v > -(1 << 27) && v < (1 << 27);        // |value| < 3p < 2^755 = 2^27 2^728
        else ok = v == 0;
        if (!ok) { if (++g_range_bad < 8) printf("G=%d: limb %d of %s out of range after batch %d: %lld\n", G, i, what, it, (long long)v); }
      }
  }

  // one half of a batch: (x, y) <- (m0 x + m1 y (+ p mp)) / 2^28, as the device does it: columns, hand-over of lo, hand-over of the carry
  template <bool WITH_P>
  void apply(int32_t out[G][LPL], const int32_t x[G][LPL], const int32_t y[G][LPL], int32_t m0, int32_t m1, int32_t mp) {
    int32_t lo[G][LPL], hi[G][LPL], v[G][LPL];
    for (int j = 0; j < G; ++j) {
      inv_grp_columns<LPL, WITH_P>(lo[j], hi[j], x[j], y[j], m0, m1, pl[j], mp);
      for (int k = 0; k < LPL; ++k) {     // the column itself, against the stated bound
        const __int128 c = (__int128)m0 * x[j][k] + (__int128)m1 * y[j][k] + (WITH_P ? (__int128)pl[j][k] * mp : 0);
        if (c >= ((__int128)1 << 58) || c <= -((__int128)1 << 58)) { if (++g_range_bad < 8) printf("G=%d: column beyond 2^58\n", G); }
      }
    }
    for (int j = 0; j < G; ++j) inv_grp_shift<LPL>(v[j], lo[j], hi[j], j + 1 < G ? lo[j + 1][0] : 0);
    for (int j = 0; j < G; ++j) inv_grp_settle<LPL>(out[j], v[j], keep[j], j ? inv_grp_carry(v[j - 1][LPL - 1], keep[j - 1][LPL - 1]) : 0);
  }

  template <int M>
  void run(uint32_t r[NL], const uint32_t a[NL]) {
    for (int j = 0; j < G; ++j) {
      inv_grp_take<LPL>(pl[j], FPC[M].p, j);
      inv_grp_take<LPL>(g[j], a, j);
      inv_grp_masks<LPL>(keep[j], j);
      for (int k = 0; k < LPL; ++k) { d[j][k] = 0; e[j][k] = 0; f[j][k] = pl[j][k]; }
    }
    e[0][0] = 1;
    int32_t eta = -1;
    for (int it = 0; it < 78; ++it) {
      InvMat t;
      // every lane runs the same steps on the same broadcast words: once here
      const int32_t sd = d[InvGrp<G>::TOP_LANE][InvGrp<G>::TOP_SLOT] >> 31, se = e[InvGrp<G>::TOP_LANE][InvGrp<G>::TOP_SLOT] >> 31;
      eta = inv_divsteps28(eta, (uint32_t)f[0][0], (uint32_t)g[0][0], t);
      int32_t md, me;
      inv_grp_pmult<M>(md, me, t, sd, se, (uint32_t)d[0][0], (uint32_t)e[0][0]);
      int32_t nd[G][LPL], ne[G][LPL], nf[G][LPL], ng[G][LPL];
      apply<true>(nd, d, e, t.u, t.v, md);
      apply<true>(ne, d, e, t.q, t.r, me);
      apply<false>(nf, f, g, t.u, t.v, 0);
      apply<false>(ng, f, g, t.q, t.r, 0);
      memcpy(d, nd, sizeof(d)); memcpy(e, ne, sizeof(e)); memcpy(f, nf, sizeof(f)); memcpy(g, ng, sizeof(g));
      check_limbs(d, "d", it); check_limbs(e, "e", it); check_limbs(f, "f", it); check_limbs(g, "g", it);
      // d, e in (-2p - 2^709, p + 2^709): on the top limb (p's is 0x1c4c62d; the lower limbs add less than 1 to it)
      for (const auto* x : {&d, &e}) {
        const int32_t top = (*x)[InvGrp<G>::TOP_LANE][InvGrp<G>::TOP_SLOT];
        if (top < -2 * (int32_t)FPC[M].p[NL - 1] - 3 || top > (int32_t)FPC[M].p[NL - 1] + 1) { if (++g_range_bad < 8) printf("G=%d: d / e outside (-2p, p) after batch %d\n", G, it); }
      }
    }
    int32_t D[NL];
    for (int i = 0; i < NL; ++i) D[i] = d[i / LPL][i % LPL];
    inv_grp_finish<M>(r, D, (uint32_t)f[0][0]);
  }
};

template <int M> static void canon_from_limbs(uint32_t a[NL]) {   // any 27 limbs of 28 bits (below 2^756) -> canonical residue
  Fp<M> x, one, t, r2, c;
  for (int i = 0; i < NL; ++i) x.l[i] = a[i];
  // x * R'^2 / R' / R' * ... : reduce by two Montgomery products that cancel (x * r2p / R' = x R', then * 1 / R' = x), then canon
  fp_const_limbs(r2, FPC[M].r2p);
  fp_mul(t, x, r2);
  fp_zero(one); one.l[0] = 1;
  fp_mul(x, t, one);
  fp_canon(c, x);
  for (int i = 0; i < NL; ++i) a[i] = c.l[i];
}

template <int M> static bool times_is_one(const uint32_t a[NL], const uint32_t inv[NL]) {
  // independent of the division steps: the host field (64-bit limbs, binary Euclid) on the same integers
  using H = host::HFp<M>;
  auto to_h = [](const uint32_t l[NL]) {
    uint64_t w[12] = {0};
    for (int i = 0; i < NL; ++i) {
      const int bit = LB * i;
      w[bit >> 6] |= (uint64_t)l[i] << (bit & 63);
      if ((bit & 63) + LB > 64 && (bit >> 6) + 1 < 12) w[(bit >> 6) + 1] |= (uint64_t)l[i] >> (64 - (bit & 63));
    }
    H r2 = H::from_words(FPC[M].r2_64);
    return H::from_words(w) * r2;          // integer -> Montgomery form
  };
  const H ha = to_h(a), hi = to_h(inv);
  if (ha.is_zero()) return hi.is_zero();
  return ha * hi == H::one() && ha.inverse() == hi;
}

template <int M, int G> static bool one_value(const uint32_t a_in[NL], const char* what, long idx) {
  uint32_t a[NL], want[NL], got[NL];
  memcpy(a, a_in, sizeof(a));
  canon_from_limbs<M>(a);
  fp_inv_integer<M>(want, a);
  static Model<G> m;
  m.template run<M>(got, a);
  if (memcmp(want, got, sizeof(want)) != 0) { printf("modulus %d G=%d: %s %ld differs from fp_inv_integer\n", M, G, what, idx); return false; }
  if (!times_is_one<M>(a, got)) { printf("modulus %d G=%d: %s %ld: not the host field's inverse\n", M, G, what, idx); return false; }
  return true;
}

template <int M, int G> static bool run_all(long n_random) {
  bool ok = true;
  long n = 0;
  auto small = [](uint32_t v, uint32_t a[NL]) { memset(a, 0, 4 * NL); a[0] = v; };
  uint32_t a[NL], p[NL];
  for (int i = 0; i < NL; ++i) p[i] = FPC[M].p[i];
  small(0, a); ok &= one_value<M, G>(a, "edge", n++);
  small(1, a); ok &= one_value<M, G>(a, "edge", n++);
  small(2, a); ok &= one_value<M, G>(a, "edge", n++);
  {                                   // p - 1, p - 2: through the field (modulus A has p_0 = 1)
    Fp<M> z, o, t, t2;
    fp_zero(z); fp_zero(o); o.l[0] = 1;
    fp_sub(t, z, o); fp_canon(t2, t); ok &= one_value<M, G>(t2.l, "edge", n++);
    fp_sub(t, t, o); fp_canon(t2, t); ok &= one_value<M, G>(t2.l, "edge", n++);
  }
  {                                   // (p - 1) / 2 and (p + 1) / 2: shift p right by one bit (p odd), then + 1
    uint32_t h[NL];
    for (int i = 0; i < NL; ++i) h[i] = (p[i] >> 1) | (i + 1 < NL ? (p[i + 1] & 1u) << (LB - 1) : 0u);
    ok &= one_value<M, G>(h, "edge", n++);
    h[0] += 1;                        // (p - 1) / 2 is followed by (p + 1) / 2; a carry out of limb 0 is folded by canon_from_limbs
    ok &= one_value<M, G>(h, "edge", n++);
  }
  {                                   // R' mod p = the Montgomery form of 1
    uint32_t o[NL];
    for (int i = 0; i < NL; ++i) o[i] = FPC[M].one[i];
    ok &= one_value<M, G>(o, "edge", n++);
  }
  for (int k = 0; k < 753; ++k) { memset(a, 0, sizeof(a)); a[k / LB] = 1u << (k % LB); ok &= one_value<M, G>(a, "2^k, k =", k); }
  for (int z = 1; z <= 3; ++z)        // low 28, 56, 84 bits zero
    for (int rep = 0; rep < 50; ++rep) {
      for (int i = 0; i < NL; ++i) a[i] = i < z ? 0u : (uint32_t)rnd() & LMASK;
      a[NL - 1] &= 0xffffffu;
      ok &= one_value<M, G>(a, "low limbs zero", z * 100 + rep);
    }
  for (long i = 0; i < n_random && ok; ++i) {
    for (int k = 0; k < NL; ++k) a[k] = (uint32_t)rnd() & LMASK;
    ok &= one_value<M, G>(a, "random", i);
  }
  printf("modulus %d, G = %2d: %ld random values and the edges: %s\n", M, G, n_random, ok ? "OK" : "FAILED");
  return ok;
}

int main(int argc, char** argv) {
  const long n16 = argc > 1 ? atol(argv[1]) : 100000, n_other = n16 / 5;
  bool ok = true;
  ok &= run_all<MOD_A, 16>(n16);
  ok &= run_all<MOD_B, 16>(n16);
  ok &= run_all<MOD_A, 8>(n_other);
  ok &= run_all<MOD_B, 8>(n_other);
  ok &= run_all<MOD_A, 32>(n_other);
  ok &= run_all<MOD_B, 32>(n_other);
  if (g_range_bad) { printf("%ld limb-range violations\n", g_range_bad); ok = false; }
  printf("%s\n", ok ? "ALL OK" : "FAILURES");
  return ok ? 0 : 1;
}
