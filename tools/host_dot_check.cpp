// The accumulation and fold routines of csrc/reduce_kernels.hip.h (k_vec_dot, k_poly_eval, k_red_fold) compiled for the host:
//   g++ -O1 -std=c++17 tools/host_dot_check.cpp
// They run here exactly as the kernels call them, on the operands that push the stated limb and value bounds hardest -- every wire
// operand r - 1 -- and on random ones, for the longest per-thread sequences the launch geometry allows at the largest domain
// (2^30 elements over 1024 blocks of 256 threads: 4096 terms of an inner product, 256 runs of 16 coefficients of a polynomial), one
// more to end on a pending term.  After every step the bounds stated at the top of reduce_kernels.hip.h are asserted, and the
// results are compared with the plain composition of fp_mul and fp_add.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "../snark-challenge-prover-reference_amd/csrc/reduce_kernels.hip.h"
using namespace mnt753;

static uint64_t st = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; }
static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++bad < 12) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// a (non-negative limbs, not normalised) * den < p * num, exactly
template <int M> bool value_below(const Fp<M>& a, uint64_t num, uint64_t den) {
  uint64_t x[NL + 2], y[NL + 2], c = 0;
  for (int i = 0; i < NL; ++i) { c += (uint64_t)a.l[i] * den; x[i] = c & LMASK; c >>= LB; }
  x[NL] = c & LMASK; x[NL + 1] = c >> LB;
  c = 0;
  for (int i = 0; i < NL; ++i) { c += (uint64_t)FPC[M].p[i] * num; y[i] = c & LMASK; c >>= LB; }
  y[NL] = c & LMASK; y[NL + 1] = c >> LB;
  for (int i = NL + 1; i >= 0; --i) if (x[i] != y[i]) return x[i] < y[i];
  return false;
}
template <int M> bool limbs_below(const Fp<M>& a, uint32_t bound) { for (int i = 0; i < NL; ++i) if (a.l[i] >= bound) return false; return true; }
template <int M> bool eq(const Fp<M>& a, const Fp<M>& b) { Fp<M> x, y; fp_canon(x, a); fp_canon(y, b); return memcmp(x.l, y.l, sizeof x.l) == 0; }
// a flushed accumulator: zero, or normalised limbs and a value below 1.51 p
template <int M> bool flushed_ok(const Fp<M>& a) { return limbs_below(a, 1u << LB) && value_below(a, 151, 100); }

template <int M> void wire_max(Fp<M>& a) { for (int i = 0; i < NL; ++i) a.l[i] = FPC[M].p[i]; a.l[0] -= 1; }      // r - 1 (r is odd)
template <int M> void wire_random(Fp<M>& a) {      // a canonical wire operand: random below r
  Fp<M> t, one;
  for (int i = 0; i < NL; ++i) t.l[i] = (uint32_t)rnd() & LMASK;
  t.l[NL - 1] &= 0x1fff;
  fp_one(one); fp_mul(a, t, one); fp_canon(a, a);
}

// one thread of k_vec_dot over `terms` terms; mode 0: all r - 1, 1: random, 2: zero
template <int M> void thread_dot(Fp<M>& acc, Fp<M>& eager, int terms, int mode) {
  uint32_t pending = 0;
  fp_zero(acc); fp_zero(eager);
  for (int i = 0; i < terms; ++i) {
    Fp<M> a, u, p;
    if (mode == 0) { wire_max(a); wire_max(u); } else if (mode == 1) { wire_random(a); wire_random(u); } else { fp_zero(a); fp_zero(u); }
    fp_mul(p, a, u);
    CHECK(limbs_below(p, 1u << LB) && value_below(p, 112, 100), "dot: product out of [0, 1.12 r), M=%d", M);
    dot_step(acc, pending, a, u);
    if (pending) CHECK(limbs_below(acc, 3u << LB) && value_below(acc, 375, 100), "dot: pending accumulator out of range, M=%d term %d", M, i);
    else CHECK(flushed_ok(acc), "dot: normalised accumulator out of range, M=%d term %d", M, i);
    fp_add(eager, eager, p);
  }
  red_flush(acc, pending);
  CHECK(pending == 0 && flushed_ok(acc) && eq(acc, eager), "dot: flushed accumulator, M=%d mode %d", M, mode);
}

// the partial sums of `n` threads the way a block and the fold combine them: pairwise, then a chain
template <int M> void combine_all(Fp<M>* part, int n, Fp<M>& out) {
  for (int off = n / 2; off > 0; off >>= 1)
    for (int i = 0; i < off; ++i) {
      Fp<M> sum = part[i];
      Fp<M> raw = sum;
      for (int j = 0; j < NL; ++j) raw.l[j] += part[i + off].l[j];
      CHECK(limbs_below(raw, 1u << (LB + 1)) && value_below(raw, 302, 100), "combine: sum of two partials out of range, M=%d", M);
      red_combine(sum, part[i + off]);
      CHECK(flushed_ok(sum), "combine: result out of range, M=%d", M);
      part[i] = sum;
    }
  out = part[0];
}

template <int M> void run_dot() {
  for (int mode = 0; mode < 3; ++mode) {
    Fp<M> acc, eager;
    thread_dot<M>(acc, eager, mode == 1 ? 301 : 4097, mode);
    // 64 lanes with the same partial (the worst case again), and with random ones
    Fp<M> part[64], esum;
    fp_zero(esum);
    for (int i = 0; i < 64; ++i) {
      if (mode == 1 && i) { Fp<M> e2; thread_dot<M>(part[i], e2, 3 + i % 4, 1); fp_add(esum, esum, e2); }
      else { part[i] = acc; fp_add(esum, esum, eager); }
    }
    Fp<M> total;
    combine_all<M>(part, 64, total);
    CHECK(eq(total, esum), "combine: value, M=%d mode %d", M, mode);
    // canonical wire words: the sum times k_in
    uint32_t w[24], we[24];
    Fp<M> k, t, c;
    red_finish(w, total);
    fp_const_limbs(k, FPC[M].k_in); fp_mul(t, esum, k); fp_canon(c, t); fp_pack(we, c);
    CHECK(memcmp(w, we, sizeof w) == 0, "finish: wire words, M=%d mode %d", M, mode);
    Fp<M> back; fp_unpack(back, w);
    CHECK(value_below(back, 1, 1), "finish: result not canonical, M=%d", M);
    if (mode == 2) { uint32_t o = 0; for (int i = 0; i < 24; ++i) o |= w[i]; CHECK(o == 0, "finish: zero sum not zero words, M=%d", M); }
  }
}

// one thread of k_poly_eval over `runs` runs of POLY_RUN coefficients starting at run index q0; mode 0: all r - 1 (t too), 1: random
template <int M> void run_poly(int runs, int mode) {
  Fp<M> tw, t, acc, eager;
  if (mode == 0) wire_max(tw); else wire_random(tw);
  { uint32_t w[24]; fp_pack(w, tw); fp_from_wire(t, w); }
  CHECK(value_below(t, 145, 100), "poly: t in device form above 1.45 r, M=%d", M);
  fp_zero(acc); fp_zero(eager);
  uint32_t pending = 0;
  const uint64_t stride = 3;                       // run indices q, q + stride, ..: any stride exercises the same arithmetic
  for (int j = 0; j < runs; ++j) {
    const uint64_t i0 = (uint64_t)j * stride * POLY_RUN;
    Fp<M> c[POLY_RUN], x, e;
    for (uint32_t k = 0; k < POLY_RUN; ++k) { if (mode == 0) wire_max(c[k]); else wire_random(c[k]); }
    x = c[POLY_RUN - 1]; e = c[POLY_RUN - 1];
    for (uint32_t k = POLY_RUN - 1; k-- > 0;) {
      horner_step(x, t, c[k]);
      CHECK(limbs_below(x, 1u << (LB + 1)) && value_below(x, 239, 100), "poly: Horner value out of range, M=%d run %d", M, j);
      Fp<M> pe; fp_mul(pe, e, t); fp_add(e, pe, c[k]);
    }
    { Fp<M> one, xn, en; fp_one(one); fp_mul(xn, x, one); fp_mul(en, e, one);      // x is not in [0, 2p): compare behind a product by one
      CHECK(eq(xn, en), "poly: Horner value, M=%d run %d", M, j); }
    Fp<M> pw, tmp;
    fp_one(pw);
    int top = 63;
    while (top >= 0 && !((i0 >> top) & 1)) --top;
    for (int b = top; b >= 0; --b) {
      fp_sqr(tmp, pw); pw = tmp;
      if ((i0 >> b) & 1) { fp_mul(tmp, pw, t); pw = tmp; }
    }
    CHECK(value_below(pw, 145, 100), "poly: t^i0 above 1.45 r, M=%d", M);
    Fp<M> p; fp_mul(p, x, pw);
    CHECK(limbs_below(p, 1u << LB) && value_below(p, 139, 100), "poly: scaled run out of [0, 1.39 r), M=%d", M);
    poly_run_add(acc, pending, x, pw);
    if (pending) CHECK(limbs_below(acc, 3u << LB) && value_below(acc, 430, 100), "poly: pending accumulator out of range, M=%d", M);
    else CHECK(flushed_ok(acc), "poly: normalised accumulator out of range, M=%d", M);
    fp_mul(tmp, e, pw); fp_add(eager, eager, tmp);
  }
  red_flush(acc, pending);
  CHECK(flushed_ok(acc) && eq(acc, eager), "poly: flushed accumulator, M=%d mode %d", M, mode);
  // the sum is in R-form already: its canonical words are the result.  One run of constant coefficients c at t = 1 sums to 16 c.
  uint32_t w[24], we[24];
  Fp<M> c;
  red_finish_plain(w, acc);
  fp_canon(c, eager); fp_pack(we, c);
  CHECK(memcmp(w, we, sizeof w) == 0, "poly: wire words, M=%d mode %d", M, mode);
  {
    Fp<M> one_dev, cw, x, sum, s16;
    uint32_t pend = 0;
    fp_one(one_dev); wire_random(cw);
    x = cw;
    for (uint32_t k = POLY_RUN - 1; k-- > 0;) horner_step(x, one_dev, cw);
    fp_zero(sum); poly_run_add(sum, pend, x, one_dev); red_flush(sum, pend);
    red_finish_plain(w, sum);
    fp_mul_small(s16, cw, POLY_RUN); fp_canon(c, s16); fp_pack(we, c);
    CHECK(memcmp(w, we, sizeof w) == 0, "poly: 16 c at t = 1, M=%d", M);
  }
}

int main() {
  run_dot<MOD_A>(); run_dot<MOD_B>();
  run_poly<MOD_A>(257, 0); run_poly<MOD_B>(257, 0);
  run_poly<MOD_A>(41, 1); run_poly<MOD_B>(41, 1);
  if (bad) { printf("%d checks failed\n", bad); return 1; }
  printf("ALL OK\n");
  return 0;
}
