// The lazy sums of the witness map and of the QAP column sums compiled for the host:
//   g++ -O1 -std=c++17 tools/host_r1cs_check.cpp
// `term_loop` below restates the term loop of k_r1cs_evaluate (csrc/mnt753_r1cs.hip) and of k_qap_chunks (csrc/qap_kernels.hip.h), and
// `fold_loop` the loop of k_qap_fold, with the same primitive calls of csrc/fp753.hip.h in the same order (fp_load / fp_store are plain
// copies of the 27 limbs).  THE KERNELS AND THIS FILE MIRROR EACH OTHER: whoever changes one changes the other.
//
// Operands, for both moduli: every designed wire integer of tests/r1cs_designed.py as coefficient (through fp_from_wire, as
// k_coeff_to_internal stores it) and as operand, all pairs of them, chains of 1 .. 5, 200 and 201 terms of each pair, sums that are
// = 0, = 1 and = r - 1 (mod r) over 2, 3 and 8 terms, and random canonical operands.  After every step, with exact big-integer comparisons:
//   * the device-form coefficient is below 2 r;
//   * every product has normalised limbs and is below r (2 r / 2^756 + 1) < 1.2211 r, what fp_mul's contract gives for (< 2 r, < r);
//   * the pending accumulator -- a flushed value and two products (below 1.51 r + 2 * 1.2211 r = 3.9522 r), in the fold a flushed value
//     and two partial sums (below 3 * 1.51 r = 4.53 r) -- is inside fp_norm's contract: value below 5 r, and |limb| + 2^28 |q| below
//     2^31 - 2^4 for the quotient q it takes off; the limbs are below 3 2^28;
//   * the flushed accumulator is in [0.49 r, 1.51 r) with limbs below 2^28;
//   * the canonical words equal the eager fp_mul / fp_add composition, and a sum = 0 gives 24 zero words.
// The maxima seen are printed per modulus; the kernels' comments quote them.
//
// --mutant N runs a deliberately broken loop (1: no final fp_canon, 2: no flush on an odd count, 3: fp_norm once per three terms) on the
// same operands: the program must then FAIL, which shows that the designed set notices each fault without a broken kernel running
// anywhere.  Per class of operands it prints how many cases gave wrong words and how many left a stated bound.
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../snark-challenge-prover-reference_amd/csrc/fp753.hip.h"
using namespace mnt753;

static uint64_t st = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; }
static int mutant = 0;
static int bad = 0;

// per class of operands: cases, cases with wrong words, failed bound checks
struct Tally { const char* name; long cases, words, bounds; };
static Tally tallies[] = {{"single pairs", 0, 0, 0}, {"chains, odd length", 0, 0, 0}, {"chains, even length", 0, 0, 0}, {"sums = 0", 0, 0, 0},
                          {"sums = 1, r - 1", 0, 0, 0}, {"random rows", 0, 0, 0}, {"fold: seed and partials", 0, 0, 0}, {"fold: sums = 0", 0, 0, 0},
                          {"fold: chains", 0, 0, 0}};
enum { SINGLE, CHAIN_ODD, CHAIN_EVEN, ZERO, TARGET, RANDOM, FOLD_SEED, FOLD_ZERO, FOLD_CHAIN };
static int cls = SINGLE;
#define BOUND(cond, ...) do { if (!(cond)) { ++tallies[cls].bounds; if (++bad < 12) { printf("FAIL %s:%d [%s]: ", __FILE__, __LINE__, tallies[cls].name); printf(__VA_ARGS__); printf("\n"); } } } while (0)
#define WORDS(cond, ...) do { if (!(cond)) { ++tallies[cls].words; if (++bad < 12) { printf("FAIL %s:%d [%s]: ", __FILE__, __LINE__, tallies[cls].name); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- exact comparisons on un-normalised non-negative limbs -------------------------------------------------------------------------------
// a * den < p * num
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
template <int M> uint32_t max_limb(const Fp<M>& a) { uint32_t m = 0; for (int i = 0; i < NL; ++i) if (a.l[i] > m) m = a.l[i]; return m; }
template <int M> bool value_less(const Fp<M>& a, const Fp<M>& b) {
  uint64_t x[NL + 1], y[NL + 1], c = 0;
  for (int i = 0; i < NL; ++i) { c += a.l[i]; x[i] = c & LMASK; c >>= LB; }
  x[NL] = c; c = 0;
  for (int i = 0; i < NL; ++i) { c += b.l[i]; y[i] = c & LMASK; c >>= LB; }
  y[NL] = c;
  for (int i = NL; i >= 0; --i) if (x[i] != y[i]) return x[i] < y[i];
  return false;
}
template <int M> int per_mille(const Fp<M>& a) { int k = 0; while (!value_below(a, k, 1000)) ++k; return k; }     // value < k / 1000 r
// the quotient fp_norm takes off, computed the way it computes it
template <int M> int norm_q(const Fp<M>& a) {
  const float t = (float)(int32_t)a.l[NL - 1] * (1.0f / (float)FPC[M].p[NL - 1]) - 0.5f;
  int32_t nq = (int32_t)t;
  nq -= (float)nq > t ? 1 : 0;
  return nq;
}
// fp_norm's contract as csrc/fp753.hip.h states it: |value| < 5 p, |limb| < 2^30, |limb| + 2^28 |q| < 2^31 - 2^4 (|q| <= 6)
template <int M> bool norm_contract(const Fp<M>& a) {
  const uint64_t q = (uint64_t)abs(norm_q(a));
  return value_below(a, 5, 1) && limbs_below(a, 1u << 30) && q <= 6 && (uint64_t)max_limb(a) + (q << LB) < (1ull << 31) - 16;
}
template <int M> bool flushed_ok(const Fp<M>& a) { return limbs_below(a, 1u << LB) && value_below(a, 151, 100) && !value_below(a, 49, 100); }

template <int M> struct Maxima {
  Fp<M> product, pending, fold_pending;
  uint32_t limb = 0, fold_limb = 0;
  int q = 0, fold_q = 0;
  Maxima() { fp_zero(product); fp_zero(pending); fp_zero(fold_pending); }
};
template <int M> Maxima<M>& maxima() { static Maxima<M> m; return m; }

// ---- wire integers (raw, canonical, 28-bit limbs) ---------------------------------------------------------------------------------------
template <int M> void raw_p(Fp<M>& a) { for (int i = 0; i < NL; ++i) a.l[i] = FPC[M].p[i]; }
template <int M> void raw_sub(Fp<M>& r, const Fp<M>& a, const Fp<M>& b) {      // a >= b, both normalised
  int32_t c = 0;
  for (int i = 0; i < NL; ++i) { int32_t t = (int32_t)a.l[i] - (int32_t)b.l[i] + c; r.l[i] = (uint32_t)t & LMASK; c = t >> LB; }
}
template <int M> void raw_small(Fp<M>& a, uint32_t v) { fp_zero(a); a.l[0] = v & LMASK; a.l[1] = v >> LB; }
template <int M> void raw_neg(Fp<M>& r, const Fp<M>& a) { Fp<M> t; fp_neg(t, a); fp_canon(r, t); }                 // r - a, 0 for 0
template <int M> void raw_times(Fp<M>& r, const Fp<M>& a, unsigned k) { Fp<M> t; fp_mul_small(t, a, k); fp_canon(r, t); }
template <int M> void raw_add(Fp<M>& r, const Fp<M>& a, const Fp<M>& b) { Fp<M> t; fp_add(t, a, b); fp_canon(r, t); }
template <int M> void raw_one(Fp<M>& a) { Fp<M> one; uint32_t w[24]; fp_one(one); fp_to_wire(w, one); fp_unpack(a, w); }   // R mod r: the wire form of 1
template <int M> void raw_random(Fp<M>& a) {
  Fp<M> t, one;
  for (int i = 0; i < NL; ++i) t.l[i] = (uint32_t)rnd() & LMASK;
  t.l[NL - 1] &= 0x1fff;
  fp_one(one); fp_mul(a, t, one); fp_canon(a, a);
}
// the wanted wire integers of tests/r1cs_designed.py, then the wire forms of the plain 1, 2 and r - 1
template <int M> std::vector<Fp<M>> designed() {
  std::vector<Fp<M>> out;
  Fp<M> p, a, b;
  raw_p(p);
  raw_small(a, 0); out.push_back(a);
  raw_small(a, 1); out.push_back(a);
  raw_small(b, 1); raw_sub(a, p, b); out.push_back(a);                                   // r - 1
  raw_small(b, 2); raw_sub(a, p, b); out.push_back(a);                                   // r - 2
  for (int i = 0; i < NL; ++i) a.l[i] = (p.l[i] >> 1) | (i + 1 < NL ? (p.l[i + 1] & 1u) << (LB - 1) : 0u);
  out.push_back(a);                                                                      // floor(r / 2)
  raw_small(b, 1); raw_add(a, out.back(), b); out.push_back(a);                          // floor(r / 2) + 1
  fp_zero(a); a.l[NL - 1] = 1u << (752 - LB * (NL - 1)); out.push_back(a);                // 2^752
  raw_small(a, LMASK); out.push_back(a);                                                 // one full limb
  for (int i = 0; i < NL; ++i) a.l[i] = i < NL - 1 ? LMASK : 0u;
  out.push_back(a);                                                                      // limbs 0 .. 25 full
  for (int i = 0; i < NL; ++i) b.l[i] = i < NL - 1 ? LMASK : (1u << (753 - LB * (NL - 1))) - 1u;
  raw_sub(a, b, p); out.push_back(a);                                                    // (2^753 - 1) mod r = 2^753 - 1 - r
  raw_small(b, 4096); raw_sub(a, p, b); out.push_back(a);                                // r - 4096: device form = r - 1
  raw_one(a); out.push_back(a);
  raw_add(b, a, a); out.push_back(b);
  raw_neg(b, a); out.push_back(b);
  for (const Fp<M>& v : out)
    if (!limbs_below(v, 1u << LB) || !value_below(v, 1, 1)) { printf("designed operand not canonical, M=%d\n", M); exit(2); }
  return out;
}
template <int M> void to_device(Fp<M>& c, const Fp<M>& raw) {       // k_coeff_to_internal
  uint32_t w[24];
  fp_pack(w, raw);
  fp_from_wire(c, w);
  BOUND(limbs_below(c, 1u << LB) && value_below(c, 2, 1), "coefficient in device form not below 2 r, M=%d", M);
}

// ---- the loops ---------------------------------------------------------------------------------------------------------------------------
struct Term { int c, x; };      // indices into the operand tables

// MIRROR of the term loop of k_r1cs_evaluate and k_qap_chunks: acc is the flushed sum (a chunk's partial), eager the fp_add composition
template <int M> void term_loop(Fp<M>& acc, Fp<M>& eager, const std::vector<Fp<M>>& cdev, const std::vector<Fp<M>>& xs, const std::vector<Term>& row) {
  Maxima<M>& mx = maxima<M>();
  const uint32_t per = mutant == 3 ? 3u : 2u;
  Fp<M> c, x, p;
  fp_zero(acc); fp_zero(eager);
  uint32_t pending = 0;
  for (const Term& t : row) {
    x = xs[t.x];                            // fp_unpack of w R / u R: an integer < r, 28-bit limbs
    c = cdev[t.c];                          // fp_load: c R'
    fp_mul(p, c, x);
    BOUND(limbs_below(p, 1u << LB) && value_below(p, 12211, 10000), "product out of [0, 1.2211 r), M=%d", M);
    if (value_less(mx.product, p)) mx.product = p;
    for (int i = 0; i < NL; ++i) acc.l[i] += p.l[i];
    fp_add(eager, eager, p);
    if (++pending == per) {
      // a flushed value (< 1.51 r) and two products (< 1.2211 r each): below 3.9522 r, limbs below 3 2^28, q <= 3
      BOUND(norm_contract(acc), "pending accumulator outside fp_norm's contract, M=%d q=%d", M, norm_q(acc));
      BOUND(value_below(acc, 39522, 10000) && limbs_below(acc, 3u << LB), "pending accumulator above what a flushed value and two products allow, M=%d", M);
      if (value_less(mx.pending, acc)) mx.pending = acc;
      if (max_limb(acc) > mx.limb) mx.limb = max_limb(acc);
      if (abs(norm_q(acc)) > mx.q) mx.q = abs(norm_q(acc));
      fp_norm(acc, acc); pending = 0;
      BOUND(flushed_ok(acc), "flushed accumulator out of [0.49 r, 1.51 r), M=%d", M);
    } else {
      // one term pending: the flushed value (or zero) and one product
      BOUND(value_below(acc, 27311, 10000) && limbs_below(acc, 2u << LB), "accumulator with one pending term out of range, M=%d", M);
    }
  }
  if (pending && mutant != 2) {
    if (value_less(mx.pending, acc)) mx.pending = acc;
    if (max_limb(acc) > mx.limb) mx.limb = max_limb(acc);
    BOUND(norm_contract(acc), "pending accumulator outside fp_norm's contract at the flush, M=%d", M);
    fp_norm(acc, acc);
  }
  if (!row.empty()) BOUND(flushed_ok(acc), "final accumulator out of [0.49 r, 1.51 r), M=%d terms %zu", M, row.size());
}
// the end of a row of k_r1cs_evaluate
template <int M> void finish(uint32_t w[24], const Fp<M>& acc) {
  Fp<M> canon;
  if (mutant == 1) canon = acc; else fp_canon(canon, acc);
  fp_pack(w, canon);
}
template <int M> void eager_words(uint32_t w[24], const Fp<M>& eager) { Fp<M> c; fp_canon(c, eager); fp_pack(w, c); }

// MIRROR of k_qap_fold: the seed (a raw wire integer, or none) and the partial sums of a column's chunks
template <int M> void fold_loop(uint32_t w[24], Fp<M>& eager, const Fp<M>* seed, const std::vector<Fp<M>>& partial) {
  Maxima<M>& mx = maxima<M>();
  const uint32_t per = mutant == 3 ? 3u : 2u;
  Fp<M> acc, x;
  fp_zero(acc); fp_zero(eager);
  uint32_t pending = 0;
  if (seed) { acc = *seed; pending = 1; eager = *seed; }
  for (const Fp<M>& part : partial) {
    x = part;                               // fp_load: [0.49 r, 1.51 r)
    for (int i = 0; i < NL; ++i) acc.l[i] += x.l[i];
    fp_add(eager, eager, x);
    if (++pending == per) {
      // a flushed value (or the seed) and two partial sums, each below 1.51 r with normalised limbs
      BOUND(norm_contract(acc), "fold: pending accumulator outside fp_norm's contract, M=%d q=%d", M, norm_q(acc));
      BOUND(value_below(acc, 453, 100) && limbs_below(acc, 3u << LB), "fold: pending accumulator above what three values below 1.51 r allow, M=%d", M);
      if (value_less(mx.fold_pending, acc)) mx.fold_pending = acc;
      if (max_limb(acc) > mx.fold_limb) mx.fold_limb = max_limb(acc);
      if (abs(norm_q(acc)) > mx.fold_q) mx.fold_q = abs(norm_q(acc));
      fp_norm(acc, acc); pending = 0;
      BOUND(flushed_ok(acc), "fold: flushed accumulator out of range, M=%d", M);
    }
  }
  if (pending && mutant != 2) {
    if (value_less(mx.fold_pending, acc)) mx.fold_pending = acc;
    BOUND(norm_contract(acc), "fold: pending accumulator outside fp_norm's contract at the flush, M=%d", M);
    fp_norm(acc, acc);
  }
  if (seed || !partial.empty()) BOUND(flushed_ok(acc), "fold: final accumulator out of [0.49 r, 1.51 r), M=%d", M);
  finish(w, acc);
}

static bool all_zero(const uint32_t w[24]) { uint32_t o = 0; for (int i = 0; i < 24; ++i) o |= w[i]; return o == 0; }

// one row: the loop, the words against the eager composition, zero words where the design says so
template <int M> void run_row(const std::vector<Fp<M>>& cdev, const std::vector<Fp<M>>& xs, const std::vector<Term>& row, const Fp<M>* want, const char* what) {
  Fp<M> acc, eager;
  uint32_t w[24], we[24];
  ++tallies[cls].cases;
  term_loop(acc, eager, cdev, xs, row);
  finish(w, acc);
  eager_words(we, eager);
  bool ok = memcmp(w, we, sizeof w) == 0;
  if (want) {
    uint32_t ww[24];
    fp_pack(ww, *want);
    ok = ok && memcmp(w, ww, sizeof w) == 0;
    if (!limbs_below(*want, 1u)) ok = ok && !all_zero(w); else ok = ok && all_zero(w);
  }
  WORDS(ok, "%s: wrong words, M=%d terms %zu", what, M, row.size());
}

template <int M> void run() {
  const std::vector<Fp<M>> des = designed<M>();
  const int nd = (int)des.size();
  // operand table: the designed integers, then their negatives, 7-fold negatives and random ones as the cases need them
  std::vector<Fp<M>> xs = des, craw = des, cdev;
  auto add_coeff = [&](const Fp<M>& raw) { craw.push_back(raw); return (int)craw.size() - 1; };
  Fp<M> zero, one, minus_one, t, u;
  fp_zero(zero); raw_one(one); raw_neg(minus_one, one);
  const int c_zero = 0, x_one = nd - 3;                      // the wire integer 0 as a coefficient; the constant column w_0 = 1
  std::vector<int> neg(nd), neg7(nd);
  for (int i = 0; i < nd; ++i) {
    raw_neg(t, des[i]); neg[i] = add_coeff(t);
    raw_times(t, des[i], 7); raw_neg(u, t); neg7[i] = add_coeff(u);
  }
  auto convert = [&]() { cls = SINGLE; cdev.resize(craw.size()); for (size_t i = 0; i < craw.size(); ++i) to_device(cdev[i], craw[i]); };
  convert();

  const int lengths[] = {1, 2, 3, 4, 5, 200, 201};
  for (int c = 0; c < nd; ++c)
    for (int x = 0; x < nd; ++x) {
      for (int len : lengths) {
        cls = len == 1 ? SINGLE : (len & 1 ? CHAIN_ODD : CHAIN_EVEN);
        run_row<M>(cdev, xs, std::vector<Term>((size_t)len, Term{c, x}), nullptr, "chain");
      }
      cls = ZERO;
      run_row<M>(cdev, xs, {{c, x}, {neg[c], x}}, &zero, "c - c");
      run_row<M>(cdev, xs, {{c, x}, {neg[c], x}, {c_zero, x_one}}, &zero, "c - c + 0");
      std::vector<Term> eight((size_t)7, Term{c, x});
      eight.push_back(Term{neg7[c], x});
      run_row<M>(cdev, xs, eight, &zero, "7 c - 7 c");
      // c x + c' 1 = target: the wire integer of c' is the target minus the canonical product
      cls = TARGET;
      Fp<M> prod, pc, cprime;
      fp_mul(prod, cdev[c], xs[x]); fp_canon(pc, prod);
      for (const Fp<M>* target : {&one, &minus_one}) {
        raw_neg(t, pc); raw_add(cprime, *target, t);
        const int k = add_coeff(cprime);
        cdev.resize(craw.size());
        to_device(cdev[k], craw[k]);
        // c' stands on the constant column, whose wire integer is R mod r: c' R' * R / R' = c' R -- the product IS the wire integer of c'
        run_row<M>(cdev, xs, {{c, x}, {k, x_one}}, target, "sum to a target");
      }
    }
  // random canonical operands, rows of 0 .. 9 terms and a few long ones
  cls = RANDOM;
  const int r0 = (int)xs.size(), c0 = (int)craw.size();
  for (int i = 0; i < 64; ++i) { raw_random(t); xs.push_back(t); raw_random(t); add_coeff(t); }
  cdev.resize(craw.size());
  for (size_t i = c0; i < craw.size(); ++i) to_device(cdev[i], craw[i]);
  for (int i = 0; i < 400; ++i) {
    const int len = i < 390 ? i % 10 : 190 + i;
    std::vector<Term> row;
    for (int k = 0; k < len; ++k) row.push_back(Term{c0 + (int)(rnd() % 64), r0 + (int)(rnd() % 64)});
    run_row<M>(cdev, xs, row, len ? nullptr : &zero, "random row");
  }

  // ---- the fold: partial sums as k_qap_chunks leaves them --------------------------------------------------------------------------------
  auto partial_of = [&](const std::vector<Term>& row, Fp<M>& eager) { Fp<M> acc; term_loop(acc, eager, cdev, xs, row); return acc; };
  uint32_t w[24], we[24];
  Fp<M> e, e2, fe;
  for (int c = 0; c < nd; ++c)
    for (int x = 1; x < nd; ++x) {
      // a seed and one partial, two partials, a seed and two: both parities, partials of one term and of 201
      cls = FOLD_SEED;
      const Fp<M> p1 = partial_of({{c, x}}, e), p201 = partial_of(std::vector<Term>((size_t)201, Term{c, x}), e2);
      const std::vector<std::vector<Fp<M>>> lists = {{}, {p1}, {p1, p201}, {p201, p201, p1}};
      for (const auto& parts : lists)
        for (int with_seed = 0; with_seed < 2; ++with_seed) {
          ++tallies[cls].cases;
          fold_loop<M>(w, fe, with_seed ? &des[x] : nullptr, parts);
          eager_words(we, fe);
          WORDS(memcmp(w, we, sizeof w) == 0, "fold: wrong words, M=%d partials %zu seed %d", M, parts.size(), with_seed);
        }
      // partials that are each non-zero and cancel in the fold: c x and -c x; with the seed x: -x (the coefficient -1 on the operand x)
      cls = FOLD_ZERO;
      if (c != c_zero) {
        const Fp<M> pn = partial_of({{neg[c], x}}, e), pn7 = partial_of({{neg7[c], x}}, e);
        Fp<M> chk; fp_canon(chk, p1);
        BOUND(!limbs_below(chk, 1u), "designed partial is zero, M=%d", M);
        const Fp<M> p7 = partial_of(std::vector<Term>((size_t)7, Term{c, x}), e);
        const std::vector<std::vector<Fp<M>>> cancel = {{p1, pn}, {p7, pn7}, {p1, p1, p1, p1, p1, p1, p1, pn7}};
        for (const auto& parts : cancel) {
          ++tallies[cls].cases;
          fold_loop<M>(w, fe, nullptr, parts);
          WORDS(all_zero(w), "fold: partials that cancel do not give zero words, M=%d", M);
        }
      }
      {
        // seed x and the partial of (-1) x: the cancelled seed
        const Fp<M> pm = partial_of({{neg[x_one], x}}, e);
        ++tallies[cls].cases;
        fold_loop<M>(w, fe, &des[x], {pm});
        WORDS(all_zero(w), "fold: the cancelled seed does not give zero words, M=%d", M);
      }
    }
  // chains of partials at the top of the range, with and without a seed, even and odd
  cls = FOLD_CHAIN;
  for (int c : {2, 10, nd - 1})
    for (int x : {2, 9}) {
      const Fp<M> p = partial_of(std::vector<Term>((size_t)201, Term{c, x}), e);
      for (int n : {200, 201})
        for (int with_seed = 0; with_seed < 2; ++with_seed) {
          ++tallies[cls].cases;
          fold_loop<M>(w, fe, with_seed ? &des[2] : nullptr, std::vector<Fp<M>>((size_t)n, p));
          eager_words(we, fe);
          WORDS(memcmp(w, we, sizeof w) == 0, "fold: chain, wrong words, M=%d n %d seed %d", M, n, with_seed);
        }
    }
  const Maxima<M>& mx = maxima<M>();
  printf("M=%d maxima: product %.3f r, pending accumulator %.3f r (limb %.3f 2^28, |q| %d), fold pending %.3f r (limb %.3f 2^28, |q| %d)\n", M,
         per_mille(mx.product) / 1000.0, per_mille(mx.pending) / 1000.0, mx.limb / 268435456.0, mx.q, per_mille(mx.fold_pending) / 1000.0,
         mx.fold_limb / 268435456.0, mx.fold_q);
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--mutant") && i + 1 < argc) mutant = atoi(argv[++i]);
    else { printf("usage: host_r1cs_check [--mutant 1|2|3]\n"); return 2; }
  }
  if (mutant < 0 || mutant > 3) { printf("usage: host_r1cs_check [--mutant 1|2|3]\n"); return 2; }
  run<MOD_A>(); run<MOD_B>();
  for (const Tally& t : tallies) printf("%-24s %7ld cases, %6ld with wrong words, %6ld bound checks failed\n", t.name, t.cases, t.words, t.bounds);
  if (bad) { printf("%d checks failed%s\n", bad, mutant ? " (a mutant: expected)" : ""); return 1; }
  printf("ALL OK\n");
  return 0;
}
