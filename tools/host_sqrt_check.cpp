// CPU-suite harness: the square root of csrc/fp_sqrt.hip.h through the base fields and the ONE-LANE extension fields, compiled for the
// host -- the same __host__ __device__ source the device instantiates with its lane-split fields (and the CPU build to take into gdb).
// Per field (Fq of both curves, Fq2 of MNT4753, Fq3 of MNT6753) and per window W = 1, 2, 4 a designed set, because random squares
// almost never reach the shallow Tonelli-Shanks depths: with c = z^t of order 2^s (the generated constant) and u random,
//   * c^(2^(s - k)) u^(2^s) for EVERY k = 0 .. s - 1: a square whose a^t has order exactly 2^k;
//   * 0, 1, -1, the element with every component q - 1;
//   * non-squares: c, c u^2, and in the extensions an element with zero c0 (its verdict from Euler's criterion);
// expected: is_square exact, r^2 = a exact, and sqrt_fix_sign gives the root of either parity.
//   g++ -O1 -std=c++17 tools/host_sqrt_check.cpp -o build/host_sqrt_check && build/host_sqrt_check      (from the repo root)
#include <cstdio>
#include <cstring>
#include <vector>
#include "../snark-challenge-prover-reference_amd/csrc/fp_sqrt.hip.h"
using namespace mnt753;

static uint64_t rng_state = 0x13198a2e03707344ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

template <class F> void rand_f(typename F::E& r) {
  for (int k = 0; k < F::DEG; ++k) {
    uint32_t w[24];
    for (int i = 0; i < 24; ++i) w[i] = (uint32_t)rnd();
    w[23] &= 0xffu;                       // below 2^744 < p
    fp_from_wire(F::comp(r, k), w);
  }
}
template <class F> bool f_equal(const typename F::E& a, const typename F::E& b) {
  uint32_t x[72], y[72];
  for (int k = 0; k < F::DEG; ++k) { fp_to_wire(x + 24 * k, F::comp(a, k)); fp_to_wire(y + 24 * k, F::comp(b, k)); }
  return memcmp(x, y, 96 * F::DEG) == 0;
}

template <class F, int W> bool run(const char* name) {
  using S = Sqrt<F>;
  using E = typename F::E;
  struct Case { E a; int square; const char* what; };   // square: 1 / 0, -1 = by Euler's criterion
  std::vector<Case> cases;
  E one, zero, c, u, t;
  F::one(one); F::zero(zero);
  S::root_of_unity(c);
  for (int k = 0; k < S::S; ++k) {
    rand_f<F>(u);
    for (int i = 0; i < S::S; ++i) S::sqr(u, u);
    t = c;
    for (int i = 0; i < S::S - k; ++i) S::sqr(t, t);
    S::mul(t, t, u);
    cases.push_back({t, 1, "depth"});
  }
  E m1, all;
  F::neg(m1, one);
  for (int k = 0; k < F::DEG; ++k) F::comp(all, k) = F::comp(m1, 0);
  cases.push_back({zero, 1, "0"});
  cases.push_back({one, 1, "1"});
  cases.push_back({m1, 1, "-1"});                    // s >= 15: -1 is a square in all four fields
  cases.push_back({all, -1, "all q - 1"});
  cases.push_back({c, 0, "z^t"});
  rand_f<F>(u); S::sqr(u, u); S::mul(t, c, u);
  cases.push_back({t, 0, "z^t u^2"});
  if (F::DEG > 1) {
    rand_f<F>(t);
    fp_zero(F::comp(t, 0));
    cases.push_back({t, -1, "zero c0"});
  }
  bool ok = true;
  int n_sq = 0;
  for (const Case& cs : cases) {
    int want = cs.square;
    if (want < 0) {                               // a^((|F| - 1) / 2) = (a^((t - 1) / 2))^2 a, squared s - 1 times
      E e;
      S::template pow_half_t<1>(e, cs.a);
      S::sqr(e, e); S::mul(e, e, cs.a);
      for (int i = 0; i < S::S - 1; ++i) S::sqr(e, e);
      want = f_equal<F>(e, one) ? 1 : 0;
    }
    E r, rr;
    bool sq = false;
    S::template sqrt<W>(r, sq, cs.a);
    if ((int)sq != want) { printf("%s W=%d %s: is_square %d, expected %d\n", name, W, cs.what, (int)sq, want); ok = false; continue; }
    if (!sq) continue;
    ++n_sq;
    S::sqr(rr, r);
    if (!f_equal<F>(rr, cs.a)) { printf("%s W=%d %s: r^2 != a\n", name, W, cs.what); ok = false; }
    if (F::is_zero(r)) continue;
    for (uint32_t par = 0; par < 2; ++par) {      // either sign on request; the root stays a root
      E y = r;
      sqrt_fix_sign<F>(y, par);
      S::sqr(rr, y);
      int first = 0;
      while (first < F::DEG - 1 && fp_is_zero(F::comp(y, first))) ++first;
      const uint32_t got = sqrt_parity(F::comp(y, first)), expect = first == 0 ? par : 0u;
      if (!f_equal<F>(rr, cs.a) || got != expect) { printf("%s W=%d %s: sign %u not honoured\n", name, W, cs.what, par); ok = false; }
    }
  }
  printf("%s W=%d: %zu cases, %d squares: %s\n", name, W, cases.size(), n_sq, ok ? "OK" : "FAILED");
  return ok;
}

template <class F> bool run_all(const char* name) { return run<F, 1>(name) & run<F, 2>(name) & run<F, 4>(name); }

int main() {
  bool ok = true;
  ok &= run_all<Mnt4G1::F>("Fq(MNT4753)");
  ok &= run_all<Mnt6G1::F>("Fq(MNT6753)");
  ok &= run_all<Mnt4G2::F>("Fq2(MNT4753)");
  ok &= run_all<Mnt6G2::F>("Fq3(MNT6753)");
  printf("%s\n", ok ? "ALL OK" : "FAILURES");
  return ok ? 0 : 1;
}
