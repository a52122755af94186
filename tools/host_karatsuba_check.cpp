// CPU-suite harness: the signed product with a Karatsuba product half (fp_mul_s_k / fp_mul_s_ip_k, fp753.hip.h) against fp_mul_s, limb
// for limb, on both moduli -- the same __host__ __device__ source the device runs.  Beside the comparison every column is recomputed
// in __int128 in the order the routine takes its parts (middle term onto the carry, u_k, then u_(k-14) + the reduction's products):
//   * the limbs of that wide model equal fp_mul_s's too (the columns are the same integers),
//   * the differences a0_i - a1_i, b1_j - b0_j fit int32, every column satisfies |column| < 2^63,
//   * and for operands inside the shipped contract (one operand limbs 0..25 in [0, 2^28), limb 26 in (-2^26, 2^28); the other
//     |limb| < 2^29) so does every PARTIAL sum of a column.  Two raw operands (|limb| < 2^29 each; no call site has them, the levels'
//     products all meet the contract) are run as well: the column bound holds there, a partial sum may pass 2^63 and is only counted.
// Inputs: 3000 seeded random pairs in the contract's ranges (and 3000 raw x raw); every limb at 0, 2^28 - 1, +-(2^29 - 1); low half at
// one extreme and high half at the other in both operands, every combination; the top limb at its negative end; the values 0, p,
// 2p - 1 on either side.  Both argument orders, both entry points.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/host_karatsuba_check.cpp -o build/host_karatsuba_check
//   build/host_karatsuba_check          (from the repo root)
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../snark-challenge-prover-reference_amd/csrc/fp753.hip.h"
using namespace mnt753;

typedef __int128 i128;
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static int32_t rnd_range(int32_t lo, int32_t hi) { return lo + (int32_t)(rnd() % (uint64_t)((int64_t)hi - lo + 1)); }   // [lo, hi]

static const i128 LIM63 = (i128)1 << 63;
static long g_bad = 0, g_pairs = 0, g_partial_wraps = 0;
static i128 g_max_col = 0, g_max_partial = 0;

static i128 iabs(i128 v) { return v < 0 ? -v : v; }
static void fail(const char* what, int mod, int k) {
  if (++g_bad < 12) printf("modulus %d: %s (column %d)\n", mod, what, k);
}

typedef std::vector<int32_t> Limbs;   // 27 signed limbs

// the routine's columns in __int128; r: the limbs they give; strict: every partial sum must stay inside int64
template <int M>
static void model(uint32_t r[NL], const Limbs& a, const Limbs& b, bool strict) {
  constexpr int H = 14, G = NL - H;
  int64_t da[H], db[H];
  for (int i = 0; i < H; ++i) {
    da[i] = (int64_t)a[i] - (i < G ? a[H + i] : 0);
    db[i] = (int64_t)(i < G ? b[H + i] : 0) - b[i];
    if (da[i] != (int32_t)da[i] || db[i] != (int32_t)db[i]) fail("an operand difference leaves int32", M, i);
  }
  i128 acc = 0, u[2 * NL];
  uint32_t m[NL];
  auto partial = [&](i128 v, int k) {
    if (strict && iabs(v) > g_max_partial) g_max_partial = iabs(v);
    if (iabs(v) >= LIM63) { if (strict) fail("a partial sum leaves int64 inside the contract", M, k); else ++g_partial_wraps; }
  };
  for (int k = 0; k < 2 * NL - 1; ++k) {
    const int j = k - H;
    i128 uk = 0, md = 0, mp = 0, plain = 0;
    for (int i = 0; i < H; ++i) if (k - i >= 0 && k - i < H) uk += (i128)a[i] * b[k - i];
    if (j >= 0) for (int i = 0; i < G; ++i) if (j - i >= 0 && j - i < G) uk += (i128)a[H + i] * b[H + j - i];
    if (j >= 0) for (int i = 0; i < H; ++i) if (j - i >= 0 && j - i < H) md += (i128)da[i] * db[j - i];
    u[k] = uk;
    for (int i = 0; i < NL; ++i) if (k - i >= 0 && k - i < NL) plain += (i128)a[i] * b[k - i];
    if (plain != uk + (j >= 0 ? u[j] + md : 0)) fail("the three parts do not add up to the schoolbook column", M, k);
    partial(uk, k);
    acc += md; partial(acc, k);
    acc += uk; partial(acc, k);
    i128 acc2 = j >= 0 ? u[j] : 0;
    for (int i = 0; i < NL; ++i) if (k - i >= 1 && k - i < NL) mp += (i128)m[i] * FPC[M].p[k - i];
    acc2 += mp; partial(acc2, k);
    acc += acc2; partial(acc, k);
    if (k < NL) {
      m[k] = ((uint32_t)(uint64_t)acc * FPC[M].inv) & LMASK;
      acc += (i128)m[k] * FPC[M].p[0];
      partial(acc, k);
      if ((uint64_t)acc & LMASK) fail("a reduced column is not a multiple of 2^28", M, k);
    } else {
      r[k - NL] = (uint32_t)(uint64_t)acc & LMASK;
    }
    if (iabs(acc) >= LIM63) fail("|column| >= 2^63", M, k);
    if (iabs(acc) > g_max_col) g_max_col = iabs(acc);
    acc >>= LB;
  }
  r[NL - 1] = (uint32_t)(int64_t)acc;
}

template <int M>
static void to_fp(Fp<M>& r, const Limbs& v) { for (int i = 0; i < NL; ++i) r.l[i] = (uint32_t)v[i]; }

template <int M>
static void one_pair(const Limbs& a, const Limbs& b, bool strict) {
  Fp<M> fa, fb, want, got, ipb, ipa;
  uint32_t wide[NL];
  to_fp(fa, a); to_fp(fb, b);
  fp_mul_s(want, fa, fb);
  fp_mul_s_k(got, fa, fb);
  ipa = fa; ipb = fb;
  fp_mul_s_ip_k(ipb, ipa);
  model<M>(wide, a, b, strict);
  if (memcmp(got.l, want.l, sizeof want.l)) fail("fp_mul_s_k differs from fp_mul_s", M, -1);
  if (memcmp(ipb.l, want.l, sizeof want.l)) fail("fp_mul_s_ip_k differs from fp_mul_s", M, -1);
  if (memcmp(ipa.l, fa.l, sizeof fa.l)) fail("fp_mul_s_ip_k changed the operand it keeps", M, -1);
  if (memcmp(wide, want.l, sizeof want.l)) fail("the __int128 columns differ from fp_mul_s", M, -1);
  ++g_pairs;
}
// both argument orders
template <int M>
static void both(const Limbs& n, const Limbs& r, bool strict) { one_pair<M>(n, r, strict); one_pair<M>(r, n, strict); }

template <int M>
static Limbs value_limbs(int what) {   // 0: zero, 1: p, 2: 2p - 1
  Limbs v(NL, 0);
  if (what == 1) for (int i = 0; i < NL; ++i) v[i] = (int32_t)FPC[M].p[i];
  if (what == 2) { for (int i = 0; i < NL; ++i) v[i] = (int32_t)FPC[M].p2[i]; v[0] -= 1; }   // 2p is even and not 0 mod 2^28
  return v;
}
static Limbs halves(int32_t low, int32_t high) {
  Limbs v(NL);
  for (int i = 0; i < NL; ++i) v[i] = i < 14 ? low : high;
  return v;
}

template <int M>
static void run() {
  const int32_t n_max = (1 << 28) - 1, r_max = (1 << 29) - 1, top_min = -(1 << 26) + 1;
  // normalised side: constant limbs, the halves at opposite extremes, the top limb at its negative end, the three values
  std::vector<Limbs> N = {halves(0, 0), halves(n_max, n_max), halves(n_max, 0), halves(0, n_max)};
  for (int32_t low : {0, n_max}) for (int32_t high : {0, n_max}) { Limbs v = halves(low, high); v[NL - 1] = top_min; N.push_back(v); }
  for (int w = 0; w < 3; ++w) N.push_back(value_limbs<M>(w));
  // raw side: constant limbs at 0, 2^28 - 1, +-(2^29 - 1), the halves at opposite extremes, alternating signs, the three values
  std::vector<Limbs> R;
  for (int32_t c : {0, n_max, r_max, -r_max}) R.push_back(halves(c, c));
  R.push_back(halves(r_max, -r_max)); R.push_back(halves(-r_max, r_max));
  R.push_back(halves(r_max, 0)); R.push_back(halves(0, r_max)); R.push_back(halves(-r_max, 0)); R.push_back(halves(0, -r_max));
  { Limbs v(NL); for (int i = 0; i < NL; ++i) v[i] = (i & 1) ? r_max : -r_max; R.push_back(v); for (auto& x : v) x = -x; R.push_back(v); }
  for (int w = 0; w < 3; ++w) R.push_back(value_limbs<M>(w));
  for (const Limbs& n : N) for (const Limbs& r : R) both<M>(n, r, true);
  for (const Limbs& r1 : R) for (const Limbs& r2 : R) one_pair<M>(r1, r2, false);        // raw x raw: the column bound alone
  for (int t = 0; t < 3000; ++t) {
    Limbs n(NL), r(NL), r2(NL);
    const int shape = t % 3;           // 0: any limbs in range; 1: a lazy element against a difference of two; 2: limbs near the ends
    for (int i = 0; i < NL; ++i) {
      if (shape == 2) {
        n[i] = (rnd() & 1) ? n_max - (int32_t)(rnd() & 7) : (int32_t)(rnd() & 7);
        r[i] = ((rnd() & 1) ? 1 : -1) * (r_max - (int32_t)(rnd() & 7));
      } else {
        n[i] = rnd_range(0, n_max);
        r[i] = shape == 0 ? rnd_range(-r_max, r_max) : rnd_range(0, n_max) - rnd_range(0, n_max);
      }
      r2[i] = rnd_range(-r_max, r_max);
    }
    n[NL - 1] = shape == 1 ? rnd_range(top_min, 1 << 26) : rnd_range(top_min, n_max);
    both<M>(n, r, true);
    one_pair<M>(r, r2, false);
  }
}

int main() {
  run<MOD_A>();
  run<MOD_B>();
  printf("%ld products checked on two moduli; largest |column| 2^63 x %.4f, largest |partial sum| inside the contract 2^63 x %.4f,\n"
         "  %ld partial sums beyond int64 (raw x raw only: they wrap and the column is still exact)\n",
         g_pairs, (double)g_max_col / 9223372036854775808.0, (double)g_max_partial / 9223372036854775808.0, g_partial_wraps);
  if (g_bad) { printf("FAILED: %ld mismatches or range violations\n", g_bad); return 1; }
  printf("ALL OK\n");
  return 0;
}
