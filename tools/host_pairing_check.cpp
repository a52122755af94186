// CPU-suite harness: the tower (tower753.hip.h) and the whole reduced ate pairing (pairing_kernels.hip.h) through the ONE-LANE fields,
// compiled for the host -- the same __host__ __device__ source the device instantiates with its lane-split fields.
//   * e(alpha_g1, beta_g2) of the six committed keys (keys.bin: alpha_g1 | beta_g1 | beta_g2 | ..) equals the GT element at the head of
//     the vk.txt beside it, which the reference's own reduced_pairing wrote: every word;
//   * on seeded random tower elements: f f^-1 = 1, sqr(f) = mul(f, f), frobenius<K>(f) = f and frobenius<1> applied K times = f,
//     mul is commutative, and the unitary inverse inverts an element of the cyclotomic subgroup (a first-chunk value).
//   g++ -O1 -std=c++17 tools/host_pairing_check.cpp -o build/host_pairing_check && build/host_pairing_check      (from the repo root)
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../snark-challenge-prover-reference_amd/csrc/pairing_kernels.hip.h"
using namespace mnt753;

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

template <class F> void rand_f(typename F::E& r) {
  for (int k = 0; k < F::DEG; ++k) {
    uint32_t w[24];
    for (int i = 0; i < 24; ++i) w[i] = (uint32_t)rnd();
    w[23] &= 0xffu;                       // below 2^744 < p
    fp_from_wire(F::comp(r, k), w);
  }
}
template <class F> void f_words(uint64_t* out, const typename F::E& a) {
  for (int k = 0; k < F::DEG; ++k) fp_to_wire((uint32_t*)(out + 12 * k), F::comp(a, k));
}
template <class F> bool t_equal(const typename Tower<F>::E& a, const typename Tower<F>::E& b) {
  uint64_t x[72], y[72];
  f_words<F>(x, a.c0); f_words<F>(x + 12 * F::DEG, a.c1);
  f_words<F>(y, b.c0); f_words<F>(y + 12 * F::DEG, b.c1);
  return memcmp(x, y, 8 * 24 * F::DEG) == 0;
}

template <class C> bool tower_identities(const char* name) {
  using F = typename C::F;
  using T = Tower<F>;
  using TE = typename T::E;
  bool ok = true;
  TE one;
  T::one(one);
  for (int it = 0; it < 12 && ok; ++it) {
    TE f, g, a, b, c;
    rand_f<F>(f.c0); rand_f<F>(f.c1); rand_f<F>(g.c0); rand_f<F>(g.c1);
    T::inv(a, f); T::mul(b, a, f);
    if (!t_equal<F>(b, one)) { printf("%s: f * f^-1 != 1\n", name); ok = false; }
    T::sqr(a, f); T::mul(b, f, f);
    if (!t_equal<F>(a, b)) { printf("%s: sqr != mul\n", name); ok = false; }
    T::mul(a, f, g); T::mul(b, g, f);
    if (!t_equal<F>(a, b)) { printf("%s: mul does not commute\n", name); ok = false; }
    T::template frobenius<T::K>(a, f);
    if (!t_equal<F>(a, f)) { printf("%s: frobenius<k> is not the identity\n", name); ok = false; }
    a = f;
    for (int i = 0; i < T::K; ++i) { T::template frobenius<1>(b, a); a = b; }
    if (!t_equal<F>(a, f)) { printf("%s: frobenius<1>^k is not the identity\n", name); ok = false; }
    T::template frobenius<1>(a, f); T::template frobenius<1>(b, g); T::mul(c, a, b);
    T::mul(a, f, g); T::template frobenius<1>(b, a);
    if (!t_equal<F>(b, c)) { printf("%s: frobenius<1> is not multiplicative\n", name); ok = false; }
    T::inv(a, f);
    Ate<C>::first_chunk(b, f, a);
    T::unitary_inverse(c, b); T::mul(a, b, c);
    if (!t_equal<F>(a, one)) { printf("%s: the unitary inverse of a first-chunk value does not invert it\n", name); ok = false; }
  }
  printf("%s tower identities: %s\n", name, ok ? "OK" : "FAILED");
  return ok;
}

static bool read_file(const std::string& path, std::vector<uint64_t>& out, size_t words) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { printf("no file %s\n", path.c_str()); return false; }
  out.resize(words);
  const size_t got = fread(out.data(), 8, words, f);
  fclose(f);
  return got == words;
}

template <class C> bool key_pairing(const char* dir) {
  using F = typename C::F;
  using A = Ate<C>;
  const int D = F::DEG;
  std::vector<uint64_t> keys, head;
  const std::string base = std::string("tests/golden/") + dir;
  if (!read_file(base + "/keys.bin", keys, 48 + 24 * D) || !read_file(base + "/vk.txt", head, 24 * D)) return false;
  typename A::B px, py;
  typename A::FE qx, qy;
  fp_from_wire(px, (const uint32_t*)keys.data());
  fp_from_wire(py, (const uint32_t*)(keys.data() + 12));
  const uint64_t* beta = keys.data() + 48;
  for (int k = 0; k < D; ++k) {
    fp_from_wire(F::comp(qx, k), (const uint32_t*)(beta + 12 * k));
    fp_from_wire(F::comp(qy, k), (const uint32_t*)(beta + 12 * (D + k)));
  }
  typename A::TE r;
  A::reduced_pairing(r, px, py, qx, qy);
  uint64_t got[72];
  f_words<F>(got, r.c0);
  f_words<F>(got + 12 * D, r.c1);
  const bool ok = memcmp(got, head.data(), 8 * 24 * D) == 0;
  printf("%s e(alpha, beta): %s\n", dir, ok ? "OK" : "MISMATCH");
  return ok;
}

// ---- case files (tests/test_pairing_designed_cpu.py) --------------------------------------------------------------------------------
// host_pairing_check cases <in> <out>: the operations of mnt753_test_tower_op and mnt753_test_miller_loop through the one-lane fields.
// in:  u64 curve (0 / 1) | u64 op | u64 n | the operands in wire words: a[n] then b[n] tower elements for the tower ops (op 0 a b,
//      1 a^2, 2 a^-1, 3 the unitary inverse, 4 a^|w0|, 5 the final exponentiation, 10 + i a^(q^i)), or g1[n] then g2[n] affine
//      points for op 20, the unreduced Miller value.
// out: n tower elements in wire words.
template <class F> void f_load(typename F::E& r, const uint64_t* w) {
  for (int k = 0; k < F::DEG; ++k) fp_from_wire(F::comp(r, k), (const uint32_t*)(w + 12 * k));
}

template <class C> bool run_cases(uint64_t op, size_t n, const std::vector<uint64_t>& in, std::vector<uint64_t>& out) {
  using F = typename C::F;
  using A = Ate<C>;
  using T = Tower<F>;
  constexpr int D = F::DEG, WT = 24 * D;
  const bool miller = op == 20;
  if (!(op <= 5 || (op >= 11 && op < 10 + (uint64_t)T::K) || miller)) { printf("cases: unknown op %llu\n", (unsigned long long)op); return false; }
  const size_t wa = miller ? 24 : WT, wb = miller ? 24 * D : WT;
  if (in.size() != 3 + n * (wa + wb)) { printf("cases: %zu words for n = %zu of op %llu\n", in.size(), n, (unsigned long long)op); return false; }
  const uint64_t *pa = in.data() + 3, *pb = pa + n * wa;
  out.assign(n * WT, 0);
  for (size_t t = 0; t < n; ++t) {
    typename T::E a, b, r;
    if (miller) {
      typename A::B px, py;
      typename A::FE qx, qy;
      fp_from_wire(px, (const uint32_t*)(pa + t * wa));
      fp_from_wire(py, (const uint32_t*)(pa + t * wa + 12));
      f_load<F>(qx, pb + t * wb);
      f_load<F>(qy, pb + t * wb + 12 * D);
      typename A::Pair p[1];
      A::setup(p[0], px, py, qx, qy);
      A::template miller_loop<1>(r, p);
    } else {
      f_load<F>(a.c0, pa + t * WT); f_load<F>(a.c1, pa + t * WT + 12 * D);
      f_load<F>(b.c0, pb + t * WT); f_load<F>(b.c1, pb + t * WT + 12 * D);
      switch (op) {
        case 0: T::mul(r, a, b); break;
        case 1: T::sqr(r, a); break;
        case 2: T::inv(r, a); break;
        case 3: T::unitary_inverse(r, a); break;
        case 4: T::pow(r, a, PAIRC[A::CURVE].w0_abs, PAIRC[A::CURVE].w0_bits); break;
        case 5: A::final_exponentiation(r, a); break;
        case 11: T::template frobenius<1>(r, a); break;
        case 12: T::template frobenius<2>(r, a); break;
        case 13: T::template frobenius<3>(r, a); break;
        case 14: T::template frobenius<4>(r, a); break;
        default: T::template frobenius<5>(r, a); break;
      }
    }
    f_words<F>(out.data() + t * WT, r.c0);
    f_words<F>(out.data() + t * WT + 12 * D, r.c1);
  }
  return true;
}

static int cases_main(const char* in_path, const char* out_path) {
  FILE* f = fopen(in_path, "rb");
  if (!f) { printf("no file %s\n", in_path); return 1; }
  std::vector<uint64_t> in;
  uint64_t buf[512];
  size_t got;
  while ((got = fread(buf, 8, 512, f)) > 0) in.insert(in.end(), buf, buf + got);
  fclose(f);
  if (in.size() < 3 || in[0] > 1 || in[2] > (1u << 20)) { printf("cases: bad header\n"); return 1; }
  std::vector<uint64_t> out;
  const bool ok = in[0] == 0 ? run_cases<Mnt4G2>(in[1], (size_t)in[2], in, out) : run_cases<Mnt6G2>(in[1], (size_t)in[2], in, out);
  if (!ok) return 1;
  FILE* o = fopen(out_path, "wb");
  if (!o) { printf("cannot write %s\n", out_path); return 1; }
  const size_t put = fwrite(out.data(), 8, out.size(), o);
  if (fclose(o) != 0 || put != out.size()) { printf("short write to %s\n", out_path); return 1; }
  printf("cases: %zu results\n", (size_t)in[2]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && strcmp(argv[1], "cases") == 0) return cases_main(argv[2], argv[3]);
  if (argc != 1) { printf("usage: host_pairing_check [cases <in> <out>]\n"); return 2; }
  bool ok = true;
  ok &= tower_identities<Mnt4G2>("Fq4");
  ok &= tower_identities<Mnt6G2>("Fq6");
  for (const char* d : {"g16_mnt4", "keygen_mnt4_cut21", "keygen_mnt4_full"}) ok &= key_pairing<Mnt4G2>(d);
  for (const char* d : {"g16_mnt6", "keygen_mnt6_cut21", "keygen_mnt6_full"}) ok &= key_pairing<Mnt6G2>(d);
  printf("%s\n", ok ? "ALL OK" : "FAILURES");
  return ok ? 0 : 1;
}
