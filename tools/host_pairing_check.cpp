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

int main() {
  bool ok = true;
  ok &= tower_identities<Mnt4G2>("Fq4");
  ok &= tower_identities<Mnt6G2>("Fq6");
  for (const char* d : {"g16_mnt4", "keygen_mnt4_cut21", "keygen_mnt4_full"}) ok &= key_pairing<Mnt4G2>(d);
  for (const char* d : {"g16_mnt6", "keygen_mnt6_cut21", "keygen_mnt6_full"}) ok &= key_pairing<Mnt6G2>(d);
  printf("%s\n", ok ? "ALL OK" : "FAILURES");
  return ok ? 0 : 1;
}
