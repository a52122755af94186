// Input validation on the device: are the points of a parameter file on their curve, are coordinates and scalars canonical, does a
// witness satisfy its constraint system.  The reference prover checks none of this on its hot path (prover_reference_functions.cpp:48-116
// reads with unchecked fread); what it has for the purpose is libff's is_well_formed() per group
// (depends/libff/libff/algebra/curves/mnt753/mnt4753/mnt4753_g1.cpp:348, mnt4753_g2.cpp:371-396, mnt6753_g1.cpp:348, mnt6753_g2.cpp:377:
// the curve equation, no subgroup test) and r1cs_constraint_system::is_satisfied, asserted before a witness is mapped
// (libsnark/reductions/r1cs_to_qap/r1cs_to_qap.tcc:216).  The three kernels here are those checks on WIRE-format words in device
// memory (12 u64 per base-field element, Montgomery R = 2^768 -- what the files hold and mnt753_load_file_to_device leaves there).
//
// Shape of every kernel: one lane per element (for G2 the one-lane Karatsuba extension fields of curve753.hip.h -- these are not
// throughput kernels: three orders of magnitude fewer products than a proof), ONE inlined instance of the multiplier per kernel (a step
// loop; DESIGN.md 4.2: every further instance is ~14 KB of straight-line code), and a report record {number of bad elements, lowest
// bad index with its reason} that does not depend on scheduling: a lane's verdict is a key (index << 2 | reason, all ones = good);
// the count and the minimum key are reduced per wave (ballot; indices grow with the lane, so the lowest set lane holds the wave's
// minimum) and per workgroup (LDS), and a workgroup that found something issues ONE 64-bit atomic add and ONE 64-bit atomic min --
// "every element is bad" on 2^20 elements is 4096 atomics on the record, not 2^20.  The minimum of the keys is the lowest bad index,
// and its low bits are that index's reason.
#include <hip/hip_runtime.h>

#include "common_host.hpp"
#include "curve753.hip.h"

using namespace mnt753;

namespace {
struct Report {
  unsigned long long n_bad, key;
};
constexpr unsigned long long KEY_GOOD = ~0ull;

__global__ void k_report_init(Report* rec) {
  rec->n_bad = 0;
  rec->key = KEY_GOOD;
}

__device__ __forceinline__ void load24(uint32_t w[24], const uint32_t* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const uint4 v = q[i];
    w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
  }
}
// the 768-bit integer of the wire words is >= the modulus (fp_unpack would drop its bits above 2^756: this looks at all of them)
template <int M>
__device__ __forceinline__ bool wire_ge_modulus(const uint32_t w[24]) {
  uint32_t borrow = 0;
#pragma unroll
  for (int j = 0; j < 24; ++j) {
    const uint32_t pj = (uint32_t)(FPC[M].p64[j >> 1] >> (32 * (j & 1)));
    const uint64_t t = (uint64_t)w[j] - pj - borrow;
    borrow = (uint32_t)(t >> 63);
  }
  return borrow == 0;
}
// reason != 0: element `index` is bad.  Called by all 256 threads of the workgroup.
__device__ __forceinline__ void block_report(uint32_t reason, uint64_t index, Report* rec) {
  __shared__ unsigned long long s_cnt[4], s_key[4];
  const unsigned long long key = ((unsigned long long)index << 2) | reason;
  const unsigned long long bad = __ballot(reason != 0);
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  if (lane == 0) {
    s_cnt[wave] = (unsigned long long)__popcll(bad);
    if (!bad) s_key[wave] = KEY_GOOD;
  }
  if (bad && lane == __ffsll(bad) - 1) s_key[wave] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long cnt = 0, mn = KEY_GOOD;
#pragma unroll
    for (int k = 0; k < 4; ++k) { cnt += s_cnt[k]; mn = s_key[k] < mn ? s_key[k] : mn; }
    if (cnt) {
      atomicAdd(&rec->n_bad, cnt);
      atomicMin(&rec->key, mn);
    }
  }
}

// the coefficient b (G1) / b' (twist) of group C in device form
template <class C>
__device__ __forceinline__ void curve_b(typename C::F::E& r) {
  using F = typename C::F;
  constexpr int curve = F::MOD == MOD_B ? CURVE_MNT4753 : CURVE_MNT6753;   // Fq of MNT4753 is modulus B
  if constexpr (F::DEG == 1) {
    fp_const_limbs(r, CURVE_B[curve].g1);
  } else {
#pragma unroll
    for (int k = 0; k < F::DEG; ++k) fp_const_limbs(F::comp(r, k), CURVE_B[curve].g2[k]);
  }
}

// Per point, the first that applies: a coordinate component >= q -> MNT753_BAD_NONCANONICAL; all words of y zero -> the identity
// (serialization.hpp:84-111 decodes it to G::zero() whatever x holds), well formed; y^2 != x^3 + a x + b (on the twist: a', b') ->
// MNT753_BAD_OFF_CURVE.  Five products of the coordinate field through one multiplier: x and y into the device radix (a product with
// (k_in, 0[, 0]): fp_from_wire through the field's own multiplier), x^2, x^2 x, y^2; both sides are lazy values in [0, 2q) and are
// compared as difference == 0 or q per component (F::is_zero).  A non-canonical point runs through the same arithmetic on whatever its
// low 756 bits hold -- integer operations only, the verdict is already fixed.
template <class C>
__global__ void __launch_bounds__(256) k_check_points(const uint32_t* __restrict__ wire, size_t n, Report* __restrict__ rec) {
  using F = typename C::F;
  using E = typename F::E;
  constexpr int M = F::MOD, DEG = F::DEG;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  const uint32_t* src = wire + (size_t)48 * DEG * (live ? i : n - 1);   // lanes behind the end re-read the last point and report nothing
  E X, Y, K, xx, rhs, yy, a, b, r;
  bool noncanon = false;
  uint32_t yor = 0;
#pragma unroll
  for (int k = 0; k < 2 * DEG; ++k) {
    uint32_t w[24];
    load24(w, src + 24 * k);
    noncanon |= wire_ge_modulus<M>(w);
    if (k >= DEG) {
#pragma unroll
      for (int j = 0; j < 24; ++j) yor |= w[j];
    }
    fp_unpack(F::comp(k < DEG ? X : Y, k % DEG), w);
  }
  F::zero(K);
  fp_const_limbs(F::comp(K, 0), FPC[M].k_in);
#pragma nounroll
  for (int step = 0; step < 5; ++step) {
    switch (step) {
      case 0: a = X; b = K; break;
      case 1: a = Y; b = K; break;
      case 2: a = X; b = X; break;
      case 3: a = xx; b = X; break;
      default: a = Y; b = Y; break;
    }
    F::mul(r, a, b);
    switch (step) {
      case 0: X = r; break;
      case 1: Y = r; break;
      case 2: xx = r; break;
      case 3: {
        E ax, cb;
        C::mul_by_a(ax, X);
        curve_b<C>(cb);
        F::add(rhs, r, ax);
        F::add(rhs, rhs, cb);
      } break;
      default: yy = r; break;
    }
  }
  E d;
  F::sub(d, yy, rhs);
  uint32_t reason = MNT753_BAD_NONE;
  if (live) {
    if (noncanon) reason = MNT753_BAD_NONCANONICAL;
    else if (yor != 0 && !F::is_zero(d)) reason = MNT753_BAD_OFF_CURVE;
  }
  block_report(reason, i, rec);
}

// n elements of the field with modulus M: bad = the stored integer is >= the modulus
template <int M>
__global__ void __launch_bounds__(256) k_check_scalars(const uint32_t* __restrict__ wire, size_t n, Report* __restrict__ rec) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  uint32_t w[24];
  load24(w, wire + (size_t)24 * (live ? i : n - 1));
  block_report(live && wire_ge_modulus<M>(w) ? MNT753_BAD_NONCANONICAL : MNT753_BAD_NONE, i, rec);
}

// a[i] b[i] == c[i] (mod r), i < n, on wire words: the row of r1cs_constraint_system::is_satisfied.  Any words below 2^768 get the
// right verdict: a row with an operand >= r is MNT753_BAD_NONCANONICAL (tested first, on all 768 bits), otherwise the operands are
// canonical and two products decide: mul'(a R, b R) = a b R 2^12 and mul'(c R, 2^768 mod r) = c R 2^12 (mul' = product / 2^756, k_out is
// 2^768 mod r), both in [0, 2r), equal mod r iff their difference is 0 or r -> else MNT753_BAD_UNSATISFIED.
template <int M>
__global__ void __launch_bounds__(256) k_check_products(const uint32_t* __restrict__ wa, const uint32_t* __restrict__ wb, const uint32_t* __restrict__ wc,
                                                       size_t n, Report* __restrict__ rec) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  const size_t at = (size_t)24 * (live ? i : n - 1);
  Fp<M> A, B, Cc, K, x, y, r, ab;
  bool noncanon = false;
  {
    uint32_t w[24];
    load24(w, wa + at); noncanon |= wire_ge_modulus<M>(w); fp_unpack(A, w);
    load24(w, wb + at); noncanon |= wire_ge_modulus<M>(w); fp_unpack(B, w);
    load24(w, wc + at); noncanon |= wire_ge_modulus<M>(w); fp_unpack(Cc, w);
  }
  fp_const_limbs(K, FPC[M].k_out);
#pragma nounroll
  for (int step = 0; step < 2; ++step) {
    if (step == 0) { x = A; y = B; } else { x = Cc; y = K; }
    fp_mul(r, x, y);
    if (step == 0) ab = r;
  }
  Fp<M> d;
  fp_sub(d, ab, r);
  uint32_t reason = MNT753_BAD_NONE;
  if (live) {
    if (noncanon) reason = MNT753_BAD_NONCANONICAL;
    else if (!fp_is_zero(d)) reason = MNT753_BAD_UNSATISFIED;
  }
  block_report(reason, i, rec);
}

// the report record on the device, and input that arrives in host memory
struct Scratch {
  Report* rec = nullptr;
  void* staged = nullptr;
  ~Scratch() {
    if (rec) (void)hipFree(rec);
    if (staged) (void)hipFree(staged);
  }
};
int begin(Scratch& s, hipStream_t st) {
  if (hipMalloc(&s.rec, sizeof(Report)) != hipSuccess) { (void)hipGetLastError(); return set_error(MNT753_ENOMEM, "check: device allocation failed"); }
  hipLaunchKernelGGL(k_report_init, dim3(1), dim3(1), 0, st, s.rec);
  HIP_TRY(hipGetLastError());
  return 0;
}
int stage(Scratch& s, const uint64_t*& ptr, size_t bytes) {
  if (hipMalloc(&s.staged, bytes) != hipSuccess) { (void)hipGetLastError(); return set_error(MNT753_ENOMEM, "check: device allocation failed"); }
  HIP_TRY(hipMemcpy(s.staged, ptr, bytes, hipMemcpyHostToDevice));
  ptr = reinterpret_cast<const uint64_t*>(s.staged);
  return 0;
}
int finish(Scratch& s, hipStream_t st, mnt753_check_report* out) {
  HIP_TRY(hipGetLastError());
  Report host;
  HIP_TRY(hipMemcpyAsync(&host, s.rec, sizeof(host), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  out->n_bad = host.n_bad;
  out->first_bad = host.n_bad ? (uint64_t)(host.key >> 2) : 0;
  out->first_reason = host.n_bad ? (uint32_t)(host.key & 3u) : (uint32_t)MNT753_BAD_NONE;
  out->reserved = 0;
  return 0;
}
unsigned grid_of(size_t n) { return (unsigned)((n + 255) / 256); }
constexpr size_t MAX_N = (size_t)1 << 38;   // keys are index << 2 | reason and the grid is n / 256 workgroups
}  // namespace

extern "C" {

int mnt753_check_points(int curve, int group, const uint64_t* affine, int on_device, size_t n, mnt753_check_report* out, void* stream) {
  if (curve < 0 || curve > 1 || (group != MNT753_G1 && group != MNT753_G2) || !out || (n && !affine) || n > MAX_N)
    return set_error(MNT753_EINVAL, "check_points: bad argument");
  if (int rc = require_device()) return rc;
  *out = mnt753_check_report{0, 0, MNT753_BAD_NONE, 0};
  if (!n) return 0;
  hipStream_t st = (hipStream_t)stream;
  Scratch s;
  if (!on_device) { if (int rc = stage(s, affine, 8 * n * mnt753_affine_words(curve, group))) return rc; }
  if (int rc = begin(s, st)) return rc;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(affine);
  const dim3 g(grid_of(n)), b(256);
  if (curve == MNT753_CURVE_MNT4753) {
    if (group == MNT753_G1) hipLaunchKernelGGL((k_check_points<Mnt4G1>), g, b, 0, st, w, n, s.rec);
    else hipLaunchKernelGGL((k_check_points<Mnt4G2>), g, b, 0, st, w, n, s.rec);
  } else {
    if (group == MNT753_G1) hipLaunchKernelGGL((k_check_points<Mnt6G1>), g, b, 0, st, w, n, s.rec);
    else hipLaunchKernelGGL((k_check_points<Mnt6G2>), g, b, 0, st, w, n, s.rec);
  }
  return finish(s, st, out);
}

int mnt753_check_scalars(int curve, const uint64_t* fr, int on_device, size_t n, mnt753_check_report* out, void* stream) {
  if (curve < 0 || curve > 1 || !out || (n && !fr) || n > MAX_N) return set_error(MNT753_EINVAL, "check_scalars: bad argument");
  if (int rc = require_device()) return rc;
  *out = mnt753_check_report{0, 0, MNT753_BAD_NONE, 0};
  if (!n) return 0;
  hipStream_t st = (hipStream_t)stream;
  Scratch s;
  if (!on_device) { if (int rc = stage(s, fr, 96 * n)) return rc; }
  if (int rc = begin(s, st)) return rc;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(fr);
  if (curve == MNT753_CURVE_MNT4753) hipLaunchKernelGGL((k_check_scalars<MOD_A>), dim3(grid_of(n)), dim3(256), 0, st, w, n, s.rec);
  else hipLaunchKernelGGL((k_check_scalars<MOD_B>), dim3(grid_of(n)), dim3(256), 0, st, w, n, s.rec);
  return finish(s, st, out);
}

int mnt753_check_products(int curve, const uint64_t* dev_a, const uint64_t* dev_b, const uint64_t* dev_c, size_t n, mnt753_check_report* out, void* stream) {
  if (curve < 0 || curve > 1 || !out || (n && (!dev_a || !dev_b || !dev_c)) || n > MAX_N) return set_error(MNT753_EINVAL, "check_products: bad argument");
  if (int rc = require_device()) return rc;
  *out = mnt753_check_report{0, 0, MNT753_BAD_NONE, 0};
  if (!n) return 0;
  hipStream_t st = (hipStream_t)stream;
  Scratch s;
  if (int rc = begin(s, st)) return rc;
  const uint32_t *a = reinterpret_cast<const uint32_t*>(dev_a), *b = reinterpret_cast<const uint32_t*>(dev_b), *c = reinterpret_cast<const uint32_t*>(dev_c);
  if (curve == MNT753_CURVE_MNT4753) hipLaunchKernelGGL((k_check_products<MOD_A>), dim3(grid_of(n)), dim3(256), 0, st, a, b, c, n, s.rec);
  else hipLaunchKernelGGL((k_check_products<MOD_B>), dim3(grid_of(n)), dim3(256), 0, st, a, b, c, n, s.rec);
  return finish(s, st, out);
}

}  // extern "C"
