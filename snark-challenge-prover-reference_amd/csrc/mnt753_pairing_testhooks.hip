// TEST INFRASTRUCTURE (libmnt753_hip_test.so, include/mnt753_hip_test.h) -- not linked into the product library.
// The tower of tower753.hip.h and the two halves of the pairing (pairing_kernels.hip.h) exposed element-wise, in the one-lane and in
// the lane-split form, so that tests/test_pairing_gpu.py can pin them against the Python-integer model (tests/pairing_ref.py): an
// error in the Miller loop that the final exponentiation happens to map to the right GT element still shows in the unreduced value.
// mnt753_test_fold_parts hands out the parts of the folded verification (csrc/mnt753_fold.hip) the same way.
#include <hip/hip_runtime.h>

#include "common_host.hpp"
#include "../../include/mnt753_hip_test.h"
#include "fold_api.hpp"
#include "fold_locate_api.hpp"
#include "pairing_kernels.hip.h"
#include "vk_inputs_api.hpp"

using namespace mnt753;

namespace {
struct DevBuf {   // freed on every path out of a hook
  uint32_t* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};

// op: 0 a b, 1 a^2, 2 a^-1 (0 -> 0), 3 the unitary inverse, 4 a^|w0|, 5 the final exponentiation of a, 10 + i: a^(q^i)
template <class C>
__global__ void __launch_bounds__(256, 1) k_tower_op(int op, const uint32_t* __restrict__ a_wire, const uint32_t* __restrict__ b_wire,
                                                    uint32_t* __restrict__ out_wire, uint32_t n) {
  using F = typename C::F;
  using T = Tower<F>;
  constexpr int HW = 24 * F::DEG;   // wire words of one half
  const uint32_t t = logical_lane<F>();
  if (t == 0xffffffffu || t >= n) return;
  typename T::E a, b, r;
  wire_load<F>(a.c0, a_wire + (size_t)t * 2 * HW); wire_load<F>(a.c1, a_wire + (size_t)t * 2 * HW + HW);
  wire_load<F>(b.c0, b_wire + (size_t)t * 2 * HW); wire_load<F>(b.c1, b_wire + (size_t)t * 2 * HW + HW);
  switch (op) {
    case 0: T::mul(r, a, b); break;
    case 1: T::sqr(r, a); break;
    case 2: T::inv(r, a); break;
    case 3: T::unitary_inverse(r, a); break;
    case 4: T::pow(r, a, PAIRC[Ate<C>::CURVE].w0_abs, PAIRC[Ate<C>::CURVE].w0_bits); break;
    case 5: Ate<C>::final_exponentiation(r, a); break;
    case 11: T::template frobenius<1>(r, a); break;
    case 12: T::template frobenius<2>(r, a); break;
    case 13: T::template frobenius<3>(r, a); break;
    case 14: T::template frobenius<4>(r, a); break;
    default: T::template frobenius<5>(r, a); break;
  }
  wire_store<F>(out_wire + (size_t)t * 2 * HW, r.c0);
  wire_store<F>(out_wire + (size_t)t * 2 * HW + HW, r.c1);
}

template <class C>
int run_tower_op(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
  using F = typename C::F;
  const size_t bytes = 8 * 24 * (size_t)F::DEG * n;
  DevBuf da, db, dout;
  HIP_TRY(hipMalloc(&da.p, bytes)); HIP_TRY(hipMalloc(&db.p, bytes)); HIP_TRY(hipMalloc(&dout.p, bytes));
  HIP_TRY(hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(db.p, b, bytes, hipMemcpyHostToDevice));
  hipLaunchKernelGGL((k_tower_op<C>), dim3(blocks_for<F>(n)), dim3(256), 0, 0, op, da.p, db.p, dout.p, (uint32_t)n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
  return 0;
}

// the unreduced Miller value of n pairs (neither argument the identity)
template <class C>
int run_miller(const uint64_t* g1, const uint64_t* g2, size_t n, uint64_t* out) {
  using F = typename C::F;
  const size_t b1 = 8 * 24 * n, b2 = 8 * 24 * (size_t)F::DEG * n;
  DevBuf d1, d2, dout;
  HIP_TRY(hipMalloc(&d1.p, b1)); HIP_TRY(hipMalloc(&d2.p, b2)); HIP_TRY(hipMalloc(&dout.p, b2));
  HIP_TRY(hipMemcpy(d1.p, g1, b1, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d2.p, g2, b2, hipMemcpyHostToDevice));
  hipLaunchKernelGGL((k_pairing<C>), dim3(blocks_for<F>(n)), dim3(256), 0, 0, d1.p, d2.p, d1.p, d2.p, dout.p, (uint32_t)n, 1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout.p, b2, hipMemcpyDeviceToHost));
  return 0;
}

// one half of the subgroup test on n points of the twist: psi(P) (what = 0) or [t - 1] P (what = 1), in the lane-split form
template <class C>
int run_subgroup_half(int what, const uint64_t* g2, size_t n, uint64_t* out) {
  using F = typename C::F;
  const size_t bytes = 8 * 24 * (size_t)F::DEG * n;
  DevBuf din, dout;
  HIP_TRY(hipMalloc(&din.p, bytes)); HIP_TRY(hipMalloc(&dout.p, bytes));
  HIP_TRY(hipMemcpy(din.p, g2, bytes, hipMemcpyHostToDevice));
  hipLaunchKernelGGL((k_g2_subgroup_half<C>), dim3(blocks_for<F>(n)), dim3(256), 0, 0, what, din.p, dout.p, (uint32_t)n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
  return 0;
}
int subgroup_half(const char* name, int what, int curve, const uint64_t* g2_affine, size_t n, uint64_t* out) {
  if (curve < 0 || curve > 1 || (n && (!g2_affine || !out)) || n > 0xffffffu) return set_error(MNT753_EINVAL, name);
  if (int rc = require_device()) return rc;
  if (n == 0) return 0;
  return curve == MNT753_CURVE_MNT4753 ? run_subgroup_half<Mnt4G2S>(what, g2_affine, n, out) : run_subgroup_half<Mnt6G2S>(what, g2_affine, n, out);
}
}  // namespace

extern "C" int mnt753_test_g2_endomorphism(int curve, const uint64_t* g2_affine, size_t n, uint64_t* out_affine) {
  return subgroup_half("test_g2_endomorphism: bad argument", 0, curve, g2_affine, n, out_affine);
}
extern "C" int mnt753_test_g2_loop_multiple(int curve, const uint64_t* g2_affine, size_t n, uint64_t* out_affine) {
  return subgroup_half("test_g2_loop_multiple: bad argument", 1, curve, g2_affine, n, out_affine);
}

extern "C" int mnt753_test_tower_op(int curve, int split, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
  const int k = curve == MNT753_CURVE_MNT4753 ? 4 : 6;
  if (curve < 0 || curve > 1 || !((op >= 0 && op <= 5) || (op >= 11 && op < 10 + k)) || (n && (!a || !b || !out)) || n > 0xffffffu)
    return set_error(MNT753_EINVAL, "test_tower_op: bad argument");
  if (int rc = require_device()) return rc;
  if (n == 0) return 0;
  if (curve == MNT753_CURVE_MNT4753) return split ? run_tower_op<Mnt4G2S>(op, a, b, n, out) : run_tower_op<Mnt4G2>(op, a, b, n, out);
  return split ? run_tower_op<Mnt6G2S>(op, a, b, n, out) : run_tower_op<Mnt6G2>(op, a, b, n, out);
}

extern "C" int mnt753_test_miller_loop(int curve, int split, const uint64_t* g1_affine, const uint64_t* g2_affine, size_t n, uint64_t* out) {
  if (curve < 0 || curve > 1 || (n && (!g1_affine || !g2_affine || !out)) || n > 0xffffffu) return set_error(MNT753_EINVAL, "test_miller_loop: bad argument");
  if (int rc = require_device()) return rc;
  if (n == 0) return 0;
  if (curve == MNT753_CURVE_MNT4753) return split ? run_miller<Mnt4G2S>(g1_affine, g2_affine, n, out) : run_miller<Mnt4G2>(g1_affine, g2_affine, n, out);
  return split ? run_miller<Mnt6G2S>(g1_affine, g2_affine, n, out) : run_miller<Mnt6G2>(g1_affine, g2_affine, n, out);
}

extern "C" int mnt753_test_fold_parts(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, const uint64_t* coefficients, uint64_t* out_f,
                                      uint64_t* out_s, uint64_t* out_t, uint64_t* out_rho, uint8_t* status, int* accepted) {
  FoldParts parts;
  parts.f = out_f; parts.s = out_s; parts.t = out_t; parts.rho = out_rho;
  return groth16_verify_folded_parts(vk, proofs, inputs, n, 0, coefficients, status, accepted, nullptr, &parts);
}
extern "C" int mnt753_test_fold_segment_parts(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, const uint64_t* coefficients,
                                              uint64_t* out_f, uint64_t* out_s, uint64_t* out_t, uint64_t* out_rho, uint8_t* out_accepted, uint8_t* status,
                                              uint8_t* verdicts, mnt753_fold_locate_report* report) {
  FoldLocateParts parts;
  parts.f = out_f; parts.s = out_s; parts.t = out_t; parts.rho = out_rho; parts.accepted = out_accepted; parts.status = status;
  return groth16_verify_folded_locate_parts(vk, proofs, inputs, n, 0, coefficients, verdicts, report, nullptr, &parts);
}
extern "C" size_t mnt753_test_fold_locate_last_chunks(void) { return groth16_fold_locate_last_chunks(); }
extern "C" int mnt753_test_fold_last_timing(float out_ms[3]) {
  if (!out_ms) return set_error(MNT753_EINVAL, "test_fold_last_timing: bad argument");
  groth16_fold_last_timing(out_ms);
  return 0;
}
extern "C" int mnt753_test_vk_force_inputs_per_lane(mnt753_vk* vk, uint32_t inputs_per_lane) {
  if (!vk) return set_error(MNT753_EINVAL, "test_vk_force_inputs_per_lane: bad argument");
  vk->test_inputs_per_lane = inputs_per_lane;
  return 0;
}
extern "C" int mnt753_test_vk_set_gt(mnt753_vk* vk, const uint64_t* gt_words) {
  if (!vk || !gt_words || !vk->dev_key) return set_error(MNT753_EINVAL, "test_vk_set_gt: bad argument");
  if (int rc = require_device()) return rc;
  OnDevice guard(vk->device);
  const size_t w2 = mnt753_affine_words(vk->curve, MNT753_G2), wt = mnt753_gt_words(vk->curve);
  HIP_TRY(hipDeviceSynchronize());                   // no call on the key is reading the old words
  HIP_TRY(hipMemcpy(vk->dev_key + 24 + 2 * w2, gt_words, 8 * wt, hipMemcpyHostToDevice));
  vk->gt.assign(gt_words, gt_words + wt);
  return 0;
}
extern "C" int mnt753_test_vk_inputs_last_timing(const mnt753_vk* vk, float out_ms[3]) {
  if (!vk || !out_ms) return set_error(MNT753_EINVAL, "test_vk_inputs_last_timing: bad argument");
  return vk_inputs_last_timing(vk, out_ms, out_ms + 1, out_ms + 2);
}
