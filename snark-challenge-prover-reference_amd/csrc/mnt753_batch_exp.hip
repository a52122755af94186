// C ABI of the fixed-base batch scalar multiplication: libff's get_window_table / batch_exp / batch_exp_with_coeff / batch_to_special
// (depends/libff/libff/algebra/scalar_multiplication/multiexp.tcc:547-720) for one base point on the device.  The kernels are in
// batch_exp_kernels.hip.h, their orchestration in batch_exp_host.hpp (one instantiation per group: batch_exp_inst_*.hip); this unit
// checks arguments and dispatches.
#include <hip/hip_runtime.h>

#include <new>

#include "batch_exp_api.hpp"
#include "batch_exp_plan.hpp"
#include "common_host.hpp"

using namespace mnt753;

namespace {
void release(mnt753_fixed_base* fb) {
  for (void* q : {(void*)fb->d_table, (void*)fb->d_acc, (void*)fb->d_pre, (void*)fb->d_scaled, (void*)fb->d_in, (void*)fb->d_out})
    if (q) (void)hipFree(q);
  for (hipEvent_t e : fb->ev)
    if (e) (void)hipEventDestroy(e);
  delete fb;
}
// [a, a + na) and [b, b + nb) share a byte
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}
}  // namespace

extern "C" {

int mnt753_fixed_base_create(int curve, int group, const uint64_t* point, int window_bits, size_t tile, mnt753_fixed_base** out) {
  if (out) *out = nullptr;
  if (curve < 0 || curve > 1 || (group != MNT753_G1 && group != MNT753_G2)) return set_error(MNT753_EINVAL, "fixed_base_create: bad curve or group id");
  if (!point || !out) return set_error(MNT753_EINVAL, "fixed_base_create: null argument");
  if (window_bits != 0 && (window_bits < FB_MIN_WINDOW_BITS || window_bits > FB_MAX_WINDOW_BITS))
    return set_error(MNT753_EINVAL, "fixed_base_create: window_bits must be 0 (chosen by the library) or 2 .. 22");
  if (int rc = require_device()) return rc;
  mnt753_fixed_base* fb = new (std::nothrow) mnt753_fixed_base();
  if (!fb) return set_error(MNT753_ENOMEM, "fixed_base_create: host allocation failed");
  fb->curve = curve;
  fb->group = group;
  fb->device = current_physical_device();
  OnDevice on(fb->device);
  int rc;
  if (curve == MNT753_CURVE_MNT4753) rc = group == MNT753_G1 ? fixed_base_build_mnt4g1(fb, point, window_bits, tile) : fixed_base_build_mnt4g2(fb, point, window_bits, tile);
  else rc = group == MNT753_G1 ? fixed_base_build_mnt6g1(fb, point, window_bits, tile) : fixed_base_build_mnt6g2(fb, point, window_bits, tile);
  if (rc) {
    release(fb);
    return rc;
  }
  *out = fb;
  return 0;
}

int mnt753_fixed_base_free(mnt753_fixed_base* fb) {
  if (!fb) return 0;
  OnDevice on(fb->device);
  (void)hipDeviceSynchronize();
  release(fb);
  return 0;
}

int mnt753_fixed_base_plan(const mnt753_fixed_base* fb, int out[4]) {
  if (!fb || !out) return set_error(MNT753_EINVAL, "fixed_base_plan: null argument");
  out[0] = fb->w;
  out[1] = fb->W;
  out[2] = (int)fb->B;
  out[3] = (int)fb->T;
  return 0;
}

size_t mnt753_fixed_base_table_bytes(const mnt753_fixed_base* fb) { return fb ? fb->table_bytes : 0; }

int mnt753_fixed_base_last_timing(mnt753_fixed_base* fb, float out_ms[3]) {
  if (!fb || !out_ms) return set_error(MNT753_EINVAL, "fixed_base_last_timing: null argument");
  out_ms[0] = fb->build_ms;
  out_ms[1] = out_ms[2] = 0.f;
  if (!fb->timed) return 0;
  OnDevice on(fb->device);
  HIP_TRY(hipEventSynchronize(fb->ev[2]));
  HIP_TRY(hipEventElapsedTime(&out_ms[1], fb->ev[0], fb->ev[1]));
  HIP_TRY(hipEventElapsedTime(&out_ms[2], fb->ev[1], fb->ev[2]));
  return 0;
}

int mnt753_batch_exp(mnt753_fixed_base* fb, const uint64_t* scalars, int scalars_on_device, size_t n, const uint64_t* host_coeff, uint64_t* out_affine,
                     int out_on_device, void* stream) {
  if (!fb) return set_error(MNT753_EINVAL, "batch_exp: null object");
  if (n && (!scalars || !out_affine)) return set_error(MNT753_EINVAL, "batch_exp: null argument");
  const size_t aw = mnt753_affine_words(fb->curve, fb->group);
  if (n > ((size_t)1 << 40)) return set_error(MNT753_EINVAL, "batch_exp: n out of range");
  if (n && !scalars_on_device == !out_on_device && overlap(scalars, 96 * n, out_affine, 8 * aw * n))
    return set_error(MNT753_EINVAL, "batch_exp: out_affine overlaps the scalars");
  if (int rc = require_device()) return rc;
  if (n == 0) return 0;
  OnDevice on(fb->device);
  hipStream_t st = (hipStream_t)stream;
  if (fb->curve == MNT753_CURVE_MNT4753)
    return fb->group == MNT753_G1 ? batch_exp_mnt4g1(fb, scalars, scalars_on_device, n, host_coeff, out_affine, out_on_device, st)
                                  : batch_exp_mnt4g2(fb, scalars, scalars_on_device, n, host_coeff, out_affine, out_on_device, st);
  return fb->group == MNT753_G1 ? batch_exp_mnt6g1(fb, scalars, scalars_on_device, n, host_coeff, out_affine, out_on_device, st)
                                : batch_exp_mnt6g2(fb, scalars, scalars_on_device, n, host_coeff, out_affine, out_on_device, st);
}

}  // extern "C"
