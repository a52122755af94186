// TEST INFRASTRUCTURE (libmnt753_hip_test.so, include/mnt753_hip_test.h) -- not linked into the product library.
// The square root of fp_sqrt.hip.h on raw field elements, with the lane mapping of the product's k_decompress (one lane per base-field
// element, one lane group per Fq2 / Fq3 element), so that tests/test_compress_gpu.py reaches every Tonelli-Shanks depth with designed
// elements, and with the window of the fixed exponent as an argument, so that tools/bench_compress.py can time the alternatives.
#include <hip/hip_runtime.h>

#include "common_host.hpp"
#include "../../include/mnt753_hip_test.h"
#include "compress_kernels.hip.h"

using namespace mnt753;

namespace {
struct DevBuf {   // freed on every path out of a hook
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};
struct Events {
  hipEvent_t a = nullptr, b = nullptr;
  ~Events() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

template <class F, int W>
int run_sqrt(const uint64_t* in, size_t n, uint64_t* out, uint8_t* is_square, float* ms) {
  const size_t bytes = 96 * (size_t)F::DEG * n;
  DevBuf din, dout, dsq;
  Events ev;
  HIP_TRY(hipMalloc(&din.p, bytes)); HIP_TRY(hipMalloc(&dout.p, bytes)); HIP_TRY(hipMalloc(&dsq.p, n));
  HIP_TRY(hipMemcpy(din.p, in, bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipEventCreate(&ev.a)); HIP_TRY(hipEventCreate(&ev.b));
  HIP_TRY(hipEventRecord(ev.a, 0));
  hipLaunchKernelGGL((k_field_sqrt<F, W>), dim3(blocks_for<F>(n)), dim3(256), 0, 0, reinterpret_cast<const uint32_t*>(din.p),
                     reinterpret_cast<uint32_t*>(dout.p), reinterpret_cast<uint8_t*>(dsq.p), (uint32_t)n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ev.b, 0));
  HIP_TRY(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(is_square, dsq.p, n, hipMemcpyDeviceToHost));
  if (ms) HIP_TRY(hipEventElapsedTime(ms, ev.a, ev.b));
  return 0;
}
template <class F>
int run_sqrt_w(int window, const uint64_t* in, size_t n, uint64_t* out, uint8_t* is_square, float* ms) {
  switch (window) {
    case 1: return run_sqrt<F, 1>(in, n, out, is_square, ms);
    case 2: return run_sqrt<F, 2>(in, n, out, is_square, ms);
    default: return run_sqrt<F, 4>(in, n, out, is_square, ms);
  }
}
}  // namespace

extern "C" int mnt753_test_field_sqrt_window(int curve, int deg, int window, const uint64_t* in_wire, size_t n, uint64_t* out_wire, uint8_t* is_square,
                                             float* ms) {
  const int ext = curve == MNT753_CURVE_MNT4753 ? 2 : 3;
  if (curve < 0 || curve > 1 || (deg != 1 && deg != ext) || (window != 1 && window != 2 && window != 4) || (n && (!in_wire || !out_wire || !is_square)) ||
      n > 0xffffffu)
    return set_error(MNT753_EINVAL, "test_field_sqrt: bad argument");
  if (int rc = require_device()) return rc;
  if (ms) *ms = 0.0f;
  if (n == 0) return 0;
  if (curve == MNT753_CURVE_MNT4753)
    return deg == 1 ? run_sqrt_w<Mnt4G1::F>(window, in_wire, n, out_wire, is_square, ms) : run_sqrt_w<Mnt4G2S::F>(window, in_wire, n, out_wire, is_square, ms);
  return deg == 1 ? run_sqrt_w<Mnt6G1::F>(window, in_wire, n, out_wire, is_square, ms) : run_sqrt_w<Mnt6G2S::F>(window, in_wire, n, out_wire, is_square, ms);
}

extern "C" int mnt753_test_field_sqrt(int curve, int deg, const uint64_t* in_wire, size_t n, uint64_t* out_wire, uint8_t* is_square) {
  return mnt753_test_field_sqrt_window(curve, deg, SQRT_WINDOW, in_wire, n, out_wire, is_square, nullptr);
}
