// C ABI of the compressed points: mnt753_compressed_words, mnt753_compress_points, mnt753_decompress_points, and libff's stream records
// of the packed form, mnt753_points_to_stream / mnt753_points_from_stream (include/mnt753_hip.h).  Kernels: compress_kernels.hip.h;
// the square root: fp_sqrt.hip.h.  mnt753_groth16_verify_compressed is in mnt753_pairing.hip, beside the verifier it feeds.
#include <hip/hip_runtime.h>
#include <cstring>
#include "common_host.hpp"
#include "compress_api.hpp"
#include "compress_kernels.hip.h"
#include "mnt753_generators.h"
#include "point_stream.hpp"

namespace mnt753 {
namespace {
constexpr size_t MAX_LAUNCH = (size_t)1 << 24;   // logical lanes are 32-bit, and the grid is n / 128 (n / 84) workgroups
constexpr size_t MAX_N = (size_t)1 << 38;        // keys are index << 3 | reason

struct Buffers {
  void *in = nullptr, *flags = nullptr, *out = nullptr, *stand = nullptr, *rec = nullptr;
  ~Buffers() {
    for (void* p : {in, flags, out, stand, rec})
      if (p) (void)hipFree(p);
  }
};
int alloc(void** p, size_t bytes) {
  if (hipMalloc(p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return set_error(MNT753_ENOMEM, "compress: device allocation failed");
  }
  return 0;
}
bool ids_ok(int curve, int group) { return (curve == 0 || curve == 1) && (group == MNT753_G1 || group == MNT753_G2); }
const uint64_t* generator(int curve, int group) {
  if (curve == MNT753_CURVE_MNT4753) return group == MNT753_G1 ? GEN_MNT4_G1 : GEN_MNT4_G2;
  return group == MNT753_G1 ? GEN_MNT6_G1 : GEN_MNT6_G2;
}
}  // namespace

size_t decompress_report_bytes() { return sizeof(CompressReport); }
int decompress_report_init(void* rec, hipStream_t st) {
  hipLaunchKernelGGL(k_subgroup_report_init, dim3(1), dim3(1), 0, st, reinterpret_cast<CompressReport*>(rec));
  HIP_TRY(hipGetLastError());
  return 0;
}

int decompress_enqueue(int curve, int group, const uint32_t* x, size_t x_stride, const uint8_t* flags, size_t f_stride, const uint32_t* stand_x,
                       uint32_t* out, size_t out_stride, size_t n, unsigned long long base, void* rec, hipStream_t st) {
  if (!ids_ok(curve, group) || n > MAX_LAUNCH) return set_error(MNT753_EINVAL, "decompress: bad argument");
  if (!n) return 0;
  CompressReport* r = reinterpret_cast<CompressReport*>(rec);
  const dim3 b(256);
  const uint32_t cnt = (uint32_t)n;
  if (group == MNT753_G1) {
    const dim3 g(blocks_for<Mnt4G1::F>(n));
    if (curve == MNT753_CURVE_MNT4753) hipLaunchKernelGGL((k_decompress<Mnt4G1>), g, b, 0, st, x, x_stride, flags, f_stride, stand_x, out, out_stride, cnt, base, r);
    else hipLaunchKernelGGL((k_decompress<Mnt6G1>), g, b, 0, st, x, x_stride, flags, f_stride, stand_x, out, out_stride, cnt, base, r);
  } else if (curve == MNT753_CURVE_MNT4753) {
    hipLaunchKernelGGL((k_decompress<Mnt4G2S>), dim3(blocks_for<Mnt4G2S::F>(n)), b, 0, st, x, x_stride, flags, f_stride, stand_x, out, out_stride, cnt, base, r);
  } else {
    hipLaunchKernelGGL((k_decompress<Mnt6G2S>), dim3(blocks_for<Mnt6G2S::F>(n)), b, 0, st, x, x_stride, flags, f_stride, stand_x, out, out_stride, cnt, base, r);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
}  // namespace mnt753

using namespace mnt753;

extern "C" {

size_t mnt753_compressed_words(int curve, int group) { return ids_ok(curve, group) ? mnt753_affine_words(curve, group) / 2 : 0; }

int mnt753_compress_points(int curve, int group, const uint64_t* affine, int on_device, size_t n, uint64_t* x_out, uint8_t* flags_out, void* stream) {
  if (!ids_ok(curve, group) || (n && (!affine || !x_out || !flags_out)) || n > MAX_N) return set_error(MNT753_EINVAL, "compress_points: bad argument");
  if (int rc = require_device()) return rc;
  if (!n) return 0;
  hipStream_t st = (hipStream_t)stream;
  const size_t wx = mnt753_compressed_words(curve, group);
  Buffers buf;
  const uint64_t* src = affine;
  uint64_t* dx = x_out;
  uint8_t* df = flags_out;
  if (!on_device) {
    if (int rc = alloc(&buf.in, 16 * wx * n)) return rc;
    if (int rc = alloc(&buf.out, 8 * wx * n)) return rc;
    if (int rc = alloc(&buf.flags, n)) return rc;
    HIP_TRY(hipMemcpyAsync(buf.in, affine, 16 * wx * n, hipMemcpyHostToDevice, st));
    src = reinterpret_cast<const uint64_t*>(buf.in);
    dx = reinterpret_cast<uint64_t*>(buf.out);
    df = reinterpret_cast<uint8_t*>(buf.flags);
  }
  for (size_t first = 0; first < n; first += MAX_LAUNCH) {
    const size_t cnt = n - first < MAX_LAUNCH ? n - first : MAX_LAUNCH;
    const uint32_t* a = reinterpret_cast<const uint32_t*>(src + first * 2 * wx);
    uint32_t* xo = reinterpret_cast<uint32_t*>(dx + first * wx);
    uint8_t* fo = df + first;
    const dim3 b(256);
    if (group == MNT753_G1) {
      const dim3 g(blocks_for<Mnt4G1::F>(cnt));
      if (curve == MNT753_CURVE_MNT4753) hipLaunchKernelGGL((k_compress<Mnt4G1>), g, b, 0, st, a, 4 * wx, xo, 2 * wx, fo, (size_t)1, (uint32_t)cnt);
      else hipLaunchKernelGGL((k_compress<Mnt6G1>), g, b, 0, st, a, 4 * wx, xo, 2 * wx, fo, (size_t)1, (uint32_t)cnt);
    } else if (curve == MNT753_CURVE_MNT4753) {
      hipLaunchKernelGGL((k_compress<Mnt4G2S>), dim3(blocks_for<Mnt4G2S::F>(cnt)), b, 0, st, a, 4 * wx, xo, 2 * wx, fo, (size_t)1, (uint32_t)cnt);
    } else {
      hipLaunchKernelGGL((k_compress<Mnt6G2S>), dim3(blocks_for<Mnt6G2S::F>(cnt)), b, 0, st, a, 4 * wx, xo, 2 * wx, fo, (size_t)1, (uint32_t)cnt);
    }
  }
  HIP_TRY(hipGetLastError());
  if (!on_device) {
    HIP_TRY(hipMemcpyAsync(x_out, dx, 8 * wx * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(flags_out, df, n, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));               // the call's buffers go when it returns
  return 0;
}

int mnt753_decompress_points(int curve, int group, const uint64_t* x, const uint8_t* flags, int on_device, size_t n, uint64_t* affine_out,
                             mnt753_check_report* out, void* stream) {
  if (!ids_ok(curve, group) || !out || (n && (!x || !flags || !affine_out)) || n > MAX_N) return set_error(MNT753_EINVAL, "decompress_points: bad argument");
  if (int rc = require_device()) return rc;
  *out = mnt753_check_report{0, 0, MNT753_BAD_NONE, 0};
  if (!n) return 0;
  hipStream_t st = (hipStream_t)stream;
  const size_t wx = mnt753_compressed_words(curve, group);
  Buffers buf;
  const uint64_t* dx = x;
  const uint8_t* df = flags;
  uint64_t* dout = affine_out;
  if (!on_device) {
    if (int rc = alloc(&buf.in, 8 * wx * n)) return rc;
    if (int rc = alloc(&buf.flags, n)) return rc;
    if (int rc = alloc(&buf.out, 16 * wx * n)) return rc;
    HIP_TRY(hipMemcpyAsync(buf.in, x, 8 * wx * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(buf.flags, flags, n, hipMemcpyHostToDevice, st));
    dx = reinterpret_cast<const uint64_t*>(buf.in);
    df = reinterpret_cast<const uint8_t*>(buf.flags);
    dout = reinterpret_cast<uint64_t*>(buf.out);
  }
  if (int rc = alloc(&buf.stand, 8 * wx)) return rc;
  if (int rc = alloc(&buf.rec, sizeof(CompressReport))) return rc;
  HIP_TRY(hipMemcpyAsync(buf.stand, generator(curve, group), 8 * wx, hipMemcpyHostToDevice, st));
  if (int rc = decompress_report_init(buf.rec, st)) return rc;
  for (size_t first = 0; first < n; first += MAX_LAUNCH) {
    const size_t cnt = n - first < MAX_LAUNCH ? n - first : MAX_LAUNCH;
    if (int rc = decompress_enqueue(curve, group, reinterpret_cast<const uint32_t*>(dx + first * wx), 2 * wx, df + first, 1,
                                    reinterpret_cast<const uint32_t*>(buf.stand), reinterpret_cast<uint32_t*>(dout + first * 2 * wx), 4 * wx, cnt,
                                    (unsigned long long)first, buf.rec, st))
      return rc;
  }
  CompressReport host;
  HIP_TRY(hipMemcpyAsync(&host, buf.rec, sizeof(host), hipMemcpyDeviceToHost, st));
  if (!on_device) HIP_TRY(hipMemcpyAsync(affine_out, dout, 16 * wx * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  out->n_bad = host.n_bad;
  out->first_bad = host.n_bad ? (uint64_t)(host.key >> 3) : 0;
  out->first_reason = host.n_bad ? (uint32_t)(host.key & 7u) : (uint32_t)MNT753_BAD_NONE;
  return 0;
}

// ---- libff's stream records (host only; the codec: point_stream.hpp) ----------------------------------------------------------------
int mnt753_points_to_stream(int curve, int group, const uint64_t* x, const uint8_t* flags, size_t n, uint8_t* buf, size_t cap, size_t* len) {
  if (!ids_ok(curve, group) || !len || (n && (!x || !flags))) return set_error(MNT753_EINVAL, "points_to_stream: bad argument");
  const size_t xb = 8 * mnt753_compressed_words(curve, group);
  *len = n * (xb + 2);
  if (!buf) return 0;                              // the size only
  if (cap < *len) return set_error(MNT753_EINVAL, "points_to_stream: buffer too small");
  if (stream_write(xb, x, flags, n, buf) != STREAM_OK) return set_error(MNT753_EINVAL, "points_to_stream: a flag byte has a bit above the identity flag set");
  return 0;
}

int mnt753_points_from_stream(int curve, int group, const uint8_t* buf, size_t len, size_t n, uint64_t* x, uint8_t* flags) {
  if (!ids_ok(curve, group) || (n && (!buf || !x || !flags))) return set_error(MNT753_EINVAL, "points_from_stream: bad argument");
  switch (stream_read(8 * mnt753_compressed_words(curve, group), buf, len, n, x, flags)) {
    case STREAM_OK: return 0;
    case STREAM_SHORT: return set_error(MNT753_EINVAL, "points_from_stream: the buffer is shorter than n records");
    default: return set_error(MNT753_EINVAL, "points_from_stream: a flag byte is neither '0' nor '1'");
  }
}

}  // extern "C"
