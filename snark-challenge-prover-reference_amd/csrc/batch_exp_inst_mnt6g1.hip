// Fixed-base batch scalar multiplication: kernels + host orchestration instantiated for Mnt6G1.
#include "batch_exp_host.hpp"
namespace mnt753 {
int fixed_base_build_mnt6g1(mnt753_fixed_base* fb, const uint64_t* point, int window_bits, size_t tile) {
  return fixed_base_build_t<Mnt6G1>(fb, point, window_bits, tile);
}
int batch_exp_mnt6g1(mnt753_fixed_base* fb, const uint64_t* scalars, int scalars_on_device, size_t n, const uint64_t* host_coeff, uint64_t* out_affine,
                     int out_on_device, hipStream_t st) {
  return batch_exp_t<Mnt6G1>(fb, scalars, scalars_on_device, n, host_coeff, out_affine, out_on_device, st);
}
}  // namespace mnt753
