// mnt753_vec_dot / mnt753_poly_eval with at most max_blocks blocks in the reducing launch (0: the device's own cap), for the test
// library: a small n then reaches the second grid-stride trip of a thread (csrc/mnt753_fft.hip, include/mnt753_hip_test.h)
#pragma once
#include <cstddef>
#include <cstdint>

namespace mnt753 {
int vec_dot_capped(int curve, const uint64_t* dev_a, const uint64_t* dev_b, size_t n, uint64_t* host_out, unsigned max_blocks, void* stream);
int poly_eval_capped(int curve, const uint64_t* dev_coeffs, size_t n, const uint64_t* host_t, uint64_t* host_out, unsigned max_blocks, void* stream);
}  // namespace mnt753
