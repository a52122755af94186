// The prepared path of a verification key's public inputs (csrc/mnt753_vk_inputs.hip) for the translation
// units that verify against the key: mnt753_pairing.hip (the per-proof verifiers, mnt753_vk_accumulate) and mnt753_fold.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "vk_input_plan.hpp"
#include "vk_object.hpp"

namespace mnt753 {
inline bool vk_inputs_prepared(const mnt753_vk* vk) { return vk->dev_in_table != nullptr; }
// scalars per lane of the walk for a chunk of n proofs of `scalars` scalars each: the host's choice (vki_inputs_per_lane) unless the
// test library forced one, raised where the launch would pass 2^31 lanes
uint32_t vk_inputs_per_lane(const mnt753_vk* vk, size_t n, uint32_t scalars);
// device memory of one chunk; all of it is the call's, allocated once per call
struct VkInputWs {
  uint32_t* partials = nullptr;   // n slices projective points, VKI_PARTIAL_BYTES each
  uint32_t* sums = nullptr;       // n projective points
  uint32_t* pre = nullptr;        // n field elements (112 bytes): the prefix products of the normalisation
};
inline size_t vk_inputs_partials_bytes(size_t n, uint32_t scalars, uint32_t ipl) { return (size_t)VKI_PARTIAL_BYTES * n * vki_slices(scalars, ipl); }
inline size_t vk_inputs_sums_bytes(size_t n) { return (size_t)VKI_PARTIAL_BYTES * n; }
inline size_t vk_inputs_pre_bytes(size_t n) { return (size_t)112 * n; }
// out_wire[i] = (first_wire ? that point : the identity) + sum_{jj < scalars} ints[i][jj] ABC[base0 + jj] for i < n, affine wire form
// (the identity: zero words).  ints: n x scalars integers of 24 words, device.  Enqueues only.
int vk_inputs_enqueue(const mnt753_vk* vk, const uint32_t* ints, size_t n, uint32_t scalars, uint32_t base0, const uint32_t* first_wire, uint32_t ipl,
                      const VkInputWs& ws, uint32_t* out_wire, hipStream_t st);
// acc[j] (+)= sum_i rho[i] x[i k + j] for j < k (rho, x: Fr in wire form, device; acc: k x 28 words, device form; carry: add to what is there)
int vk_inputs_dots_enqueue(int curve, const uint32_t* rho, const uint32_t* x, size_t n, uint32_t k, uint32_t* acc, int carry, hipStream_t st);
// ints[j] = acc[j] as an integer for j < k
int vk_inputs_fold_scalars_enqueue(int curve, const uint32_t* acc, uint32_t k, uint32_t* ints, hipStream_t st);
// milliseconds of the walk and of the segment sum with the normalisation of the key's last chunk (HIP events; synchronises on them);
// build: of the last mnt753_vk_prepare_inputs
int vk_inputs_last_timing(const mnt753_vk* vk, float* walk_ms, float* sum_ms, float* build_ms);
}  // namespace mnt753
