// The verification-key object of the C ABI (include/mnt753_hip.h: mnt753_vk), shared by the translation units that verify against it
// (mnt753_pairing.hip creates and destroys it; mnt753_fold.hip reads it).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// a verification key: libsnark's r1cs_gg_ppzksnark_processed_verification_key, the coefficients of its two G2 points on the device
struct mnt753_vk {
  int curve = 0, device = 0;
  size_t num_inputs = 0;
  std::vector<uint64_t> delta, abc, gt;
  uint64_t* dev_key = nullptr;   // stand-in G1 (the generator) | G2::one() | delta_g2 | e(alpha, beta)
  uint64_t* dev_abc = nullptr;   // num_inputs + 1 G1 points
  uint32_t* dev_coeffs = nullptr;   // the Miller-loop coefficients of G2::one(), then of delta_g2 (k_g2_precompute)
  size_t workspace_cap = 0;      // bytes a verify call may allocate; 0: the default chunk of 2^16 proofs
  // the input tables (mnt753_vk_prepare_inputs, mnt753_vk_inputs.hip): one signed-digit window table per ABC
  // point in one allocation, window j of point p being window p in_W + j of one long table of batch_exp's layout.  nullptr: the key
  // was not prepared and every call launches k_vk_accumulate.
  uint32_t* dev_in_table = nullptr;
  int in_w = 0, in_W = 0;
  size_t in_table_bytes = 0;
  float in_build_ms = 0.f;
  void* in_ev[3] = {nullptr, nullptr, nullptr};   // hipEvent_t: around the walk and the segment sum of the last chunk (the test library reads them)
  mutable bool in_timed = false;
  uint32_t test_inputs_per_lane = 0;   // the test library's hook: scalars per lane of the walk instead of the host's choice
};
