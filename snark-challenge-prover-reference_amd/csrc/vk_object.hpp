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
};
