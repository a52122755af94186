// mnt753_groth16_verify_folded with its parts handed out, for the test library (csrc/mnt753_fold.hip, include/mnt753_hip_test.h): a
// wrong Miller product that the final exponentiation or a wrong T happens to hide still shows in the part.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/mnt753_hip.h"

namespace mnt753 {
// host memory, any of them may be null: f the unreduced product of the stepped pairs' Miller values (mnt753_gt_words words), s and t
// the two G1 points of the tail (affine wire form, 24 words each), rho the sum of the coefficients as an element of Fr (wire form)
struct FoldParts {
  uint64_t *f = nullptr, *s = nullptr, *t = nullptr, *rho = nullptr;
};
int groth16_verify_folded_parts(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int on_device, const uint64_t* coefficients,
                                uint8_t* status, int* accepted, void* stream, const FoldParts* parts);
// milliseconds the stages of the calling thread's last folded verification took on the device (HIP events): the scaling with the
// point sum, the Miller loops with the products, the tail (0 where it was skipped)
void groth16_fold_last_timing(float out_ms[3]);
}  // namespace mnt753
