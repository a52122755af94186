// mnt753_groth16_verify_folded_locate with the parts of every segment handed out, for the test library (csrc/mnt753_fold_locate.hip,
// include/mnt753_hip_test.h), as fold_api.hpp does for the fold.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/mnt753_hip.h"

namespace mnt753 {
// host memory, any of them may be null; one entry per segment of the call, in order: f the unreduced product of the segment's stepped
// pairs' Miller values (mnt753_gt_words words each), s and t the two G1 points of its tail (affine wire form, 24 words each), rho the
// sum of its coefficients as an element of Fr (wire form, 12 words each), accepted its verdict (1 byte each); status: k_fold_miller's
// byte of every proof (n bytes)
struct FoldLocateParts {
  uint64_t *f = nullptr, *s = nullptr, *t = nullptr, *rho = nullptr;
  uint8_t *accepted = nullptr, *status = nullptr;
};
int groth16_verify_folded_locate_parts(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int on_device, const uint64_t* coefficients,
                                       uint8_t* verdicts, mnt753_fold_locate_report* report, void* stream, const FoldLocateParts* parts);
// chunks the calling thread's last call ran (each a whole number of segments)
size_t groth16_fold_locate_last_chunks();
}  // namespace mnt753
