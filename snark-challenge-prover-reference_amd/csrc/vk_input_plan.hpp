// Plan arithmetic of the input tables of a verification key (mnt753_vk_prepare_inputs) that needs no device:
// the bytes of the tables of a width, the width the library picks under a cap, the row a digit of an input names, and the split of a
// proof's inputs into slices.  Plain integer code on top of batch_exp_plan.hpp, __host__ __device__ where a HIP compiler reads it:
// the walk kernel (vk_input_kernels.hip.h), the host (mnt753_vk_inputs.hip) and the host check (tools/host_vk_inputs_check.cpp,
// compiled by the CPU tests) share exactly these functions.
//
// The tables of the num_inputs + 1 points ABC[p] are ONE long table of section 4.9's layout: window j of base p is window p W + j of
// it, so its row of multiple m is fb_row_of(p W + j, m, w).row = (p W + j) 2^(w-1) + m - 1, and the builder's level kernels
// (k_fb_level, k_fb_normalise<.., true>) enumerate it through FbTargets without knowing that there are several bases.
#pragma once
#include <stdint.h>

#include "batch_exp_plan.hpp"

namespace mnt753 {

constexpr int VKI_MIN_WINDOW_BITS = FB_MIN_WINDOW_BITS;   // 2
constexpr int VKI_MAX_WINDOW_BITS = 16;
constexpr uint32_t VKI_ROW_BYTES = 256;                   // a G1 row of the window tables (row_words<G1>() words)
constexpr uint64_t VKI_DEFAULT_TABLE_BYTES = (uint64_t)256 << 20;   // the Infinity Cache of the MI355X, as for fb_default_window_bits
constexpr uint32_t VKI_PARTIAL_BYTES = 336;               // one projective G1 point in storage form (proj_words<G1>() words)
// lanes a chunk should bring to the walk: one wave per SIMD of a 256-CU part (the walk runs at __launch_bounds__(256, 1))
constexpr uint64_t VKI_TARGET_LANES = 65536;

// rows of the tables of `points` bases at width w; 0 where the count does not fit the 32-bit row index of the kernels
MNT753_PLAN_HD uint64_t vki_table_rows(uint64_t points, int w) {
  const uint64_t rows = points * fb_table_rows(w);
  return rows < ((uint64_t)1 << 32) ? rows : 0;
}
MNT753_PLAN_HD uint64_t vki_table_bytes(uint64_t points, int w) { return points * fb_table_rows(w) * VKI_ROW_BYTES; }
// the widest w in 2 .. 16 whose tables fit `cap` bytes (and the row index); 0: not even w = 2 does
MNT753_PLAN_HD int vki_default_window_bits(uint64_t points, uint64_t cap) {
  int best = 0;
  for (int w = VKI_MIN_WINDOW_BITS; w <= VKI_MAX_WINDOW_BITS; ++w)
    if (vki_table_rows(points, w) && vki_table_bytes(points, w) <= cap) best = w;
  return best;
}
// the row of digit d != 0 of window j of base p, and whether it is taken with y negated
MNT753_PLAN_HD FbRow vki_row_of(uint32_t p, int j, int32_t d, int w) { return fb_row_of((int)(p * (uint32_t)fb_windows(w)) + j, d, w); }
// the rows [first, end) that belong to base p
MNT753_PLAN_HD uint64_t vki_first_row(uint32_t p, int w) { return (uint64_t)p * fb_table_rows(w); }

// ---- the slices of a proof -------------------------------------------------------------------------------------------------------
// A proof's k scalars are walked by S = ceil(k / ipl) lanes: slice s takes the scalars [s ipl, min(k, (s + 1) ipl)), the last one may
// be ragged.  ipl for a chunk of n proofs: as many slices as bring the chunk to VKI_TARGET_LANES lanes, never more than k -- one
// scalar per lane for a single proof, one lane per proof (and a single partial) for a chunk that fills the chip by itself.
MNT753_PLAN_HD uint32_t vki_slices(uint32_t k, uint32_t ipl) { return ipl ? (k + ipl - 1u) / ipl : 0u; }
MNT753_PLAN_HD uint32_t vki_inputs_per_lane(uint64_t n, uint32_t k) {
  if (k == 0) return 1u;
  if (n == 0) n = 1;
  uint64_t want = VKI_TARGET_LANES / n;
  if (want < 1) want = 1;
  const uint32_t s = want < k ? (uint32_t)want : k;
  return (k + s - 1u) / s;
}
struct VkiSlice {
  uint32_t first, end;
};
MNT753_PLAN_HD VkiSlice vki_slice(uint32_t s, uint32_t k, uint32_t ipl) {
  const uint64_t a = (uint64_t)s * ipl, b = a + ipl;
  return VkiSlice{(uint32_t)(a < k ? a : k), (uint32_t)(b < k ? b : k)};
}
// bytes of one proof of a chunk that the prepared path adds to the workspace: S partials, the sum, and the prefix product of the
// normalisation (one field element, 112 bytes)
MNT753_PLAN_HD uint64_t vki_workspace_per_proof(uint32_t k, uint32_t ipl) { return (uint64_t)VKI_PARTIAL_BYTES * (vki_slices(k, ipl) + 1u) + 112u; }

}  // namespace mnt753
