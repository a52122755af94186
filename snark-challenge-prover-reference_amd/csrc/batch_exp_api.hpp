// The object behind mnt753_fixed_base_* / mnt753_batch_exp and the per-group entry points of its host code (each defined in its own
// translation unit, batch_exp_inst_*.hip, so that the four instantiations of the kernels compile in parallel).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// One base point, its table and the workspace of one pass of T scalars.  Everything is allocated by mnt753_fixed_base_create; a
// mnt753_batch_exp call allocates nothing.
struct mnt753_fixed_base {
  int curve = 0, group = 0, device = -1;
  int w = 0, W = 0;            // window bits, windows
  uint32_t B = 0;              // results per inversion
  size_t T = 0;                // scalars per pass
  bool identity = false;       // the base is the identity: no table is built, every output is the identity
  uint32_t* d_table = nullptr;
  size_t table_bytes = 0;
  uint32_t* d_acc = nullptr;     // T projective accumulators
  uint32_t* d_pre = nullptr;     // T prefix products of the normalisation
  uint32_t* d_scaled = nullptr;  // T scalars times the coefficient
  uint32_t* d_in = nullptr;      // staging of T scalars that arrive in host memory
  uint32_t* d_out = nullptr;     // staging of T results that leave to host memory
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // around the walk and the normalisation of the last pass
  bool timed = false;
  float build_ms = 0.f;
};

namespace mnt753 {
#define MNT753_DECL_FB_GROUP(tag)                                                                                            \
  int fixed_base_build_##tag(mnt753_fixed_base* fb, const uint64_t* point, int window_bits, size_t tile);                     \
  int batch_exp_##tag(mnt753_fixed_base* fb, const uint64_t* scalars, int scalars_on_device, size_t n, const uint64_t* host_coeff, \
                      uint64_t* out_affine, int out_on_device, hipStream_t st);
MNT753_DECL_FB_GROUP(mnt4g1)
MNT753_DECL_FB_GROUP(mnt4g2)
MNT753_DECL_FB_GROUP(mnt6g1)
MNT753_DECL_FB_GROUP(mnt6g2)
#undef MNT753_DECL_FB_GROUP
}  // namespace mnt753
