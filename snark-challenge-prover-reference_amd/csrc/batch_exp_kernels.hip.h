// Fixed-base batch scalar multiplication for gfx950: n scalars times ONE base point.
//
// Replaces libff's get_window_table / windowed_exp / batch_exp / batch_exp_with_coeff followed by batch_to_special
// (depends/libff/libff/algebra/scalar_multiplication/multiexp.tcc:547-583, :585-612, :614-668, :670-720): what the Groth16 generator
// applies to its A, B, L, H and IC queries (libsnark/zk_proof_systems/ppzksnark/r1cs_gg_ppzksnark/r1cs_gg_ppzksnark.tcc:293-352).  Same
// group elements, in the affine wire format; the schedule is the device's:
//
//   table       rows m 2^(jw) P, m = 1 .. 2^(w-1), for every window j (batch_exp_plan.hpp: signed digits halve libff's 2^w rows per
//               window), affine, in the row format of the MSM's tables (row_words / row_y_off, msm_kernels.hip.h).  Window bases
//               2^(jw) P: the doubling chain of the MSM's table (k_precompute_windows: jac_dbl, one simultaneous inversion).  Multiples:
//               level by level, row[2m] = 2 row[m], row[2m+1] = row[2m] + row[1] -- k_fb_level, one lane per new row and one group
//               operation or two deep, then k_fb_normalise to affine: w - 1 levels, not 2^(w-1) additions in a chain.
//   k_fb_walk   one logical lane (1, 2 or 3 threads, logical_lane<F>()) per scalar: Montgomery form -> integer (as_bigint,
//               fp.tcc:227-238), signed digits, and per non-zero digit one gathered row (y negated for a negative digit) added with
//               the complete mixed addition of k_bucket_accumulate: an identity accumulator takes the row over, equal points double,
//               opposite points give Z = 0.
//   k_fb_normalise   projective -> affine with Montgomery's simultaneous inversion over runs of B consecutive results (batch_to_special,
//               multiexp.tcc:670-720, which also filters the identities out of its product); writes wire-format points (identity: all
//               words zero) or table rows.
#pragma once
#include <hip/hip_runtime.h>
#include "batch_exp_plan.hpp"
#include "msm_kernels.hip.h"

namespace mnt753 {

// where element t of a normalise launch goes: wire point first + t, or the table row of multiple m0 + g % cnt of window g / cnt,
// g = first + t (the enumeration of one level of the table: k_fb_level)
struct FbTargets {
  uint64_t first;
  uint32_t cnt, m0;
  int w;
};
__device__ __forceinline__ uint32_t fb_target_row(const FbTargets& tg, uint32_t t, uint32_t* multiple) {
  const uint64_t g = tg.first + t;
  const uint32_t j = (uint32_t)(g / tg.cnt), m = tg.m0 + (uint32_t)(g % tg.cnt);
  *multiple = m;
  return fb_row_of((int)j, (int32_t)m, tg.w).row;
}

// ---- one level of the table ----------------------------------------------------------------------------------------------------
// Lane t builds multiple m (m0 <= m < m0 + cnt, m0 = 2^level) of one window as 2 row[m >> 1] (+ row[1] for odd m) into out[t]
// (projective).  Rows are complete: a row whose y is zero is the identity (a base of small order can reach it; no affine point of
// these curves' prime-order subgroups has y = 0), and the doubling and the addition run through the point VM, which handles equal
// and opposite operands.  One instance of the VM: the two operations are two trips of one loop.
template <class C>
__global__ void __launch_bounds__(256, 1) k_fb_level(const uint32_t* __restrict__ table, uint32_t* __restrict__ out, FbTargets tg, uint32_t count) {
  using F = typename C::F;
  const uint32_t t = logical_lane<F>();
  if (t == 0xffffffffu || t >= count) return;
  uint32_t m;
  const uint32_t dst = fb_target_row(tg, t, &m);
  const uint32_t first_of_window = dst - (m - 1u);
  Proj<C> P, Q;
  pt_set_zero(P);
  F::one(Q.Z);
#pragma unroll 1
  for (int phase = 0; phase < 2; ++phase) {
    if (phase == 1 && !(m & 1u)) break;
    const uint32_t* src = table + (size_t)(phase == 0 ? first_of_window + (m >> 1) - 1u : first_of_window) * row_words<C>();
    e_load<F>(Q.X, src);
    e_load<F>(Q.Y, src + row_y_off<C>());
    int pc = phase == 0 ? PC_DBL : PC_MADD;
    if (F::is_zero(Q.Y)) pc = PC_END;                                     // adding or doubling the identity
    else if (phase == 0 || pt_is_zero(P)) {                               // take the row over: doubled in phase 0, as it is in phase 1
      P.X = Q.X; P.Y = Q.Y; F::one(P.Z);
      if (phase == 1) pc = PC_END;
    }
    pt_vm<C, false>(P, Q, pc);
  }
  proj_store<C>(out + (size_t)t * proj_words<C>(), P);
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------------
// out[t] = scalars[t] * P (projective, device form) for t < count, through the table of width w with W windows.
template <class C>
__global__ void __launch_bounds__(256, 1) k_fb_walk(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scal_wire,
                                                   uint32_t* __restrict__ out, uint32_t count, int w, int W) {
  using F = typename C::F;
  __shared__ uint32_t sw[24 * 256];   // the integer of this thread's scalar, word k at sw[k * 256 + tid]: indexed by the digit's position
  const uint32_t t = logical_lane<F>();
  if (t == 0xffffffffu || t >= count) return;   // (all threads of a logical lane leave together)
  const int tid = threadIdx.x;
  {
    uint32_t wr[24], s[24];
    load_wire24(wr, scal_wire + (size_t)t * 24);
    fp_wire_to_integer<C::FR>(s, wr);
#pragma unroll
    for (int k = 0; k < 24; ++k) sw[k * 256 + tid] = s[k];
  }
  // every thread reads back its own column only: no barrier
  bool acc_zero = true;
  Proj<C> acc, Q;
  pt_set_zero(acc);
  F::zero(Q.X); F::zero(Q.Y); F::one(Q.Z);
#pragma unroll 1
  for (int j = 0; j < W; ++j) {
    const int32_t d = fb_digit(sw + tid, 256, j, w);
    int pc = PC_END;
    if (d != 0) {
      const FbRow r = fb_row_of(j, d, w);
      const uint32_t* src = table + (size_t)r.row * row_words<C>();
      e_load<F>(Q.X, src);
      e_load<F>(Q.Y, src + row_y_off<C>());
      if (r.negate) F::neg(Q.Y, Q.Y);
      if (!F::is_zero(Q.Y)) {                      // (an identity row: a base of small order)
        if (acc_zero || pt_is_zero(acc)) {         // nothing yet, or a sum that cancelled: take the row over
          acc.X = Q.X; acc.Y = Q.Y; F::one(acc.Z);
          acc_zero = false;
        } else {
          pc = PC_MADD;
        }
      }
    }
    if constexpr ((F::LANES == 1 && F::DEG == 1) || F::LANES == 2) {
      // base fields and the two-lane Fq2: the straight-line mixed addition of k_bucket_accumulate; lanes without an addition run the
      // same instructions and keep their value, equal points fall back to the VM's doubling
      MNT753_MADD_LINE(C, F, acc, Q, pc);
    } else {
      pt_vm<C, false>(acc, Q, pc);
    }
  }
  if (acc_zero) pt_set_zero(acc);
  proj_store<C>(out + (size_t)t * proj_words<C>(), acc);
}

// ---- projective -> affine, B results per inversion ----------------------------------------------------------------------------------
// Logical lane q owns results [q B, min((q + 1) B, count)) of `in`: prefix products of their Z (identities left out, as
// batch_to_special leaves them out) into `pre`, one inversion, and on the way back x = X / Z, y = Y / Z.
// ROWS: the results are one level of the table and go to their rows (device form; an identity is a row of zeros); otherwise they
// are written as wire-format affine points tg.first + t of out (identity: all words zero).
template <class C, bool ROWS>
__global__ void __launch_bounds__(256, 1) k_fb_normalise(const uint32_t* __restrict__ in, uint32_t* __restrict__ pre, uint32_t* __restrict__ out,
                                                        FbTargets tg, uint32_t count, uint32_t B) {
  using F = typename C::F;
  using E = typename F::E;
  constexpr int EW = F::DEG * FPS_WORDS;
  const uint32_t q = logical_lane<F>();
  if (q == 0xffffffffu || (uint64_t)q * B >= count) return;
  const uint32_t t0 = q * B, len = min(B, count - t0);
  E run, z, tmp, inv;
  F::one(run);
#pragma unroll 1
  for (uint32_t k = 0; k < len; ++k) {
    e_store<F>(pre + (size_t)(t0 + k) * EW, run);
    e_load<F>(z, in + (size_t)(t0 + k) * proj_words<C>() + 2 * EW);
    if (F::is_zero(z)) F::one(z);
    F::mul(tmp, run, z);
    run = tmp;
  }
  static_assert(has_inv<F>::value, "the point kernels run on base fields and lane-split extension fields");
  F::inv(inv, run);
#pragma unroll 1
  for (uint32_t k = len; k-- > 0;) {
    const uint32_t t = t0 + k;
    const uint32_t* src = in + (size_t)t * proj_words<C>();
    E x, y, zi;
    e_load<F>(x, src);
    e_load<F>(y, src + EW);
    e_load<F>(z, src + 2 * EW);
    e_load<F>(tmp, pre + (size_t)t * EW);
    const bool ident = F::is_zero(z);
    if (ident) F::one(z);
    // four products through one instance of the multiplier: 1 / Z, the inverse of the shorter prefix, x, y
#pragma nounroll
    for (int step = 0; step < 4; ++step) {
      E a, b, r;
      switch (step) {
        case 0: a = inv; b = tmp; break;
        case 1: a = inv; b = z; break;
        case 2: a = x; b = zi; break;
        default: a = y; b = zi; break;
      }
      F::mul(r, a, b);
      switch (step) {
        case 0: zi = r; break;
        case 1: inv = r; break;
        case 2: x = r; break;
        default: y = r; break;
      }
    }
    if constexpr (ROWS) {
      uint32_t m;
      uint32_t* row = out + (size_t)fb_target_row(tg, t, &m) * row_words<C>();
      if (ident) { F::zero(x); F::zero(y); }
      e_store<F>(row, x);
      e_store<F>(row + row_y_off<C>(), y);
    } else {
      uint32_t* dst = out + (tg.first + t) * 2 * wire_coord_words<C>() + 24 * lane_comp<F>();
#pragma unroll 1
      for (int c = 0; c < 2; ++c) {
        uint32_t wr[24];
        fp_to_wire(wr, c == 0 ? x : y);
        if (ident) {
#pragma unroll
          for (int i = 0; i < 24; ++i) wr[i] = 0u;
        }
        store_wire24(dst + c * wire_coord_words<C>(), wr);
      }
    }
  }
}

}  // namespace mnt753
