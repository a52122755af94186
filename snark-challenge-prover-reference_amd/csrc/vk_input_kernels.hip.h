// The public inputs of a Groth16 verifier on window tables: many scalars, each against the table of its own
// fixed base, summed per proof.
//
// Replaces, for a key that was prepared (mnt753_vk_prepare_inputs), the accumulation of r1cs_gg_ppzksnark_online_verifier_weak_IC
// (libsnark/zk_proof_systems/ppzksnark/r1cs_gg_ppzksnark/r1cs_gg_ppzksnark.tcc:522-525: ABC.accumulate_chunk over the primary input)
// by libff's fixed-base method (get_window_table / windowed_exp / batch_exp, depends/libff/libff/algebra/scalar_multiplication/
// multiexp.tcc:547-720) with one table per ABC point.  Same group elements; the schedule is the device's:
//
//   k_vk_window_bases   one lane per ABC point p: the doubling chain 2^(jw) ABC[p] in modified Jacobian coordinates (jac_dbl), every
//                       w-th point dropped onto row (p W + j, 1) of the long table (vk_input_plan.hpp), then ONE inversion per lane
//                       over its W - 1 points (Montgomery's trick, as k_precompute_windows does for its layout).  The multiples come
//                       from batch_exp's k_fb_level / k_fb_normalise<.., true> over all windows of all points at once.
//   k_vk_walk           one lane per (proof, slice of inputs_per_lane consecutive scalars): per scalar the integer k_inputs_to_integer
//                       wrote, parked in the thread's LDS column, its W signed digits from low to high against the table of that
//                       scalar's base, one straight-line mixed addition per non-zero digit (k_fb_walk's step).  One accumulator per
//                       slice, one projective partial per lane.
//   k_vk_segment_sum    one lane per proof: ABC[0] plus the proof's partials through the point VM (they may be equal, opposite or the
//                       identity: g1_sum_step).  k_fb_normalise<.., false> then writes the affine wire form, the identity as zero words.
//   k_vk_input_dots     the fold's c_j = sum_i rho_i x_ij for ALL inputs j of a chunk in one launch: one block per column, the
//                       arithmetic of k_vec_dot (reduce_kernels.hip.h), the sum carried from chunk to chunk in device form.
//   k_vk_fold_scalars   the carried sums -> integers, the scalars of the one walk that forms the fold's S.
// G1 only: two instantiations of each point kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "batch_exp_kernels.hip.h"
#include "fold_kernels.hip.h"
#include "reduce_kernels.hip.h"
#include "vk_input_plan.hpp"

namespace mnt753 {

// ---- the window bases --------------------------------------------------------------------------------------------------------------
// Lane p < points: row (p W + j, 1) = 2^(jw) ABC[p], affine, for j < W.  abc: the key's points in the affine wire form (none of them
// is the identity: mnt753_vk_create refuses such a key).  Between the two passes a window keeps X, Y in its row of multiple 1 and Z
// and the prefix product in its row of multiple 2 (every width has one: w >= 2), in the x and y words of that row -- the level
// kernels overwrite exactly those words afterwards, and the padding words of a row are never touched.
template <class C1>
__global__ void __launch_bounds__(256, 1) k_vk_window_bases(const uint32_t* __restrict__ abc, uint32_t* __restrict__ table, uint32_t points, int w, int W) {
  using F = typename C1::F;
  using E = typename F::E;
  constexpr size_t RW = row_words<C1>();
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= points) return;
  const size_t H = fb_rows_per_window(w);
  uint32_t* first = table + (size_t)p * (size_t)W * H * RW;     // row (p W, 1)
  Jac<F> R;
  {
    uint32_t wr[24];
    load_wire24(wr, abc + (size_t)p * 48); fp_from_wire(R.X, wr);
    load_wire24(wr, abc + (size_t)p * 48 + 24); fp_from_wire(R.Y, wr);
  }
  F::one(R.Z);
  C1::coeff_a(R.W);
  e_store<F>(first, R.X);
  e_store<F>(first + row_y_off<C1>(), R.Y);
  // pass 1: R_j = 2^w R_(j-1); X, Y into row (p W + j, 1), Z into the x words of row (p W + j, 2)
#pragma unroll 1
  for (int j = 1; j < W; ++j) {
#pragma unroll 1
    for (int k = 0; k < w; ++k) jac_dbl<C1>(R);
    uint32_t* row = first + (size_t)j * H * RW;
    e_store<F>(row, R.X);
    e_store<F>(row + row_y_off<C1>(), R.Y);
    e_store<F>(row + RW, R.Z);
  }
  // pass 2: the prefix products of Z_1 .. Z_(W-1) into the y words of row (p W + j, 2), one inversion, and on the way back
  // x = X / Z^2, y = Y / Z^3
  E pre, z, inv, zi, x, y, tmp;
  F::one(pre);
#pragma unroll 1
  for (int j = 1; j < W; ++j) {
    uint32_t* row = first + (size_t)j * H * RW;
    e_store<F>(row + RW + row_y_off<C1>(), pre);
    e_load<F>(z, row + RW);
    F::mul(tmp, pre, z);
    pre = tmp;
  }
  F::inv(inv, pre);
#pragma unroll 1
  for (int j = W - 1; j >= 1; --j) {
    uint32_t* row = first + (size_t)j * H * RW;
    e_load<F>(tmp, row + RW + row_y_off<C1>());
    e_load<F>(z, row + RW);
    e_load<F>(x, row);
    e_load<F>(y, row + row_y_off<C1>());
    // six products through one multiplier instance (k_precompute_windows): 1 / Z_j, the running inverse, 1 / Z^2, x, 1 / Z^3, y
    E zi2;
#pragma nounroll
    for (int step = 0; step < 6; ++step) {
      E a, b, r;
      switch (step) {
        case 0: a = inv; b = tmp; break;
        case 1: a = inv; b = z; break;
        case 2: a = zi; b = zi; break;
        case 3: a = x; b = zi2; break;
        case 4: a = zi2; b = zi; break;
        default: a = y; b = zi; break;
      }
      F::mul(r, a, b);
      switch (step) {
        case 0: zi = r; break;
        case 1: inv = r; break;
        case 2: zi2 = r; break;
        case 3: e_store<F>(row, r); break;
        case 4: zi = r; break;
        default: e_store<F>(row + row_y_off<C1>(), r); break;
      }
    }
  }
}

// ---- the multi-base walk ---------------------------------------------------------------------------------------------------------
// Lane t < n slices: proof i = t / slices, slice s = t % slices, scalars [s ipl, min(k, (s + 1) ipl)) of the proof's k
// (vki_slice).  ints: n x k integers of 24 words (k_inputs_to_integer); scalar jj of a proof walks the table of base base0 + jj.
// out[t]: the slice's sum, projective in storage form (Z = 0: the identity).  A scalar is walked on whatever its 768 bits say (an input
// >= r: the proof's bad flag decides its verdict); |digit| <= 2^(w-1) for any words, so every row read lies inside that base's tables.
template <class C1>
__global__ void __launch_bounds__(256, 1) k_vk_walk(const uint32_t* __restrict__ table, const uint32_t* __restrict__ ints, uint32_t* __restrict__ out,
                                                   uint32_t n, uint32_t k, uint32_t ipl, uint32_t slices, uint32_t base0, int w, int W) {
  using F = typename C1::F;
  // the integer of the scalar in hand, word q at sw[q * 256 + tid]: indexed by the digit's position; behind it the lane's place in
  // its slice -- the scalar it is at and the one it ends before -- which lives here, not in registers, while the W additions of a
  // scalar run: the addition takes every register the kernel has (volatile: the compiler must not keep a copy)
  __shared__ uint32_t sw[26 * 256];
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;     // (the host keeps n slices below 2^31)
  if ((uint64_t)t >= (uint64_t)n * slices) return;
  const int tid = threadIdx.x;
  volatile uint32_t* at = sw + 24 * 256 + tid;                  // at[0]: the next scalar, at[256]: the end of the slice
  {
    const VkiSlice sl = vki_slice(t % slices, k, ipl);
    at[0] = sl.first;
    at[256] = sl.end;
  }
  bool acc_zero = true;
  Proj<C1> acc, Q;
  pt_set_zero(acc);
  F::zero(Q.X); F::zero(Q.Y); F::one(Q.Z);
#pragma unroll 1
  for (;;) {
    const uint32_t jj = at[0];
    if (jj >= at[256]) break;
    at[0] = jj + 1u;
    {
      uint32_t s[24];
      load_wire24(s, ints + ((size_t)((blockIdx.x * blockDim.x + threadIdx.x) / slices) * k + jj) * 24);
#pragma unroll
      for (int q = 0; q < 24; ++q) sw[q * 256 + tid] = s[q];
    }
    // every thread reads back its own column only: no barrier
    const uint32_t window0 = (base0 + jj) * (uint32_t)W;        // the first window of this scalar's base in the long table
#pragma unroll 1
    for (int j = 0; j < W; ++j) {
      const int32_t d = fb_digit(sw + tid, 256, j, w);
      int pc = PC_END;
      if (d != 0) {
        const FbRow r = fb_row_of((int)window0 + j, d, w);       // vki_row_of(base0 + jj, j, d, w)
        const uint32_t* src = table + (size_t)r.row * row_words<C1>();
        e_load<F>(Q.X, src);
        e_load<F>(Q.Y, src + row_y_off<C1>());
        if (r.negate) F::neg(Q.Y, Q.Y);
        if (acc_zero || pt_is_zero(acc)) {           // nothing yet, or a sum that cancelled: take the row over
          acc.X = Q.X; acc.Y = Q.Y; F::one(acc.Z);
          acc_zero = false;
        } else {
          pc = PC_MADD;
        }
      }
      // the straight-line mixed addition of k_fb_walk: lanes without an addition run the same instructions and keep their value,
      // equal points fall back to the VM's doubling, opposite points give Z = 0
      MNT753_MADD_LINE(C1, F, acc, Q, pc);
    }
  }
  if (acc_zero) pt_set_zero(acc);
  proj_store<C1>(out + (size_t)(blockIdx.x * blockDim.x + threadIdx.x) * proj_words<C1>(), acc);
}

// ---- the sum of a proof ----------------------------------------------------------------------------------------------------------
// sums[i] = (first ? the point first[0..48) in affine wire form : the identity) + partials[i slices] + .. + partials[i slices + slices - 1]
template <class C1>
__global__ void __launch_bounds__(256, 1) k_vk_segment_sum(const uint32_t* __restrict__ first, const uint32_t* __restrict__ partials, uint32_t* __restrict__ sums,
                                                          uint32_t n, uint32_t slices) {
  using F = typename C1::F;
  constexpr int PW = proj_words<C1>();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Proj<C1> acc, Q;
  if (first) {
    uint32_t wr[24];
    load_wire24(wr, first); fp_from_wire(acc.X, wr);
    load_wire24(wr, first + 24); fp_from_wire(acc.Y, wr);
    F::one(acc.Z);
  } else {
    pt_set_zero(acc);
  }
#pragma unroll 1
  for (uint32_t s = 0; s < slices; ++s) {
    proj_load<C1>(Q, partials + ((size_t)i * slices + s) * PW);
    g1_sum_step<C1>(acc, Q);
  }
  if (pt_is_zero(acc)) pt_set_zero(acc);
  proj_store<C1>(sums + (size_t)i * PW, acc);
}

// ---- the fold's scalars ------------------------------------------------------------------------------------------------------------
// Block j < k: acc[j] (+)= sum_{i < n} rho[i] x[i k + j] in Fr: both operands as they lie in wire form, the sum in device form behind
// fp_norm (FPS_WORDS words: k_vec_dot's partial), `carry`: acc[j] holds the sum of the chunks before.  One launch for all columns.
template <int M>
__global__ void __launch_bounds__(RED_BLOCK) k_vk_input_dots(const uint32_t* __restrict__ rho, const uint32_t* __restrict__ x, uint32_t n, uint32_t k,
                                                            uint32_t* __restrict__ acc_out, int carry) {
  __shared__ __align__(16) uint32_t lds[(RED_BLOCK / 64) * FPS_WORDS];
  const uint32_t j = blockIdx.x;
  Fp<M> acc;
  fp_zero(acc);
  uint32_t pending = 0;
#pragma unroll 1
  for (uint32_t i = threadIdx.x; i < n; i += RED_BLOCK) {
    uint32_t wr[24];
    Fp<M> y;
    load_wire24(wr, rho + (size_t)i * 24);
    fp_unpack(y, wr);
    dot_term<M>(acc, pending, x + ((size_t)i * k + j) * 24, y);
  }
  red_flush(acc, pending);
  red_block_sum(acc, lds);
  if (threadIdx.x == 0) {
    if (carry) {
      Fp<M> o;
      fp_load(o, acc_out + (size_t)j * FPS_WORDS);
      red_combine(acc, o);
    }
    fp_store(acc_out + (size_t)j * FPS_WORDS, acc);
  }
}
// ints[j] = the integer of c_j for j < k: the carried sum of products of wire operands -> canonical wire form (red_finish) -> integer
template <int M>
__global__ void __launch_bounds__(256) k_vk_fold_scalars(const uint32_t* __restrict__ acc, uint32_t k, uint32_t* __restrict__ ints) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  Fp<M> a;
  fp_load(a, acc + (size_t)j * FPS_WORDS);
  uint32_t wr[24], s[24];
  red_finish(wr, a);
  fp_wire_to_integer<M>(s, wr);
  store_wire24(ints + (size_t)j * 24, s);
}

}  // namespace mnt753
