// Reductions over Fr for gfx950: inner products against one shared vector and the value of a polynomial at a point
// (DESIGN.md section 4.14).  They carry the spot check of compute_H, H(t) Z(t) = A(t) B(t) - C(t) at a random t.
//
//   k_vec_dot<M, K>   K sums  sum_i a_k[i] u[i]  against one u, which is read once for all K vectors.  A thread walks a grid-stride
//                     sequence of elements: both operands as they lie in wire form (x R as an integer below r), one product each,
//                     limb-wise sums without carries, one fp_norm per two terms (the arithmetic of k_r1cs_evaluate / k_qap_chunks).
//                     The product of two wire operands is a u R^2 / R'; the one product by k_in that returns it to a R-form is paid
//                     once per RESULT (red_finish), not once per element as in k_vec_muleq.
//   k_poly_eval<M>    sum_i c_i t^i without the powers in memory: a thread takes a run of POLY_RUN consecutive coefficients, does
//                     Horner inside the run (one product per coefficient: the accumulator stays in R-form, the coefficient is added
//                     as it lies in wire form) and scales the run by t^(run start), which it raises by squaring as k_vec_powers does.
//   k_red_fold<M>     one block: the per-block partial sums of either kernel, K results in canonical wire form.
//
// The threads of a block combine by cross-lane shifts inside a wave and through 4 x 28 words of LDS across the waves; a block writes
// one partial per k.  No atomics, no last-block flag.  Field addition is exact, so the result does not depend on the geometry.
//
// Ranges (r / R' < 0.1106 for both moduli; fp753.hip.h states fp_mul's and fp_norm's contracts):
//   dot     operands canonical (below r, limbs below 2^28): a product lies in [0, 1.12 r) with limbs below 2^28.  The accumulator is in
//           [0.49 r, 1.51 r) behind fp_norm (or 0 before the first term); with two products on top its value is below 3.75 r and a limb
//           below 3 * 2^28: fp_norm takes off q <= 3 multiples of r, 3 * 2^28 + 3 * 2^28 < 2^31 - 2^4.
//   combine two normalised partials: value below 3.02 r, limbs below 2^29, q <= 2.
//   Horner  t in device form, below 1.45 r.  x' = x t / R' + c with c below r: x' < 0.1604 x + 2 r, so x stays below 2.39 r; its limbs
//           are a normalised product plus a wire operand, below 2^29, which fp_mul takes as its first operand; x t < 3.5 r^2 < 4 r^2.
//           The run times t^(run start) (below 1.45 r) is again a product in [0, 1.39 r): two of them on a normalised accumulator are
//           below 4.3 r with limbs below 3 * 2^28, q <= 3.
//   finish  accumulator (below 1.51 r) times k_in (below r), fp_canon, fp_pack; a sum of polynomial runs is in R-form already (a
//           wire coefficient times t^i in device form is c t^i R): fp_canon, fp_pack.
// tools/host_dot_check.cpp runs these routines on the host at all-(r - 1) operands and asserts the bounds after every step.
#pragma once
#include "fp753.hip.h"

namespace mnt753 {

constexpr uint32_t RED_BLOCK = 256;         // threads per block of every kernel here
constexpr uint32_t RED_MAX_BLOCKS = 1024;   // blocks per launch at most: 4 per CU on 256 CUs; the partials are sized for it
constexpr uint32_t RED_BLOCKS_PER_CU = 4;
constexpr uint32_t POLY_RUN = 16;           // coefficients per Horner run (POW_RUN of k_vec_powers)

// acc += p limb-wise; every second term normalises
template <int M>
HD void red_add(Fp<M>& acc, uint32_t& pending, const Fp<M>& p) {
#pragma unroll
  for (int i = 0; i < NL; ++i) acc.l[i] += p.l[i];
  if (++pending == 2u) { fp_norm(acc, acc); pending = 0; }
}
template <int M>
HD void red_flush(Fp<M>& acc, uint32_t& pending) {
  if (pending) fp_norm(acc, acc);
  pending = 0;
}
// one term of an inner product: both operands unpacked wire words
template <int M>
HD void dot_step(Fp<M>& acc, uint32_t& pending, const Fp<M>& a_raw, const Fp<M>& u_raw) {
  Fp<M> p;
  fp_mul(p, a_raw, u_raw);
  red_add(acc, pending, p);
}
// a <- a + b, both flushed (normalised or zero)
template <int M>
HD void red_combine(Fp<M>& a, const Fp<M>& b) {
#pragma unroll
  for (int i = 0; i < NL; ++i) a.l[i] += b.l[i];
  fp_norm(a, a);
}
// x <- x t + c: t in device form, c an unpacked wire operand
template <int M>
HD void horner_step(Fp<M>& x, const Fp<M>& t, const Fp<M>& c_raw) {
  Fp<M> p;
  fp_mul(p, x, t);
#pragma unroll
  for (int i = 0; i < NL; ++i) x.l[i] = p.l[i] + c_raw.l[i];
}
// one run of a polynomial: x (the Horner value of the run) times pw = t^(run start) in device form, onto the accumulator
template <int M>
HD void poly_run_add(Fp<M>& acc, uint32_t& pending, const Fp<M>& x, const Fp<M>& pw) {
  Fp<M> p;
  fp_mul(p, x, pw);
  red_add(acc, pending, p);
}
// a flushed sum of products of wire operands -> canonical wire words
template <int M>
HD void red_finish(uint32_t w[24], const Fp<M>& acc) {
  Fp<M> k, t, c;
  fp_const_limbs(k, FPC[M].k_in);
  fp_mul(t, acc, k);
  fp_canon(c, t);
  fp_pack(w, c);
}
// a flushed sum of polynomial runs: already in R-form (a wire coefficient times t^i in device form is c t^i R)
template <int M>
HD void red_finish_plain(uint32_t w[24], const Fp<M>& acc) {
  Fp<M> c;
  fp_canon(c, acc);
  fp_pack(w, c);
}

}  // namespace mnt753

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "ntt_kernels.hip.h"

namespace mnt753 {

// the flushed accumulators of a block's 256 threads into thread 0 (every thread calls; `lds`: 4 * FPS_WORDS words)
template <int M>
__device__ __forceinline__ void red_block_sum(Fp<M>& acc, uint32_t* lds) {
#pragma unroll 1
  for (int off = 32; off > 0; off >>= 1) {
    Fp<M> o;
#pragma unroll
    for (int i = 0; i < NL; ++i) o.l[i] = (uint32_t)__shfl_down((int)acc.l[i], off, 64);
    red_combine(acc, o);      // lanes whose partner lies outside the wave add their own value: bounded, and never read
  }
  const uint32_t wave = threadIdx.x >> 6;
  __syncthreads();            // the previous use of lds is over
  if ((threadIdx.x & 63u) == 0) lds_store_fp(lds + wave * FPS_WORDS, acc);
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll 1
    for (uint32_t w = 1; w < RED_BLOCK / 64; ++w) {
      Fp<M> o;
      lds_load_fp(o, lds + w * FPS_WORDS);
      red_combine(acc, o);
    }
  }
}

struct DotVecs { const uint32_t* a[3]; };

template <int M>
__device__ __forceinline__ void dot_term(Fp<M>& acc, uint32_t& pending, const uint32_t* a_wire, const Fp<M>& u_raw) {
  uint32_t w[24];
  Fp<M> x;
  load_wire24(w, a_wire);
  fp_unpack(x, w);
  dot_step(acc, pending, x, u_raw);
}

// partial: gridDim.x * K elements of FPS_WORDS words, block b's sum for vector k at (b * K + k)
template <int M, int K>
__global__ void __launch_bounds__(RED_BLOCK) k_vec_dot(DotVecs v, const uint32_t* u, size_t n, uint32_t* __restrict__ partial) {
  __shared__ __align__(16) uint32_t lds[(RED_BLOCK / 64) * FPS_WORDS];
  Fp<M> acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) fp_zero(acc[k]);
  uint32_t pending = 0;
  const size_t stride = (size_t)gridDim.x * RED_BLOCK;
#pragma unroll 1
  for (size_t i = (size_t)blockIdx.x * RED_BLOCK + threadIdx.x; i < n; i += stride) {
    uint32_t w[24];
    Fp<M> y;
    load_wire24(w, u + i * 24);
    fp_unpack(y, w);
    // (spelled out: the compiler leaves a loop over k rolled, and the accumulators then live in scratch memory)
    uint32_t pk = pending;
    dot_term<M>(acc[0], pk, v.a[0] + i * 24, y);
    if constexpr (K > 1) { pk = pending; dot_term<M>(acc[1], pk, v.a[1] + i * 24, y); }
    if constexpr (K > 2) { pk = pending; dot_term<M>(acc[2], pk, v.a[2] + i * 24, y); }
    pending = pk;
  }
  const uint32_t left = pending;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (left) fp_norm(acc[k], acc[k]);
    red_block_sum(acc[k], lds);
    if (threadIdx.x == 0) fp_store(partial + ((size_t)blockIdx.x * K + k) * FPS_WORDS, acc[k]);
  }
}

template <int M>
__global__ void __launch_bounds__(RED_BLOCK) k_poly_eval(const uint32_t* __restrict__ c, size_t n, WireElem tw, uint32_t* __restrict__ partial) {
  __shared__ __align__(16) uint32_t lds[(RED_BLOCK / 64) * FPS_WORDS];
  Fp<M> t, acc;
  fp_from_wire(t, tw.w);
  fp_zero(acc);
  uint32_t pending = 0;
  const size_t runs = (n + POLY_RUN - 1) / POLY_RUN;
  const size_t stride = (size_t)gridDim.x * RED_BLOCK;
#pragma unroll 1
  for (size_t q = (size_t)blockIdx.x * RED_BLOCK + threadIdx.x; q < runs; q += stride) {
    const size_t i0 = q * POLY_RUN;
    const uint32_t len = (uint32_t)(n - i0 < POLY_RUN ? n - i0 : POLY_RUN);
    uint32_t w[24];
    Fp<M> x, cr, pw, tmp;
    load_wire24(w, c + (i0 + len - 1) * 24);
    fp_unpack(x, w);
#pragma unroll 1
    for (uint32_t k = len - 1; k-- > 0;) {
      load_wire24(w, c + (i0 + k) * 24);
      fp_unpack(cr, w);
      horner_step(x, t, cr);
    }
    fp_one(pw);
    int top = 63;
    while (top >= 0 && !((i0 >> top) & 1)) --top;
#pragma unroll 1
    for (int b = top; b >= 0; --b) {     // t^i0, most significant bit first
      fp_sqr(tmp, pw);
      pw = tmp;
      if ((i0 >> b) & 1) { fp_mul(tmp, pw, t); pw = tmp; }
    }
    poly_run_add(acc, pending, x, pw);
  }
  red_flush(acc, pending);
  red_block_sum(acc, lds);
  if (threadIdx.x == 0) fp_store(partial + (size_t)blockIdx.x * FPS_WORDS, acc);
}

// one block: out[k] = the sum over b < nb of partial[b * K + k], canonical wire form; products: the partials are sums of products of
// two wire operands (k_vec_dot), else of polynomial runs (k_poly_eval)
template <int M>
__global__ void __launch_bounds__(RED_BLOCK) k_red_fold(const uint32_t* __restrict__ partial, uint32_t nb, int K, int products, uint32_t* __restrict__ out) {
  __shared__ __align__(16) uint32_t lds[(RED_BLOCK / 64) * FPS_WORDS];
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    Fp<M> acc, x;
    fp_zero(acc);
#pragma unroll 1
    for (uint32_t b = threadIdx.x; b < nb; b += RED_BLOCK) {
      fp_load(x, partial + ((size_t)b * K + k) * FPS_WORDS);
      red_combine(acc, x);
    }
    red_block_sum(acc, lds);
    if (threadIdx.x == 0) {
      uint32_t w[24];
      if (products) red_finish(w, acc);
      else red_finish_plain(w, acc);
      store_wire24(out + 24 * k, w);
    }
  }
}

}  // namespace mnt753
#endif
