// The QAP at a point for gfx950: the Lagrange coefficients of an evaluation domain at t, the powers of t, and the column sums
// At / Bt / Ct of a constraint system.
//
// Replaces libfqfft's evaluate_all_lagrange_polynomials (basic_radix2_domain_aux.tcc:333-395, extended_radix2_domain.tcc:120-139,
// step_radix2_domain.tcc:189-214) and the loops of r1cs_to_qap_instance_map_with_evaluation (libsnark/reductions/r1cs_to_qap/
// r1cs_to_qap.tcc:110-159).  Same field elements in the wire format; the schedule is the device's:
//
//   k_lagrange_run        a multiplicative subgroup of order n with generator omega: u_i = c omega^i / (t - omega^i), c = Z / n times the
//                         coefficient of the half (extended, step) on the host.  n inversions in the reference; here Montgomery's
//                         simultaneous inversion over runs of B consecutive indices per thread, the shape of k_fb_normalise
//                         (batch_exp_kernels.hip.h): prefix products of the denominators into `pre`, one fp_inv, and the walk back.
//                         omega^i comes from the domain's twiddle table (half a table: the other half is the negation).  STEP: the big
//                         half of a step domain carries the second factor 1 / (omega_big^(i small_m) - omega^small_m) per element
//                         (step_radix2_domain.tcc:199-204); it joins the denominator of the same inversion.
//                         The caller guarantees t^n != 1: no denominator is zero.
//   k_lagrange_indicator  t inside the subgroup (t^n = 1, decided on the host): the reference returns the indicator vector of the
//                         matching index (basic_radix2_domain_aux.tcc:353-366); every thread compares its omega^i with t and writes
//                         the (scaled) one or zero.  Nothing is inverted.
//   k_vec_powers          1, t, .., t^(n-1): a thread raises t to the first index of its run by squaring and walks the run by products.
//   k_qap_chunks          one thread per chunk of a column (qap_transpose.hpp), chunks by decreasing length: the arithmetic of
//                         k_r1cs_evaluate -- coefficient in the device radix times u as it lies in wire form, limb-wise sums, one
//                         fp_norm per two terms -- into one partial sum per chunk.
//   k_qap_fold            one thread per column: the partial sums of its chunks, the seed u[nc + i] of At (r1cs_to_qap.tcc:130-133),
//                         canonical wire form; a column without terms is written as zero.
#pragma once
#include <hip/hip_runtime.h>
#include "fp_inv.hip.h"
#include "ntt_kernels.hip.h"

namespace mnt753 {

constexpr uint32_t LAG_INV_BATCH = 16;    // indices per inversion: the run length of k_fb_normalise (FB_INV_BATCH)
constexpr uint32_t POW_RUN = 16;          // powers per thread of k_vec_powers

// omega^i from a table of omega^j, j < n / 2 (half: the upper half is the negation) or j < n
template <int M>
__device__ __forceinline__ void lag_root(Fp<M>& w, const uint32_t* __restrict__ tab, size_t i, size_t n, bool half) {
  if (half && i >= n / 2) {
    Fp<M> v;
    fp_load(v, tab + (i - n / 2) * FPS_WORDS);
    fp_neg(w, v);
  } else {
    fp_load(w, tab + i * FPS_WORDS);
  }
}
// the denominator of index i: t - omega^i, times omega_big^(i stride) - os in the big half of a step domain (n a power of two there)
template <int M, bool STEP>
__device__ __forceinline__ void lag_denominator(Fp<M>& d, Fp<M>& w, const uint32_t* __restrict__ tab, size_t i, size_t n, bool half, const Fp<M>& t,
                                                const Fp<M>& os, size_t stride) {
  lag_root<M>(w, tab, i, n, half);
  fp_sub(d, t, w);
  if constexpr (STEP) {
    Fp<M> e, f;
    lag_root<M>(e, tab, (i * stride) & (n - 1), n, half);
    fp_sub(f, e, os);
    fp_mul(e, d, f);
    d = e;
  }
}

template <int M, bool STEP>
__global__ void __launch_bounds__(256) k_lagrange_run(const uint32_t* __restrict__ tab, size_t n, int half, uint32_t* __restrict__ pre,
                                                      uint32_t* __restrict__ out, WireElem tw, WireElem cw, WireElem osw, size_t stride) {
  constexpr uint32_t B = LAG_INV_BATCH;
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q * B >= n) return;
  const size_t i0 = q * B;
  const uint32_t len = (uint32_t)(n - i0 < B ? n - i0 : B);
  Fp<M> t, os, run, d, w, tmp, inv;
  fp_from_wire(t, tw.w);
  fp_from_wire(os, osw.w);
  fp_one(run);
#pragma unroll 1
  for (uint32_t k = 0; k < len; ++k) {
    fp_store(pre + (i0 + k) * FPS_WORDS, run);
    lag_denominator<M, STEP>(d, w, tab, i0 + k, n, half != 0, t, os, stride);
    fp_mul(tmp, run, d);
    run = tmp;
  }
  fp_inv(inv, run);
  Fp<M> c;
  fp_from_wire(c, cw.w);
#pragma unroll 1
  for (uint32_t k = len; k-- > 0;) {
    lag_denominator<M, STEP>(d, w, tab, i0 + k, n, half != 0, t, os, stride);
    fp_load(tmp, pre + (i0 + k) * FPS_WORDS);
    Fp<M> di, u;
    fp_mul(di, inv, tmp);        // 1 / d_i
    fp_mul(tmp, inv, d);         // the inverse of the shorter prefix
    inv = tmp;
    fp_mul(u, c, w);
    fp_mul(tmp, u, di);
    uint32_t wr[24];
    fp_to_wire(wr, tmp);
    store_wire24(out + (i0 + k) * 24, wr);
  }
}

// out[i] = value where omega^i == t, zero elsewhere; tab == nullptr: the subgroup of order 1, whose only element is 1 == t
template <int M>
__global__ void __launch_bounds__(256) k_lagrange_indicator(const uint32_t* __restrict__ tab, size_t n, int half, uint32_t* __restrict__ out, WireElem tw,
                                                            WireElem value) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool hit = true;
  if (tab) {
    Fp<M> t, w, a, b;
    fp_from_wire(t, tw.w);
    lag_root<M>(w, tab, i, n, half != 0);
    fp_canon(a, t);
    fp_canon(b, w);
    uint32_t diff = 0;
#pragma unroll
    for (int j = 0; j < NL; ++j) diff |= a.l[j] ^ b.l[j];
    hit = diff == 0;
  }
  uint32_t wr[24];
#pragma unroll
  for (int j = 0; j < 24; ++j) wr[j] = hit ? value.w[j] : 0u;
  store_wire24(out + i * 24, wr);
}

template <int M>
__global__ void __launch_bounds__(256) k_vec_powers(uint32_t* __restrict__ out, WireElem tw, size_t n) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q * POW_RUN >= n) return;
  const size_t i0 = q * POW_RUN;
  const uint32_t len = (uint32_t)(n - i0 < POW_RUN ? n - i0 : POW_RUN);
  Fp<M> t, acc, tmp;
  fp_from_wire(t, tw.w);
  fp_one(acc);
  int top = 63;
  while (top >= 0 && !((i0 >> top) & 1)) --top;
#pragma unroll 1
  for (int b = top; b >= 0; --b) {     // t^i0, most significant bit first
    fp_sqr(tmp, acc);
    acc = tmp;
    if ((i0 >> b) & 1) { fp_mul(tmp, acc, t); acc = tmp; }
  }
#pragma unroll 1
  for (uint32_t k = 0; k < len; ++k) {
    uint32_t wr[24];
    fp_to_wire(wr, acc);
    store_wire24(out + (i0 + k) * 24, wr);
    fp_mul(tmp, acc, t);
    acc = tmp;
  }
}

// the matrices of a constraint system as the chunk kernel reads them
struct QapMatrices {
  const uint32_t* coeff[3];      // device radix, FPS_WORDS per term, row-major (mnt753_r1cs)
  uint64_t base1, base2;         // first term of b and of c in the permutation
};

template <int M>
__global__ void __launch_bounds__(256) k_qap_chunks(QapMatrices mats, const uint32_t* __restrict__ perm_row, const uint32_t* __restrict__ perm_k,
                                                    const uint64_t* __restrict__ chunk_start, const uint32_t* __restrict__ chunk_len,
                                                    const uint32_t* __restrict__ order, const uint32_t* __restrict__ u_wire, uint32_t* __restrict__ partial,
                                                    uint64_t n_chunks) {
  const uint64_t tix = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tix >= n_chunks) return;
  const uint32_t chunk = order[tix];
  const uint64_t start = chunk_start[chunk];
  const uint32_t len = chunk_len[chunk];
  const int which = start >= mats.base2 ? 2 : (start >= mats.base1 ? 1 : 0);
  const uint32_t* cf = which == 0 ? mats.coeff[0] : (which == 1 ? mats.coeff[1] : mats.coeff[2]);
  Fp<M> acc, c, x, p;
  fp_zero(acc);
  uint32_t pending = 0, wv[24];
#pragma unroll 1
  for (uint64_t j = start; j < start + len; ++j) {
    load_wire24(wv, u_wire + 24 * (size_t)perm_row[j]);
    fp_unpack(x, wv);                                        // u R as an integer < r
    fp_load(c, cf + (size_t)perm_k[j] * FPS_WORDS);          // c R'
    fp_mul(p, c, x);                                         // c u R, lazily in [0, 1.2211 r): c < 2r, x < r (fp_mul's contract)
#pragma unroll
    for (int i = 0; i < NL; ++i) acc.l[i] += p.l[i];
    // a flushed value and two products: < 1.51 r + 2 * 1.2211 r = 3.9522 r, limbs < 3 2^28, |q| <= 3 -- inside fp_norm's contract.  The
    // loop of k_r1cs_evaluate (csrc/mnt753_r1cs.hip) over u; tools/host_r1cs_check.cpp MIRRORS both (change them together) and asserts
    // the bounds on the designed operands: largest product 1.027 r / 1.103 r (MNT4753 / MNT6753), largest accumulator 3.443 r / 3.372 r
    if (++pending == 2u) { fp_norm(acc, acc); pending = 0; }
  }
  if (pending) fp_norm(acc, acc);
  fp_store(partial + (size_t)chunk * FPS_WORDS, acc);
}

template <int M>
__global__ void __launch_bounds__(256) k_qap_fold(const uint32_t* __restrict__ partial, const uint64_t* __restrict__ col_chunk, const uint32_t* __restrict__ u_wire,
                                                  uint32_t* __restrict__ at, uint32_t* __restrict__ bt, uint32_t* __restrict__ ct, uint64_t ncols, uint64_t nc,
                                                  uint64_t num_inputs) {
  const uint64_t tix = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tix >= 3 * ncols) return;
  const int which = (int)(tix / ncols);
  const uint64_t col = tix - (uint64_t)which * ncols;
  Fp<M> acc, x;
  fp_zero(acc);
  uint32_t pending = 0, wv[24];
  if (which == 0 && col <= num_inputs) {                     // At[i] = u[nc + i], the input-consistency rows
    load_wire24(wv, u_wire + 24 * (size_t)(nc + col));
    fp_unpack(acc, wv);
    pending = 1;
  }
#pragma unroll 1
  for (uint64_t j = col_chunk[tix]; j < col_chunk[tix + 1]; ++j) {
    fp_load(x, partial + (size_t)j * FPS_WORDS);             // [0.49 r, 1.51 r)
#pragma unroll
    for (int i = 0; i < NL; ++i) acc.l[i] += x.l[i];
    // a flushed value (or the seed, < r) and two partial sums: < 3 * 1.51 r = 4.53 r, limbs < 3 2^28, |q| <= 4 -- inside fp_norm's
    // contract (|value| < 5 r, |limb| + 2^28 |q| < 2^31 - 2^4), with less room than the term loops have.  tools/host_r1cs_check.cpp
    // MIRRORS this loop (change them together); the largest it saw: 4.266 r / 4.494 r (MNT4753 / MNT6753), limb 3.000 2^28, |q| 3
    if (++pending == 2u) { fp_norm(acc, acc); pending = 0; }
  }
  if (pending) fp_norm(acc, acc);
  Fp<M> canon;
  fp_canon(canon, acc);
  fp_pack(wv, canon);
  store_wire24((which == 0 ? at : (which == 1 ? bt : ct)) + 24 * col, wv);
}

}  // namespace mnt753
