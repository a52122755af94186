// The kernels of the Groth16 generator that are its own; the QAP at t and the fixed-base walks are in
// qap_kernels.hip.h and batch_exp_kernels.hip.h.
//
//   k_keygen_combine   (beta At[i] + alpha Bt[i] + Ct[i]) c_i, c_i = 1 for i <= num_inputs and delta^-1 above: ABC and Lt of
//                      libsnark/zk_proof_systems/ppzksnark/r1cs_gg_ppzksnark/r1cs_gg_ppzksnark.tcc:252-274 as one vector.  The vectors
//                      are used as they lie in wire form (x R as an integer < r); beta, alpha and 1 in the device radix (k R') make
//                      the three-term product of fp_mul3 the wire form of the sum, with one reduction; the factor delta^-1 is one
//                      more product of the same kind.  No conversion of an input, none of the result.
//   k_nz_count / k_nz_scan / k_nz_write
//                      stable compaction of the non-zero elements of a vector.  One thread per element: the flag (any word set), the
//                      wave's ballot, its population count into shared memory -> one count per workgroup; ONE workgroup scans the
//                      counts (a run per thread, then the 256 run sums in shared memory) into
//                      exclusive offsets with the total behind them; the write kernel takes the flag again and puts element i at
//                      offset[workgroup] + waves before it + bits of the ballot below its lane.  No atomics: the positions are a
//                      function of the input alone.
//   k_scatter_rows     row j of the compacted result to row index[j] of the output (zeroed beforehand): one thread per 16 bytes.
#pragma once
#include <hip/hip_runtime.h>
#include "ntt_kernels.hip.h"

namespace mnt753 {

constexpr uint32_t NZ_BLOCK = 256;                 // elements (= threads) per workgroup of k_nz_count / k_nz_write
constexpr uint32_t NZ_WAVES = NZ_BLOCK / 64;       // gfx950: 64 lanes per wave

template <int M>
__global__ void __launch_bounds__(256) k_keygen_combine(const uint32_t* at, const uint32_t* bt, const uint32_t* ct, uint32_t* out, WireElem beta_w,
                                                        WireElem alpha_w, WireElem dinv_w, size_t n, size_t num_inputs) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[24];
  Fp<M> a, b, c, beta, alpha, one, s;
  load_wire24(w, at + i * 24);
  fp_unpack(a, w);
  load_wire24(w, bt + i * 24);
  fp_unpack(b, w);
  load_wire24(w, ct + i * 24);
  fp_unpack(c, w);
  fp_from_wire(beta, beta_w.w);
  fp_from_wire(alpha, alpha_w.w);
  fp_one(one);
  fp_mul3(s, beta, a, alpha, b, one, c);           // (beta a + alpha b + c) R, lazily in [0, 2r)
  if (i > num_inputs) {
    Fp<M> dinv, t;
    fp_from_wire(dinv, dinv_w.w);
    fp_mul(t, dinv, s);
    s = t;
  }
  Fp<M> canon;
  fp_canon(canon, s);
  fp_pack(w, canon);
  store_wire24(out + i * 24, w);
}

// any of the 12 words of element i set; elements at and beyond n count as zero
__device__ __forceinline__ bool nz_flag(const uint64_t* __restrict__ v, size_t i, size_t n) {
  if (i >= n) return false;
  const ulonglong2* p = reinterpret_cast<const ulonglong2*>(v + 12 * i);   // 96-byte elements: 16-byte aligned
  uint64_t o = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const ulonglong2 q = p[k];
    o |= q.x | q.y;
  }
  return o != 0;
}

__global__ void __launch_bounds__(NZ_BLOCK) k_nz_count(const uint64_t* __restrict__ v, size_t n, uint32_t* __restrict__ block_count) {
  __shared__ uint32_t wave_count[NZ_WAVES];
  const size_t i = (size_t)blockIdx.x * NZ_BLOCK + threadIdx.x;
  const uint64_t ballot = __ballot(nz_flag(v, i, n));
  if ((threadIdx.x & 63u) == 0) wave_count[threadIdx.x >> 6] = (uint32_t)__popcll(ballot);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < NZ_WAVES; ++k) s += wave_count[k];
    block_count[blockIdx.x] = s;
  }
}

// one workgroup: count[0 .. nb) -> exclusive prefix sums in place, the total into count[nb].  Thread t owns the run
// [t * run, (t + 1) * run); the 256 run sums are scanned in shared memory (Hillis-Steele, 8 steps).
__global__ void __launch_bounds__(256) k_nz_scan(uint32_t* __restrict__ count, uint32_t nb) {
  __shared__ uint32_t sums[256];
  const uint32_t t = threadIdx.x, run = (nb + 255u) / 256u;
  const uint32_t lo = min(t * run, nb), hi = min(lo + run, nb);
  uint32_t s = 0;
  for (uint32_t k = lo; k < hi; ++k) s += count[k];
  sums[t] = s;
  __syncthreads();
  for (uint32_t step = 1; step < 256u; step <<= 1) {
    const uint32_t add = t >= step ? sums[t - step] : 0u;
    __syncthreads();
    sums[t] += add;
    __syncthreads();
  }
  uint32_t off = sums[t] - s;                      // exclusive prefix of this thread's run
  for (uint32_t k = lo; k < hi; ++k) {
    const uint32_t c = count[k];
    count[k] = off;
    off += c;
  }
  if (t == 255u) count[nb] = sums[255];
}

__global__ void __launch_bounds__(NZ_BLOCK) k_nz_write(const uint64_t* __restrict__ v, size_t n, const uint32_t* __restrict__ block_offset,
                                                       uint64_t* __restrict__ compact, uint32_t* __restrict__ index) {
  __shared__ uint32_t wave_count[NZ_WAVES];
  const size_t i = (size_t)blockIdx.x * NZ_BLOCK + threadIdx.x;
  const bool flag = nz_flag(v, i, n);
  const uint64_t ballot = __ballot(flag);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) wave_count[wave] = (uint32_t)__popcll(ballot);
  __syncthreads();
  if (!flag) return;
  uint32_t pos = block_offset[blockIdx.x] + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
  for (uint32_t k = 0; k < wave; ++k) pos += wave_count[k];
  const ulonglong2* src = reinterpret_cast<const ulonglong2*>(v + 12 * i);
  ulonglong2* dst = reinterpret_cast<ulonglong2*>(compact + 12 * (size_t)pos);
#pragma unroll
  for (int k = 0; k < 6; ++k) dst[k] = src[k];
  index[pos] = (uint32_t)i;
}

// rows of `pairs` 16-byte pairs; thread (j, k) copies pair k of compacted row j
__global__ void __launch_bounds__(256) k_scatter_rows(const ulonglong2* __restrict__ rows, const uint32_t* __restrict__ index, size_t count, uint32_t pairs,
                                                      ulonglong2* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t j = t / pairs;
  if (j >= count) return;
  const uint32_t k = (uint32_t)(t - j * pairs);
  out[(size_t)index[j] * pairs + k] = rows[j * pairs + k];
}

}  // namespace mnt753
