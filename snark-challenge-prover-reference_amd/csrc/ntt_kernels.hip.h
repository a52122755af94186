// Radix-2 NTT over Fr for gfx950.
//
// Replaces libfqfft's basic_radix2_domain on the device (reference:
// depends/libfqfft/libfqfft/evaluation_domain/domains/basic_radix2_domain.tcc:62-134 and
// basic_radix2_domain_aux.tcc:167-202 _basic_serial_radix2_FFT, :321-330 _multiply_by_coset).
// Same transform (bit-reversal, then log2 m decimation-in-time passes); GPU-native schedule:
//
//   * vectors stay in HBM in the wire format (96 B / element, Montgomery R = 2^768).  Twiddles and coset
//     powers are precomputed once per domain in the device form (Montgomery R' = 2^756), and a Montgomery
//     product  mul'(w * R', x * R) = (w x) * R  leaves the data in wire form -- so the transform never
//     converts its data between the two Montgomery radices.
//   * k_ntt_group runs up to 8 consecutive butterfly stages on a 2^ns-element tile held in LDS
//     (27 limbs + 1 pad word = 112 B per element: a 112-byte stride maps 16 consecutive lanes'
//     ds_read_b128 onto 16 distinct bank groups), so a 2^20-point transform makes 3 passes over HBM
//     instead of 20.  The first group gathers its input in bit-reversed order (no separate permutation pass).
//   * the libfqfft scale loops (1/m, g^i, g^-i, 1/Z) are table multiplies fused pairwise.
#pragma once
#include <hip/hip_runtime.h>
#include "fp753.hip.h"
#include "msm_kernels.hip.h"   // storage helpers (fp_load / fp_store / load_wire24 / store_wire24)

namespace mnt753 {

#ifndef MNT753_NTT_LAZY
#define MNT753_NTT_LAZY 1
#endif
constexpr int NTT_MAX_NS = 8;                 // stages per LDS group
constexpr int NTT_BLOCK = 256;                // threads per block = 512 elements per block
constexpr int NTT_LDS_WORDS = 2 * NTT_BLOCK * FPS_WORDS;

template <int M>
__device__ __forceinline__ void lds_load_fp(Fp<M>& r, const uint32_t* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    uint4 v = q[i];
    r.l[4 * i] = v.x; r.l[4 * i + 1] = v.y; r.l[4 * i + 2] = v.z;
    if (4 * i + 3 < NL) r.l[4 * i + 3] = v.w;
  }
}
template <int M>
__device__ __forceinline__ void lds_store_fp(uint32_t* p, const Fp<M>& a) {
  uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (int i = 0; i < 7; ++i)
    q[i] = make_uint4(a.l[4 * i], a.l[4 * i + 1], a.l[4 * i + 2], (4 * i + 3 < NL) ? a.l[4 * i + 3] : 0u);
}

// stages [s0, s0 + ns) of the decimation-in-time transform of size 2^logm.
//   src/dst: wire vectors (may alias unless bitrev is set);  tw: omega^i, i < m/2, device form.
//   in_scale / out_scale (may be null): tables in device form the elements are multiplied by as they are read (index = the element's
//   position in `src`) / written (position in `dst`) -- libfqfft's coset and 1/m loops ride on the transform's own passes over HBM
//   instead of a pass of their own (k_vec_mul_table: 0.10 ms per 2^20 elements, four of them in compute_H).  A product of a canonical
//   element and a table entry below 2p is below 1.22p, inside the range the first carry-free stage assumes.
//   (IN_SCALE / OUT_SCALE are template switches: the plain transform keeps the code and the registers it had without them -- with
//   run-time null checks alone the 2^20 FFT measured 0.80 ms against 0.76.)
template <int M, bool IN_SCALE, bool OUT_SCALE>
__global__ void __launch_bounds__(NTT_BLOCK) k_ntt_group(const uint32_t* src, uint32_t* dst,
                                                        const uint32_t* __restrict__ tw, int logm, int s0, int ns, int bitrev,
                                                        const uint32_t* __restrict__ in_scale, const uint32_t* __restrict__ out_scale) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[NTT_LDS_WORDS];
  const int tpt = 1 << (ns - 1);                       // threads (= butterflies) per tile
  const int tiles_per_block = NTT_BLOCK / tpt;
  const int tile_in_block = threadIdx.x / tpt, bt = threadIdx.x % tpt;
  const size_t n_tiles = (size_t)1 << (logm - ns);
  const size_t tile = (size_t)blockIdx.x * tiles_per_block + tile_in_block;
  const bool active = tile < n_tiles;
  const size_t lo = tile & (((size_t)1 << s0) - 1), hi = tile >> s0;
  const size_t base_idx = (hi << (s0 + ns)) + lo;      // element e of the tile sits at base_idx + (e << s0)
  uint32_t* my = lds + (size_t)tile_in_block * ((size_t)FPS_WORDS << ns);
  if (active) {
#pragma unroll 1
    for (int r = 0; r < 2; ++r) {
      const int e = bt + r * tpt;
      size_t idx = base_idx + ((size_t)e << s0);
      if (bitrev) idx = (size_t)(__brevll((unsigned long long)idx) >> (64 - logm));
      uint32_t w[24];
      load_wire24(w, src + idx * 24);
      Fp<M> x;
      fp_unpack(x, w);
      if constexpr (IN_SCALE) {
        Fp<M> k, y;
        fp_load(k, in_scale + idx * FPS_WORDS);
        fp_mul(y, x, k);
        x = y;
      }
      lds_store_fp(my + e * FPS_WORDS, x);
    }
  }
  __syncthreads();
  // the twiddle of a stage is fetched one stage ahead (its address needs nothing the stage computes): the load's latency then
  // hides behind a product instead of standing between the barrier and the product
  auto twiddle_index = [=](int q) -> size_t {
    const int e_lo = ((bt >> q) << (q + 1)) | (bt & ((1 << q) - 1));
    const size_t j = ((size_t)(e_lo & ((1 << q) - 1)) << s0) + lo;
    return j << (logm - 1 - (s0 + q));
  };
  Fp<M> w, w_next;
  fp_zero(w_next);
  if (active && s0 != 0) fp_load(w_next, tw + twiddle_index(0) * FPS_WORDS);
#pragma unroll 1
  for (int q = 0; q < ns; ++q) {
    if (active) {
      const int e_lo = ((bt >> q) << (q + 1)) | (bt & ((1 << q) - 1));
      const int e_hi = e_lo + (1 << q);
      Fp<M> xl, xh, t;
      w = w_next;
      if (q + 1 < ns) fp_load(w_next, tw + twiddle_index(q + 1) * FPS_WORDS);
      lds_load_fp(xl, my + e_lo * FPS_WORDS);
      lds_load_fp(xh, my + e_hi * FPS_WORDS);
#if MNT753_NTT_LAZY
      // Carry-free butterflies (the lazy arithmetic of the pairing levels, fp753.hip.h): x_lo +- w x_hi limb-wise with signed limbs
      // (54 instructions instead of the 540 of fp_add + fp_sub), the product through the signed multiplier, and one normalisation
      // per element every SECOND stage.  Ranges (p / R' < 0.1106 for both moduli): stage A takes values in [0, 1.51p) with limbs
      // below 2^28 (fresh from fp_unpack or fp_norm) and a twiddle in [0, 2p): t in [0, 1.34p), outputs in (-1.34p, 2.85p) with
      // |limb| < 2^29; stage B takes those: t in (-0.30p, 1.63p), outputs in (-2.97p, 4.48p) with |limb| < 3 * 2^28.  The first
      // stage of the transform (s0 + q == 0, below) takes t = x_hi itself, in [0, 1.51p): its outputs lie in (-1.51p, 3.02p), and
      // the stage B behind it gives t in (-0.34p, 1.67p), outputs in (-3.18p, 4.69p) with |limb| < 3 * 2^28.  All of it inside what
      // fp_norm accepts (|value| < 5p; |limb| + 2^28 |q| < 2^31 - 2^4 with |q| <= 4 here), which returns them to [0.49p, 1.51p).
      // Values mod p are those of the eager form.  (tests/test_field_raw_*.py assert these ranges, both first-stage forms, at
      // their edges.)
      if (s0 + q == 0) {
        t = xh;                                        // the first stage's only twiddle is omega^0 (block-uniform: one product in twenty saved)
      } else {
        fp_mul_s(t, w, xh);
      }
      fp_sub_raw(xh, xl, t);
      fp_addsub_raw(xl, xl, t, false);
      if ((q & 1) || q == ns - 1) { fp_norm(xl, xl); fp_norm(xh, xh); }
#else
      if (s0 + q == 0) {
        t = xh;
      } else {
        fp_mul(t, w, xh);
      }
      fp_sub(xh, xl, t);
      fp_add(xl, xl, t);
#endif
      lds_store_fp(my + e_lo * FPS_WORDS, xl);
      lds_store_fp(my + e_hi * FPS_WORDS, xh);
    }
    __syncthreads();
  }
  if (active) {
#pragma unroll 1
    for (int r = 0; r < 2; ++r) {
      const int e = bt + r * tpt;
      const size_t idx = base_idx + ((size_t)e << s0);
      Fp<M> x, c;
      lds_load_fp(x, my + e * FPS_WORDS);
      if constexpr (OUT_SCALE) {
        Fp<M> k, y;
        fp_load(k, out_scale + idx * FPS_WORDS);
        fp_mul(y, x, k);
        x = y;
      }
      fp_canon(c, x);
      uint32_t w[24];
      fp_pack(w, c);
      store_wire24(dst + idx * 24, w);
    }
  }
}

// size-1 ... special case is handled on the host (m == 1 is the identity transform).

// a[i] = a[i] * table[i]      (table in device form; a in wire form)
template <int M>
__global__ void __launch_bounds__(256) k_vec_mul_table(uint32_t* __restrict__ a, const uint32_t* __restrict__ table, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[24];
  load_wire24(w, a + i * 24);
  Fp<M> x, t, r, c;
  fp_unpack(x, w);
  fp_load(t, table + i * FPS_WORDS);
  fp_mul(r, x, t);
  fp_canon(c, r);
  fp_pack(w, c);
  store_wire24(a + i * 24, w);
}

// a[i] = a[i] * k              (k: one element in device form, in global memory)
template <int M>
__global__ void __launch_bounds__(256) k_vec_mul_const(uint32_t* __restrict__ a, const uint32_t* __restrict__ k, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[24];
  load_wire24(w, a + i * 24);
  Fp<M> x, t, r, c;
  fp_unpack(x, w);
  fp_load(t, k);
  fp_mul(r, x, t);
  fp_canon(c, r);
  fp_pack(w, c);
  store_wire24(a + i * 24, w);
}

// a[i] = a[i] * b[i]           both wire form: mul' gives ab*R*2^12, a second mul' by 2^744 restores ab*R
template <int M>
__global__ void __launch_bounds__(256) k_vec_muleq(uint32_t* __restrict__ a, const uint32_t* __restrict__ b, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[24];
  Fp<M> x, y, t, r, k, c;
  load_wire24(w, a + i * 24);
  fp_unpack(x, w);
  load_wire24(w, b + i * 24);
  fp_unpack(y, w);
  fp_mul(t, x, y);
  fp_const_limbs(k, FPC[M].k_in);
  fp_mul(r, t, k);
  fp_canon(c, r);
  fp_pack(w, c);
  store_wire24(a + i * 24, w);
}

// dst[i] = src[i] * k          all wire form, k passed by value (one element, 24 words); dst may be src
struct WireElem { uint32_t w[24]; };
template <int M>
__global__ void __launch_bounds__(256) k_vec_scale(uint32_t* __restrict__ dst, const uint32_t* src, WireElem kw, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[24];
  Fp<M> x, y, t, r, k, c;
  load_wire24(w, src + i * 24);
  fp_unpack(x, w);
  fp_unpack(y, kw.w);
  fp_mul(t, x, y);
  fp_const_limbs(k, FPC[M].k_in);
  fp_mul(r, t, k);
  fp_canon(c, r);
  fp_pack(w, c);
  store_wire24(dst + i * 24, w);
}

// a[i] = a[i] - b[i]
template <int M>
__global__ void __launch_bounds__(256) k_vec_subeq(uint32_t* __restrict__ a, const uint32_t* __restrict__ b, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[24];
  Fp<M> x, y, r, c;
  load_wire24(w, a + i * 24);
  fp_unpack(x, w);
  load_wire24(w, b + i * 24);
  fp_unpack(y, w);
  fp_sub(r, x, y);
  fp_canon(c, r);
  fp_pack(w, c);
  store_wire24(a + i * 24, w);
}

// compute_H pointwise step, fused:  a[i] = (a[i]*b[i] - c[i]) / Z      (cuda_prover_piecewise.cu:35-45)
//   k1 = 2^12 * R'  (lifts c to the same 2^12-shifted radix as mul'(a,b)),  k2 = Z^-1 * R' * 2^-12
template <int M>
__global__ void __launch_bounds__(256) k_h_pointwise(uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                    const uint32_t* __restrict__ cvec, const uint32_t* __restrict__ k1,
                                                    const uint32_t* __restrict__ k2, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[24];
  Fp<M> x, y, z, ab, cz, d, kk, r, c;
  load_wire24(w, a + i * 24);
  fp_unpack(x, w);
  load_wire24(w, b + i * 24);
  fp_unpack(y, w);
  load_wire24(w, cvec + i * 24);
  fp_unpack(z, w);
  fp_mul(ab, x, y);
  fp_load(kk, k1);
  fp_mul(cz, z, kk);
  fp_sub(d, ab, cz);
  fp_load(kk, k2);
  fp_mul(r, d, kk);
  fp_canon(c, r);
  fp_pack(w, c);
  store_wire24(a + i * 24, w);
}

// out[i] = scale * base^i in device form.  pow2[k] = base^(2^k) and scale arrive in wire form.
template <int M>
__global__ void __launch_bounds__(256) k_pow_table(uint32_t* __restrict__ out, const uint32_t* __restrict__ pow2_wire,
                                                  const uint32_t* __restrict__ scale_wire, size_t n, int nbits) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[24];
  Fp<M> acc, f, t;
  load_wire24(w, scale_wire);
  fp_from_wire(acc, w);
#pragma unroll 1
  for (int k = 0; k < nbits; ++k) {
    if ((i >> k) & 1) {
      load_wire24(w, pow2_wire + 24 * k);
      fp_from_wire(f, w);
      fp_mul(t, acc, f);
      acc = t;
    }
  }
  fp_store(out + i * FPS_WORDS, acc);
}

// wire element -> device form (single constants)
template <int M>
__global__ void k_consts_to_internal(uint32_t* __restrict__ out, const uint32_t* __restrict__ wire, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[24];
  load_wire24(w, wire + 24 * i);
  Fp<M> v;
  fp_from_wire(v, w);
  fp_store(out + i * FPS_WORDS, v);
}

// ---- step and extended radix-2 domains (libfqfft step_radix2_domain.tcc, extended_radix2_domain.tcc) ---------------------------
// A domain of size big_m + small_m (step) or 2 * small_m (extended) is two radix-2 transforms (k_ntt_group, unchanged) with one
// O(m) pass in front of them (forward) or behind them (inverse).  The passes are out of place -- vec -> work in front, work -> vec
// behind -- so the inner transforms read one buffer and write the other and no pass needs a copy.  Wire in, wire out; tables in
// device form; one element (pair) per lane.  COSET multiplies by g^k on the way in (forward) / g^-k on the way out (inverse), the
// _multiply_by_coset of cosetFFT / icosetFFT.

template <int M>
__device__ __forceinline__ void load_wire_fp(Fp<M>& x, const uint32_t* p) {
  uint32_t w[24];
  load_wire24(w, p);
  fp_unpack(x, w);
}
template <int M>
__device__ __forceinline__ void store_wire_fp(uint32_t* p, const Fp<M>& x) {
  Fp<M> c;
  uint32_t w[24];
  fp_canon(c, x);
  fp_pack(w, c);
  store_wire24(p, w);
}
template <int M>
__device__ __forceinline__ void mul_table(Fp<M>& x, const uint32_t* entry) {
  Fp<M> k, y;
  fp_load(k, entry);
  fp_mul(y, x, k);
  x = y;
}

// Step, forward:  out[k] = c[k] = a[k] (+ a[k + big_m] for k < small_m),  k < big_m
//                 out[big_m + i] = e[i] = sum_j d[i + j small_m],  d[k] = omega^k (a[k] (- a[k + big_m] for k < small_m))
// Mapping: a block is ti_n x tj_n threads; thread (ti, tj) of block b owns output i = b ti_n + ti and walks j = tj, tj + tj_n, ...
// ti is the fast index, so the lanes of a wave read consecutive elements k = i + j small_m for every j (and where small_m < 64,
// k = threadIdx.x itself): each load of the strided fold is coalesced.  The tj_n partial sums of one output meet in LDS.
// The host picks ti_n = min(small_m, 64), tj_n = min(compr, 256 / ti_n); both powers of two, ti_n divides small_m.
template <int M, bool COSET>
__global__ void __launch_bounds__(256) k_step_pre(const uint32_t* __restrict__ a, uint32_t* __restrict__ out,
                                                 const uint32_t* __restrict__ om, const uint32_t* __restrict__ cos,
                                                 size_t big_m, size_t small_m, int ti_n, int tj_n) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[256 * FPS_WORDS];
  const int ti = threadIdx.x % ti_n, tj = threadIdx.x / ti_n;
  const size_t i = (size_t)blockIdx.x * ti_n + ti;            // < small_m: ti_n divides small_m
  const size_t compr = big_m / small_m;
  Fp<M> acc;
  fp_zero(acc);
#pragma unroll 1
  for (size_t j = tj; j < compr; j += tj_n) {
    const size_t k = i + j * small_m;
    Fp<M> x, c, dd;
    load_wire_fp(x, a + k * 24);
    if constexpr (COSET) mul_table(x, cos + k * FPS_WORDS);
    if (j == 0) {
      Fp<M> y;
      load_wire_fp(y, a + (k + big_m) * 24);
      if constexpr (COSET) mul_table(y, cos + (k + big_m) * FPS_WORDS);
      fp_add(c, x, y);
      fp_sub(dd, x, y);
    } else {
      c = x;
      dd = x;
    }
    store_wire_fp(out + k * 24, c);
    mul_table(dd, om + k * FPS_WORDS);
    fp_add(c, acc, dd);
    acc = c;
  }
  lds_store_fp(lds + threadIdx.x * FPS_WORDS, acc);
  __syncthreads();
  if (tj == 0) {
#pragma unroll 1
    for (int q = 1; q < tj_n; ++q) {
      Fp<M> t, s;
      lds_load_fp(t, lds + (q * ti_n + ti) * FPS_WORDS);
      fp_add(s, acc, t);
      acc = s;
    }
    store_wire_fp(out + (big_m + i) * 24, acc);
  }
}

// Step, inverse, behind the two inverse transforms (w = their raw outputs):
//   U0[k] = w[k] / big_m;  a[k] = U0[k] for k >= small_m
//   U1[i] = (w[big_m + i] / small_m - sum_{j >= 1} omega^k U0[k]) omega^-i,  k = i + j small_m
//   a[i] = (U0[i] + U1[i]) / 2;  a[big_m + i] = (U0[i] - U1[i]) / 2
// The halves ride in the tables: om_s[k] = omega^k / (2 big_m), om_inv[i] = omega^-i, kc = {1 / (2 big_m), 1 / (2 small_m), 1 / big_m}.
// Same thread mapping as k_step_pre.
template <int M, bool COSET>
__global__ void __launch_bounds__(256) k_step_post(const uint32_t* __restrict__ w, uint32_t* __restrict__ a,
                                                  const uint32_t* __restrict__ om_s, const uint32_t* __restrict__ om_inv,
                                                  const uint32_t* __restrict__ cos_inv, const uint32_t* __restrict__ kc,
                                                  size_t big_m, size_t small_m, int ti_n, int tj_n) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[256 * FPS_WORDS];
  const int ti = threadIdx.x % ti_n, tj = threadIdx.x / ti_n;
  const size_t i = (size_t)blockIdx.x * ti_n + ti;
  const size_t compr = big_m / small_m;
  Fp<M> acc, u0h;
  fp_zero(acc);
  fp_zero(u0h);
#pragma unroll 1
  for (size_t j = tj; j < compr; j += tj_n) {
    const size_t k = i + j * small_m;
    Fp<M> x;
    load_wire_fp(x, w + k * 24);
    if (j == 0) {
      u0h = x;
      mul_table(u0h, kc);
    } else {
      Fp<M> t = x, s;
      mul_table(t, om_s + k * FPS_WORDS);
      fp_add(s, acc, t);
      acc = s;
      mul_table(x, kc + 2 * FPS_WORDS);
      if constexpr (COSET) mul_table(x, cos_inv + k * FPS_WORDS);
      store_wire_fp(a + k * 24, x);
    }
  }
  lds_store_fp(lds + threadIdx.x * FPS_WORDS, acc);
  __syncthreads();
  if (tj == 0) {        // this thread took j = 0: u0h is set
#pragma unroll 1
    for (int q = 1; q < tj_n; ++q) {
      Fp<M> t, s;
      lds_load_fp(t, lds + (q * ti_n + ti) * FPS_WORDS);
      fp_add(s, acc, t);
      acc = s;
    }
    Fp<M> y, u1h, lo, hi;
    load_wire_fp(y, w + (big_m + i) * 24);
    mul_table(y, kc + 1 * FPS_WORDS);
    fp_sub(u1h, y, acc);
    mul_table(u1h, om_inv + i * FPS_WORDS);
    fp_add(lo, u0h, u1h);
    fp_sub(hi, u0h, u1h);
    if constexpr (COSET) {
      mul_table(lo, cos_inv + i * FPS_WORDS);
      mul_table(hi, cos_inv + (big_m + i) * FPS_WORDS);
    }
    store_wire_fp(a + i * 24, lo);
    store_wire_fp(a + (big_m + i) * 24, hi);
  }
}

// Extended, forward:  out[i] = a[i] + a[s + i];  out[s + i] = shift^i (a[i] + shift^s a[s + i]),  s = small_m.   kc = {shift^s}
template <int M, bool COSET>
__global__ void __launch_bounds__(256) k_ext_pre(const uint32_t* __restrict__ a, uint32_t* __restrict__ out,
                                                const uint32_t* __restrict__ sh, const uint32_t* __restrict__ cos,
                                                const uint32_t* __restrict__ kc, size_t small_m) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= small_m) return;
  Fp<M> x, y, s, t;
  load_wire_fp(x, a + i * 24);
  load_wire_fp(y, a + (small_m + i) * 24);
  if constexpr (COSET) {
    mul_table(x, cos + i * FPS_WORDS);
    mul_table(y, cos + (small_m + i) * FPS_WORDS);
  }
  fp_add(s, x, y);
  store_wire_fp(out + i * 24, s);
  mul_table(y, kc);
  fp_add(t, x, y);
  mul_table(t, sh + i * FPS_WORDS);
  store_wire_fp(out + (small_m + i) * 24, t);
}

// Extended, inverse, behind the two inverse transforms (w0 = w[0, s), w1 = w[s, 2s)):
//   a[i] = sconst (shift^-i w1[i] - shift^s w0[i]);  a[s + i] = sconst (w0[i] - shift^-i w1[i])
// sh_inv_s[i] = sconst shift^-i;  kc = {shift^s, sconst},  sconst = 1 / (s (1 - shift^s))
template <int M, bool COSET>
__global__ void __launch_bounds__(256) k_ext_post(const uint32_t* __restrict__ w, uint32_t* __restrict__ a,
                                                 const uint32_t* __restrict__ sh_inv_s, const uint32_t* __restrict__ cos_inv,
                                                 const uint32_t* __restrict__ kc, size_t small_m) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= small_m) return;
  Fp<M> u, t, lo, hi;
  load_wire_fp(u, w + i * 24);
  load_wire_fp(t, w + (small_m + i) * 24);
  mul_table(u, kc + 1 * FPS_WORDS);
  mul_table(t, sh_inv_s + i * FPS_WORDS);
  fp_sub(hi, u, t);
  mul_table(u, kc);
  fp_sub(lo, t, u);
  if constexpr (COSET) {
    mul_table(lo, cos_inv + i * FPS_WORDS);
    mul_table(hi, cos_inv + (small_m + i) * FPS_WORDS);
  }
  store_wire_fp(a + i * 24, lo);
  store_wire_fp(a + (small_m + i) * 24, hi);
}

// 1 / Z on the coset takes few distinct values on these domains: entry (i & mask) of `zt` for i < split, entry mask + 1 behind it.
//   step:      split = big_m, mask = compr - 1 (omega^(2 small_m) has order compr = big_m / small_m);   extended: split = small_m, mask = 0
__device__ __forceinline__ size_t z_index(size_t i, size_t split, size_t mask) { return i < split ? (i & mask) : mask + 1; }

// a[i] = a[i] / Z(g x_i)       (divide_by_Z_on_coset; zt in device form)
template <int M>
__global__ void __launch_bounds__(256) k_vec_mul_ztab(uint32_t* __restrict__ a, const uint32_t* __restrict__ zt, size_t split, size_t mask, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fp<M> x;
  load_wire_fp(x, a + i * 24);
  mul_table(x, zt + z_index(i, split, mask) * FPS_WORDS);
  store_wire_fp(a + i * 24, x);
}

// k_h_pointwise with 1 / Z from the table:  k2t[.] = Z^-1 * R' * 2^-12
template <int M>
__global__ void __launch_bounds__(256) k_h_pointwise_ztab(uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                         const uint32_t* __restrict__ cvec, const uint32_t* __restrict__ k1,
                                                         const uint32_t* __restrict__ k2t, size_t split, size_t mask, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fp<M> x, y, z, ab, d;
  load_wire_fp(x, a + i * 24);
  load_wire_fp(y, b + i * 24);
  load_wire_fp(z, cvec + i * 24);
  fp_mul(ab, x, y);
  mul_table(z, k1);
  fp_sub(d, ab, z);
  mul_table(d, k2t + z_index(i, split, mask) * FPS_WORDS);
  store_wire_fp(a + i * 24, d);
}

// ---- mixed-radix domains m = Q T, Q = 5^b, T = 2^a (MNT6753: libfqfft basic_radix2_domain over the small subgroup of Fr,
// basic_radix2_domain_aux.tcc:46-165 _basic_serial_mixed_radix_FFT) ------------------------------------------------------------------
// Decimation in time over the radix-5 digits of the index:  x[i1 + Q i2]  ->  Q radix-2 transforms of size T over i2 (k_ntt_group,
// unchanged, root omega^Q)  ->  b radix-5 levels that merge five neighbouring sub-transforms of width W = T (and 5T for Q = 25) each:
//   X[base + W k1 + j] = sum_{l < 5} zeta^(k1 l) omega_W^(l j) Y[base + W l + j],   omega_W = omega^(m / 5W),  zeta = omega^(m / 5)
// k_mixed_pre puts sub-vector i1 at slot s(i1) (i1 itself for Q = 5, its two base-5 digits swapped for Q = 25: the order the two
// levels need), out of place; a level is in place: each butterfly reads and writes the same five positions.

constexpr int R5_COLS = 64;                   // butterflies (columns) per block: one wave per row of the butterfly
constexpr int R5_BLOCK = 5 * R5_COLS;

// out[slot(i % Q) T + i / Q] = a[i] (* g^i: cosetFFT).  One lane per source element: reads and the coset table are coalesced.
template <int M, bool COSET>
__global__ void __launch_bounds__(256) k_mixed_pre(const uint32_t* __restrict__ a, uint32_t* __restrict__ out,
                                                  const uint32_t* __restrict__ cos, size_t m, unsigned q_n, size_t t_n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const unsigned i1 = (unsigned)(i % q_n);
  const size_t i2 = i / q_n;
  const unsigned slot = q_n == 25 ? (i1 % 5) * 5 + i1 / 5 : i1;
  uint32_t* dst = out + ((size_t)slot * t_n + i2) * 24;
  if constexpr (COSET) {
    Fp<M> x;
    load_wire_fp(x, a + i * 24);
    mul_table(x, cos + i * FPS_WORDS);
    store_wire_fp(dst, x);
  } else {
    uint32_t w[24];
    load_wire24(w, a + i * 24);
    store_wire24(dst, w);
  }
}

// One radix-5 level of width W, in place on `v` (m elements, wire form).  Five lanes per butterfly: wave l of a block holds row l of
// 64 consecutive columns c = group * W + j (columns run on across the groups of 5W elements, so a width that is no multiple of 64 --
// T = 1, 2, 8, 5T = 5, 10, 40 -- needs nothing special; a row's loads are coalesced wherever W >= 64).
//   tw:  omega^k, k < m, device form (omega^-k for the inverse);  the lane's twiddle is entry l j tw_stride, tw_stride = m / 5W
//   zc:  zeta^e, e < 5, device form (inverse, last level: zeta^-e / m -- the iFFT's scale rides on the constants; SCALED)
//   out_scale (OUT_SCALE): table indexed by the output position, icosetFFT's g^-k on the last level
// Ranges: a wire element is below p, the table entries below 2p; fp_mul and fp_add keep [0, 2p).
template <int M, bool SCALED, bool OUT_SCALE>
__global__ void __launch_bounds__(R5_BLOCK) k_radix5_merge(uint32_t* v, const uint32_t* __restrict__ tw, const uint32_t* __restrict__ zc,
                                                          const uint32_t* __restrict__ out_scale, size_t n_cols, size_t width,
                                                          size_t tw_stride) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[R5_BLOCK * FPS_WORDS];
  const int row = threadIdx.x / R5_COLS, cc = threadIdx.x % R5_COLS;      // row is wave-uniform
  const size_t c = (size_t)blockIdx.x * R5_COLS + cc;
  const bool active = c < n_cols;
  const size_t grp = c / width, j = c % width;
  const size_t pos = grp * 5 * width + (size_t)row * width + j;           // < m wherever active
  if (active) {
    Fp<M> x;
    load_wire_fp(x, v + pos * 24);
    if (row != 0) mul_table(x, tw + (size_t)row * j * tw_stride * FPS_WORDS);
    lds_store_fp(lds + (row * R5_COLS + cc) * FPS_WORDS, x);
  }
  __syncthreads();
  if (!active) return;
  Fp<M> acc, t, s;
  lds_load_fp(acc, lds + cc * FPS_WORDS);
  if constexpr (SCALED) mul_table(acc, zc);
#pragma unroll 1
  for (int l = 1; l < 5; ++l) {
    const int e = (row * l) % 5;
    lds_load_fp(t, lds + (l * R5_COLS + cc) * FPS_WORDS);
    if (SCALED || e != 0) mul_table(t, zc + e * FPS_WORDS);
    fp_add(s, acc, t);
    acc = s;
  }
  if constexpr (OUT_SCALE) mul_table(acc, out_scale + pos * FPS_WORDS);
  store_wire_fp(v + pos * 24, acc);
}

static __global__ void __launch_bounds__(256) k_copy_h(uint32_t* __restrict__ h, const uint32_t* __restrict__ a, size_t m) {
  // h[0..m) = a[0..m), h[m] = 0      (vector_Fr_zeros(m+1) + vector_Fr_copy_into, cuda_prover_piecewise.cu:50-51)
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per 16-byte quad
  size_t quads = m * 6;
  if (i < quads) reinterpret_cast<uint4*>(h)[i] = reinterpret_cast<const uint4*>(a)[i];
  else if (i < quads + 6) reinterpret_cast<uint4*>(h)[i] = make_uint4(0, 0, 0, 0);
}

}  // namespace mnt753
