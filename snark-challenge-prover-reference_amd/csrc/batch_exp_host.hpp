// Host orchestration of the fixed-base batch scalar multiplication (mnt753_fixed_base_*, mnt753_batch_exp), templated on the group;
// instantiated once per group in batch_exp_inst_*.hip so that the four sets of kernels compile in parallel, as the MSM's do.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "batch_exp_api.hpp"
#include "batch_exp_kernels.hip.h"
#include "common_host.hpp"
#include "ntt_kernels.hip.h"   // k_vec_scale: the coefficient of batch_exp_with_coeff

namespace mnt753 {

inline int fb_nomem(const char* what) {
  (void)hipGetLastError();
  return set_error(MNT753_ENOMEM, what);
}

template <class C>
int fixed_base_build_t(mnt753_fixed_base* fb, const uint64_t* point, int window_bits, size_t tile) {
  using V = PointCfg<C>;   // the configuration of the point kernels: two / three lanes per point for G2
  using F = typename V::F;
  constexpr size_t ROW_BYTES = sizeof(uint32_t) * row_words<C>();
  constexpr size_t EW = (size_t)C::F::DEG * FPS_WORDS;
  constexpr size_t WIRE_WORDS = 2 * wire_coord_words<C>();
  // the widest table inside the 256 MiB Infinity Cache (counted, the sweep of tools/bench_batch_exp.py decides)
  fb->w = window_bits ? window_bits : fb_default_window_bits((uint32_t)ROW_BYTES, (uint64_t)256 << 20);
  fb->W = fb_windows(fb->w);
  fb->B = FB_INV_BATCH;
  fb->T = (size_t)fb_round_tile(tile);
  const uint32_t H = fb_rows_per_window(fb->w);
  const uint32_t* pw = reinterpret_cast<const uint32_t*>(point);
  uint32_t yor = 0;
  for (size_t k = WIRE_WORDS / 2; k < WIRE_WORDS; ++k) yor |= pw[k];
  fb->identity = yor == 0;

  fb->table_bytes = (size_t)fb_table_rows(fb->w) * ROW_BYTES;
  if (hipMalloc(&fb->d_table, fb->table_bytes) != hipSuccess) return fb_nomem("fixed_base_create: the table does not fit the device memory");
  if (hipMalloc(&fb->d_acc, sizeof(uint32_t) * proj_words<C>() * fb->T) != hipSuccess || hipMalloc(&fb->d_pre, sizeof(uint32_t) * EW * fb->T) != hipSuccess ||
      hipMalloc(&fb->d_scaled, 96 * fb->T) != hipSuccess || hipMalloc(&fb->d_in, 96 * fb->T) != hipSuccess ||
      hipMalloc(&fb->d_out, sizeof(uint32_t) * WIRE_WORDS * fb->T) != hipSuccess)
    return fb_nomem("fixed_base_create: the workspace does not fit the device memory");
  for (auto& e : fb->ev) HIP_TRY(hipEventCreate(&e));
  // rows that are never written (the padding of the 256-byte rows; all of it for an identity base) read as zero
  HIP_TRY(hipMemsetAsync(fb->d_table, 0, fb->table_bytes, 0));
  if (fb->identity) {
    HIP_TRY(hipDeviceSynchronize());
    return 0;
  }

  // the base, then the window bases 2^(jw) P: row 0 of every window -- the MSM's table kernel over ONE point whose "number of
  // points" is the rows of a window, so that its row j lands on row(j, 1)
  uint32_t *d_point = nullptr, *ztmp = nullptr, *ptmp = nullptr;
  uint8_t* d_inf = nullptr;
  struct Tmp {
    uint32_t *&a, *&b, *&c;
    uint8_t*& d;
    ~Tmp() { for (void* q : {(void*)a, (void*)b, (void*)c, (void*)d}) if (q) (void)hipFree(q); }
  } tmp{d_point, ztmp, ptmp, d_inf};
  if (hipMalloc(&d_point, sizeof(uint32_t) * WIRE_WORDS) != hipSuccess || hipMalloc(&d_inf, 16) != hipSuccess ||
      hipMalloc(&ztmp, sizeof(uint32_t) * EW * fb->W) != hipSuccess || hipMalloc(&ptmp, sizeof(uint32_t) * EW * fb->W) != hipSuccess)
    return fb_nomem("fixed_base_create: device allocation failed");
  HIP_TRY(hipMemcpy(d_point, point, sizeof(uint32_t) * WIRE_WORDS, hipMemcpyHostToDevice));
  HIP_TRY(hipEventRecord(fb->ev[0], 0));
  hipLaunchKernelGGL((k_bases_to_internal<C, true>), dim3(1), dim3(256), 0, 0, d_point, fb->d_table, d_inf, (size_t)1);
  hipLaunchKernelGGL((k_precompute_windows<V>), dim3(blocks_for<F>(1)), dim3(256), 0, 0, fb->d_table, d_inf, ztmp, ptmp, (size_t)H, (size_t)0, (size_t)1,
                     fb->w, fb->W);
  HIP_TRY(hipGetLastError());
  // the multiples, level by level: level l holds m = 2^l .. 2^(l+1) - 1 (the last level only m = 2^(w-1)), each from row m >> 1
  for (int l = 1; l < fb->w; ++l) {
    FbTargets tg;
    tg.cnt = l < fb->w - 1 ? 1u << l : 1u;
    tg.m0 = 1u << l;
    tg.w = fb->w;
    const uint64_t total = (uint64_t)fb->W * tg.cnt;
    for (uint64_t first = 0; first < total; first += fb->T) {
      const uint32_t count = (uint32_t)std::min<uint64_t>(fb->T, total - first);
      tg.first = first;
      hipLaunchKernelGGL((k_fb_level<V>), dim3(blocks_for<F>(count)), dim3(256), 0, 0, fb->d_table, fb->d_acc, tg, count);
      hipLaunchKernelGGL((k_fb_normalise<V, true>), dim3(blocks_for<F>((count + fb->B - 1) / fb->B)), dim3(256), 0, 0, fb->d_acc, fb->d_pre, fb->d_table, tg,
                         count, fb->B);
    }
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(fb->ev[1], 0));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipEventElapsedTime(&fb->build_ms, fb->ev[0], fb->ev[1]));
  return 0;
}

template <class C>
int batch_exp_t(mnt753_fixed_base* fb, const uint64_t* scalars, int scalars_on_device, size_t n, const uint64_t* host_coeff, uint64_t* out_affine,
                int out_on_device, hipStream_t st) {
  using V = PointCfg<C>;
  using F = typename V::F;
  constexpr size_t WIRE_WORDS = 2 * wire_coord_words<C>();
  WireElem k;
  if (host_coeff) memcpy(k.w, host_coeff, 96);
  const uint32_t* sw = reinterpret_cast<const uint32_t*>(scalars);
  uint32_t* ow = reinterpret_cast<uint32_t*>(out_affine);
  for (size_t off = 0; off < n; off += fb->T) {
    const uint32_t cnt = (uint32_t)std::min(fb->T, n - off);
    const uint32_t* src = sw + off * 24;
    if (!scalars_on_device) {
      HIP_TRY(hipMemcpyAsync(fb->d_in, src, 96 * (size_t)cnt, hipMemcpyHostToDevice, st));
      src = fb->d_in;
    }
    if (host_coeff) {   // batch_exp_with_coeff (multiexp.tcc:641-668): coeff * v[i] in Fr, into the object's copy -- the caller's scalars are only read
      hipLaunchKernelGGL((k_vec_scale<C::FR>), dim3((cnt + 255) / 256), dim3(256), 0, st, fb->d_scaled, src, k, (size_t)cnt);
      src = fb->d_scaled;
    }
    FbTargets tg{out_on_device ? (uint64_t)off : 0, 1u, 0u, fb->w};
    uint32_t* dst = out_on_device ? ow : fb->d_out;
    if (fb->identity) {
      HIP_TRY(hipMemsetAsync(dst + tg.first * WIRE_WORDS, 0, sizeof(uint32_t) * WIRE_WORDS * cnt, st));
    } else {
      const bool last = off + cnt == n;
      if (last) HIP_TRY(hipEventRecord(fb->ev[0], st));
      hipLaunchKernelGGL((k_fb_walk<V>), dim3(blocks_for<F>(cnt)), dim3(256), 0, st, fb->d_table, src, fb->d_acc, cnt, fb->w, fb->W);
      if (last) HIP_TRY(hipEventRecord(fb->ev[1], st));
      hipLaunchKernelGGL((k_fb_normalise<V, false>), dim3(blocks_for<F>((cnt + fb->B - 1) / fb->B)), dim3(256), 0, st, fb->d_acc, fb->d_pre, dst, tg, cnt,
                         fb->B);
      if (last) { HIP_TRY(hipEventRecord(fb->ev[2], st)); fb->timed = true; }
      HIP_TRY(hipGetLastError());
    }
    if (!out_on_device) HIP_TRY(hipMemcpyAsync(ow + off * WIRE_WORDS, fb->d_out, sizeof(uint32_t) * WIRE_WORDS * cnt, hipMemcpyDeviceToHost, st));
  }
  // an end in host memory: the call returns when that end is done (the convention of the entry points that take host data)
  if (!scalars_on_device || !out_on_device) HIP_TRY(hipStreamSynchronize(st));
  return 0;
}


}  // namespace mnt753
