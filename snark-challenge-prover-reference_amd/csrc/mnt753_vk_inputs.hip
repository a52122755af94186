// C ABI of the input tables of a verification key: mnt753_vk_prepare_inputs, mnt753_vk_input_plan, mnt753_vk_release_inputs
// (include/mnt753_hip.h), and the launches of the prepared path for the verifiers (vk_inputs_api.hpp).
// Kernels: vk_input_kernels.hip.h, and batch_exp's level and normalisation kernels over the long table.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include "common_host.hpp"
#include "vk_input_kernels.hip.h"
#include "vk_inputs_api.hpp"

namespace mnt753 {
namespace {

constexpr size_t VKI_BUILD_TILE = (size_t)1 << 17;   // rows per level launch of the builder (FB_DEFAULT_TILE)

struct BuildTmp {
  uint32_t *table = nullptr, *acc = nullptr, *pre = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~BuildTmp() {
    for (void* p : {(void*)table, (void*)acc, (void*)pre})
      if (p) (void)hipFree(p);
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// the tables of all points of the key into `table` (zeroed): the window bases by one lane per point, then w - 1 levels over all
// windows of all points at once, in tiles -- O(w) launches per tile of a level, whatever the number of inputs
template <class C1>
int build_tables(const mnt753_vk* vk, uint32_t* table, uint32_t* acc, uint32_t* pre, size_t tile, int w, int W) {
  using V = PointCfg<C1>;
  using F = typename V::F;
  const uint32_t points = (uint32_t)vk->num_inputs + 1u;
  hipLaunchKernelGGL((k_vk_window_bases<C1>), dim3((points + 255u) / 256u), dim3(256), 0, 0, reinterpret_cast<const uint32_t*>(vk->dev_abc), table, points, w, W);
  HIP_TRY(hipGetLastError());
  for (int l = 1; l < w; ++l) {
    FbTargets tg;
    tg.cnt = l < w - 1 ? 1u << l : 1u;
    tg.m0 = 1u << l;
    tg.w = w;
    const uint64_t total = (uint64_t)points * (uint64_t)W * tg.cnt;
    for (uint64_t first = 0; first < total; first += tile) {
      const uint32_t count = (uint32_t)std::min<uint64_t>(tile, total - first);
      tg.first = first;
      hipLaunchKernelGGL((k_fb_level<V>), dim3(blocks_for<F>(count)), dim3(256), 0, 0, table, acc, tg, count);
      hipLaunchKernelGGL((k_fb_normalise<V, true>), dim3(blocks_for<F>((count + FB_INV_BATCH - 1) / FB_INV_BATCH)), dim3(256), 0, 0, acc, pre, table, tg, count,
                         FB_INV_BATCH);
    }
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

template <class C1>
int enqueue_t(const mnt753_vk* vk, const uint32_t* ints, uint32_t n, uint32_t scalars, uint32_t base0, const uint32_t* first_wire, uint32_t ipl,
              const VkInputWs& ws, uint32_t* out_wire, hipStream_t st) {
  using V = PointCfg<C1>;
  using F = typename V::F;
  const uint32_t slices = vki_slices(scalars, ipl);
  const uint64_t lanes = (uint64_t)n * slices;
  hipEvent_t* ev = reinterpret_cast<hipEvent_t*>(const_cast<void**>(vk->in_ev));
  HIP_TRY(hipEventRecord(ev[0], st));
  hipLaunchKernelGGL((k_vk_walk<C1>), dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, vk->dev_in_table, ints, ws.partials, n, scalars, ipl, slices, base0,
                     vk->in_w, vk->in_W);
  HIP_TRY(hipEventRecord(ev[1], st));
  hipLaunchKernelGGL((k_vk_segment_sum<C1>), dim3((n + 255u) / 256u), dim3(256), 0, st, first_wire, ws.partials, ws.sums, n, slices);
  const FbTargets tg{0, 1u, 0u, vk->in_w};
  hipLaunchKernelGGL((k_fb_normalise<V, false>), dim3(blocks_for<F>((n + FB_INV_BATCH - 1) / FB_INV_BATCH)), dim3(256), 0, st, ws.sums, ws.pre, out_wire, tg, n,
                     FB_INV_BATCH);
  HIP_TRY(hipEventRecord(ev[2], st));
  vk->in_timed = true;
  HIP_TRY(hipGetLastError());
  return 0;
}

void drop_tables(mnt753_vk* vk) {
  if (vk->dev_in_table) (void)hipFree(vk->dev_in_table);
  for (auto& e : vk->in_ev) {
    if (e) (void)hipEventDestroy((hipEvent_t)e);
    e = nullptr;
  }
  vk->dev_in_table = nullptr;
  vk->in_w = vk->in_W = 0;
  vk->in_table_bytes = 0;
  vk->in_build_ms = 0.f;
  vk->in_timed = false;
}

}  // namespace

uint32_t vk_inputs_per_lane(const mnt753_vk* vk, size_t n, uint32_t scalars) {
  uint32_t ipl = vk->test_inputs_per_lane ? vk->test_inputs_per_lane : vki_inputs_per_lane(n, scalars);
  if (ipl > scalars && scalars) ipl = scalars;
  while ((uint64_t)n * vki_slices(scalars, ipl) > ((uint64_t)1 << 31)) ipl *= 2;
  return ipl;
}

int vk_inputs_enqueue(const mnt753_vk* vk, const uint32_t* ints, size_t n, uint32_t scalars, uint32_t base0, const uint32_t* first_wire, uint32_t ipl,
                      const VkInputWs& ws, uint32_t* out_wire, hipStream_t st) {
  if (!vk_inputs_prepared(vk) || !n || !scalars || !ipl || (uint64_t)base0 + scalars > vk->num_inputs + 1) return set_error(MNT753_EINVAL, "vk inputs: bad argument");
  if (vk->curve == MNT753_CURVE_MNT4753) return enqueue_t<Mnt4G1>(vk, ints, (uint32_t)n, scalars, base0, first_wire, ipl, ws, out_wire, st);
  return enqueue_t<Mnt6G1>(vk, ints, (uint32_t)n, scalars, base0, first_wire, ipl, ws, out_wire, st);
}

int vk_inputs_dots_enqueue(int curve, const uint32_t* rho, const uint32_t* x, size_t n, uint32_t k, uint32_t* acc, int carry, hipStream_t st) {
  if (curve == MNT753_CURVE_MNT4753) hipLaunchKernelGGL((k_vk_input_dots<MOD_A>), dim3(k), dim3(RED_BLOCK), 0, st, rho, x, (uint32_t)n, k, acc, carry);
  else hipLaunchKernelGGL((k_vk_input_dots<MOD_B>), dim3(k), dim3(RED_BLOCK), 0, st, rho, x, (uint32_t)n, k, acc, carry);
  HIP_TRY(hipGetLastError());
  return 0;
}

int vk_inputs_fold_scalars_enqueue(int curve, const uint32_t* acc, uint32_t k, uint32_t* ints, hipStream_t st) {
  if (curve == MNT753_CURVE_MNT4753) hipLaunchKernelGGL((k_vk_fold_scalars<MOD_A>), dim3((k + 255u) / 256u), dim3(256), 0, st, acc, k, ints);
  else hipLaunchKernelGGL((k_vk_fold_scalars<MOD_B>), dim3((k + 255u) / 256u), dim3(256), 0, st, acc, k, ints);
  HIP_TRY(hipGetLastError());
  return 0;
}

int vk_inputs_last_timing(const mnt753_vk* vk, float* walk_ms, float* sum_ms, float* build_ms) {
  if (!vk) return set_error(MNT753_EINVAL, "vk inputs: bad argument");
  if (walk_ms) *walk_ms = 0.f;
  if (sum_ms) *sum_ms = 0.f;
  if (build_ms) *build_ms = vk->in_build_ms;
  if (!vk_inputs_prepared(vk) || !vk->in_timed) return 0;
  OnDevice guard(vk->device);
  hipEvent_t* ev = reinterpret_cast<hipEvent_t*>(const_cast<void**>(vk->in_ev));
  HIP_TRY(hipEventSynchronize(ev[2]));
  float a = 0.f, b = 0.f;
  HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
  HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
  if (walk_ms) *walk_ms = a;
  if (sum_ms) *sum_ms = b;
  return 0;
}

}  // namespace mnt753

using namespace mnt753;

extern "C" {

int mnt753_vk_prepare_inputs(mnt753_vk* vk, int window_bits, size_t max_table_bytes) {
  if (!vk) return set_error(MNT753_EINVAL, "vk_prepare_inputs: bad argument");
  if (int rc = require_device()) return rc;
  if (vk->num_inputs == 0) return set_error(MNT753_EINVAL, "vk_prepare_inputs: the key has no public inputs");
  if (window_bits != 0 && (window_bits < VKI_MIN_WINDOW_BITS || window_bits > VKI_MAX_WINDOW_BITS))
    return set_error(MNT753_EINVAL, "vk_prepare_inputs: window_bits must be 0 or lie in 2 .. 16");
  const uint64_t cap = max_table_bytes ? (uint64_t)max_table_bytes : VKI_DEFAULT_TABLE_BYTES;
  const uint64_t points = (uint64_t)vk->num_inputs + 1;
  const int w = window_bits ? window_bits : vki_default_window_bits(points, cap);
  const int asked = w ? w : VKI_MIN_WINDOW_BITS;
  if (!w || !vki_table_rows(points, w) || vki_table_bytes(points, w) > cap) {
    char msg[256];
    snprintf(msg, sizeof(msg), "vk_prepare_inputs: the tables of %llu points at width %d need %llu bytes, the cap is %llu bytes%s",
             (unsigned long long)points, asked, (unsigned long long)vki_table_bytes(points, asked), (unsigned long long)cap,
             vki_table_rows(points, asked) ? "" : " (and more than 2^32 rows)");
    return set_error(MNT753_EINVAL, msg);
  }
  const int W = fb_windows(w);
  const size_t bytes = (size_t)vki_table_bytes(points, w);
  // the widest level: every window's multiples 2^(w-2) .. 2^(w-1) - 1
  const uint64_t widest = points * (uint64_t)W * (w > 2 ? (uint64_t)1 << (w - 2) : 1u);
  const size_t tile = (size_t)std::min<uint64_t>(VKI_BUILD_TILE, (widest + FB_INV_BATCH - 1) / FB_INV_BATCH * FB_INV_BATCH);
  OnDevice guard(vk->device);
  BuildTmp tmp;   // the new tables stay the builder's until they are complete: a failure leaves the key as it was
  if (hipMalloc(&tmp.table, bytes) != hipSuccess || hipMalloc(&tmp.acc, (size_t)VKI_PARTIAL_BYTES * tile) != hipSuccess ||
      hipMalloc(&tmp.pre, (size_t)112 * tile) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(MNT753_ENOMEM, "vk_prepare_inputs: the tables do not fit the device memory");
  }
  hipEvent_t walk_ev[3] = {nullptr, nullptr, nullptr};
  auto drop_events = [&]() { for (auto e : walk_ev) if (e) (void)hipEventDestroy(e); };
  for (auto& e : tmp.ev) HIP_TRY(hipEventCreate(&e));
  // rows that are never written (the padding of the 256-byte rows) read as zero
  HIP_TRY(hipMemsetAsync(tmp.table, 0, bytes, 0));
  HIP_TRY(hipEventRecord(tmp.ev[0], 0));
  const int rc = vk->curve == MNT753_CURVE_MNT4753 ? build_tables<Mnt4G1>(vk, tmp.table, tmp.acc, tmp.pre, tile, w, W)
                                                  : build_tables<Mnt6G1>(vk, tmp.table, tmp.acc, tmp.pre, tile, w, W);
  if (rc) { (void)hipDeviceSynchronize(); return rc; }
  HIP_TRY(hipEventRecord(tmp.ev[1], 0));
  HIP_TRY(hipDeviceSynchronize());
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, tmp.ev[0], tmp.ev[1]));
  for (auto& e : walk_ev)
    if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); drop_events(); return set_error(MNT753_EHIP, "vk_prepare_inputs: event creation failed"); }
  drop_tables(vk);
  vk->dev_in_table = tmp.table;
  tmp.table = nullptr;
  for (int k = 0; k < 3; ++k) vk->in_ev[k] = walk_ev[k];
  vk->in_w = w;
  vk->in_W = W;
  vk->in_table_bytes = bytes;
  vk->in_build_ms = ms;
  return 0;
}

int mnt753_vk_input_plan(const mnt753_vk* vk, size_t n, mnt753_vk_input_plan_t* out) {
  if (!vk || !out) return set_error(MNT753_EINVAL, "vk_input_plan: bad argument");
  *out = mnt753_vk_input_plan_t{0, 0, 0u, 0u, 0u, 0, 0};
  if (!vk_inputs_prepared(vk)) return 0;
  out->window_bits = vk->in_w;
  out->windows = vk->in_W;
  out->inputs_per_lane = vk_inputs_per_lane(vk, n ? n : 1, (uint32_t)vk->num_inputs);
  out->table_bytes = vk->in_table_bytes;
  out->prepared = 1;
  return 0;
}

int mnt753_vk_release_inputs(mnt753_vk* vk) {
  if (!vk) return set_error(MNT753_EINVAL, "vk_release_inputs: bad argument");
  OnDevice guard(vk->device);
  drop_tables(vk);
  return 0;
}

}  // extern "C"
