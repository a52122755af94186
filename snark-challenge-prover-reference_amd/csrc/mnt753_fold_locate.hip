// C ABI of the folded Groth16 verification with one tail per segment: mnt753_fold_segment_proofs, mnt753_groth16_verify_folded_locate
// (include/mnt753_hip.h).  Kernels: fold_kernels.hip.h (the scaling and the Miller loops, unchanged) and
// fold_locate_kernels.hip.h; the plan of segments, chunks and rechecked runs: fold_locate_plan.hpp.  The recheck is the per-proof
// verifier's chunked path as it stands, entered through mnt753_groth16_verify_ex (which is that path and nothing else).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>
#include "common_host.hpp"
#include "fold_locate_api.hpp"
#include "fold_locate_kernels.hip.h"
#include "fold_locate_plan.hpp"
#include "host_field.hpp"
#include "vk_inputs_api.hpp"
#include "vk_object.hpp"

namespace mnt753 {
namespace {

constexpr size_t LOCATE_CHUNK = (size_t)1 << 16;    // proofs per launch at most, as for mnt753_groth16_verify_folded
constexpr size_t LOCATE_MAX = (size_t)1 << 24;

// device memory of one call
struct LocateBuffers {
  void *proofs = nullptr, *inputs = nullptr, *coef = nullptr, *rhom = nullptr, *ints = nullptr, *u = nullptr, *c = nullptr, *flags = nullptr,
       *partials = nullptr, *seg = nullptr, *sints = nullptr, *fwire = nullptr, *wpart = nullptr, *wsums = nullptr, *wpre = nullptr;
  ~LocateBuffers() {
    for (void* p : {proofs, inputs, coef, rhom, ints, u, c, flags, partials, seg, sints, fwire, wpart, wsums, wpre})
      if (p) (void)hipFree(p);
  }
};
// the rejected segments of a device batch side by side, for one call of the per-proof verifier
struct GatheredBatch {
  void *proofs = nullptr, *inputs = nullptr;
  ~GatheredBatch() {
    for (void* p : {proofs, inputs})
      if (p) (void)hipFree(p);
  }
};
int locate_alloc(void** p, size_t bytes) {
  if (hipMalloc(p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return set_error(MNT753_ENOMEM, "groth16_verify_folded_locate: device allocation failed");
  }
  return 0;
}
// HIP events around the stages of a chunk: scale (with the point sums), Miller, tails (with the scalars and S_s)
struct LocateEvents {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ok = true;
  LocateEvents() { for (auto& v : e) if (hipEventCreate(&v) != hipSuccess) { (void)hipGetLastError(); v = nullptr; ok = false; } }
  ~LocateEvents() { for (auto v : e) if (v) (void)hipEventDestroy(v); }
  void mark(int k, hipStream_t st) { if (ok) (void)hipEventRecord(e[k], st); }
  void add(float& to, int a, int b) {   // after the stream has been synchronised
    float ms = 0.f;
    if (ok && hipEventElapsedTime(&ms, e[a], e[b]) == hipSuccess) to += ms; else (void)hipGetLastError();
  }
};
thread_local size_t t_locate_chunks = 0;   // chunks of the calling thread's last call, for the test library
bool locate_on_device_of(const void* p, int device) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.device == device;
}

// C: the lane-split G2 configuration, C1: G1, FR: the modulus id of the scalar field
template <class C, class C1, int FR>
int locate_t(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int on_device, const uint64_t* coef, uint8_t* verdicts,
             mnt753_fold_locate_report* report, hipStream_t st, const FoldLocateParts* parts) {
  using F = typename C::F;
  using G = FoldGroups<F>;
  typedef host::HFp<FR> Fr;
  const int curve = vk->curve;
  constexpr size_t g = (size_t)G::GROUPS;
  const size_t ni = vk->num_inputs, w2 = mnt753_affine_words(curve, MNT753_G2), pw = 48 + w2, wt = mnt753_gt_words(curve);
  const uint32_t scalars = (uint32_t)ni + 1u;
  constexpr size_t PB = 4 * (size_t)proj_words<C1>(), TB = 4 * (size_t)G::TW;
  // Per proof of a CHUNK as for mnt753_groth16_verify_folded.  Per segment of the CALL, kept from chunk to chunk so that S_s and the
  // tails of all segments run in one launch each: F_s, S_s and T_s, rho_s as exponent and as integer, the verdict, the scalars of S_s,
  // the status bytes of its proofs, and a prepared key's walk of the scalars (include/mnt753_hip.h).  Under a cap the segments' share
  // comes off first and the rest bounds the chunk.
  const bool prepared = vk_inputs_prepared(vk);
  const size_t all_segments = fold_segments(n, g);
  const uint32_t ipl = prepared ? vk_inputs_per_lane(vk, all_segments, scalars) : 0u;
  const size_t per_proof = 192 + PB + 2 + 16 + (ni ? 96 * ni + 96 : 0) + (on_device ? 0 : 8 * pw + 96 * ni);
  const size_t per_segment = TB + 516 + g + 96 * (size_t)scalars + (prepared ? (size_t)vki_workspace_per_proof(scalars, ipl) : 0);
  const size_t fixed = per_segment * all_segments;
  const size_t chunk_cap = !vk->workspace_cap ? 0 : (vk->workspace_cap > fixed ? vk->workspace_cap - fixed : 1);
  const size_t chunk = fold_chunk_proofs(n, g, per_proof, 0, chunk_cap, LOCATE_CHUNK);
  const size_t max_seg = chunk / g;
  LocateBuffers buf;
  if (!on_device) {
    if (int rc = locate_alloc(&buf.proofs, 8 * pw * chunk)) return rc;
    if (ni) { if (int rc = locate_alloc(&buf.inputs, 96 * ni * chunk)) return rc; }
  }
  if (ni) {
    if (int rc = locate_alloc(&buf.ints, 96 * ni * chunk)) return rc;
    if (int rc = locate_alloc(&buf.rhom, 96 * chunk)) return rc;
  }
  if (int rc = locate_alloc(&buf.coef, 16 * chunk)) return rc;
  if (int rc = locate_alloc(&buf.u, 192 * chunk)) return rc;
  if (int rc = locate_alloc(&buf.c, PB * chunk)) return rc;
  if (int rc = locate_alloc(&buf.flags, chunk)) return rc;
  if (int rc = locate_alloc(&buf.partials, TB * all_segments)) return rc;
  // seg: S_s | T_s (wire) | rho_s as exponent | rho_s as integer | the verdict, each an array over the call's segments, then the
  // status bytes of the call's proofs
  const size_t off_t = 192 * all_segments, off_e = off_t + 192 * all_segments, off_r = off_e + sizeof(FoldExp) * all_segments,
               off_acc = off_r + 96 * all_segments, off_st = off_acc + 4 * all_segments;
  if (int rc = locate_alloc(&buf.seg, off_st + n)) return rc;
  if (int rc = locate_alloc(&buf.sints, 96 * (size_t)scalars * all_segments)) return rc;
  if (parts && parts->f) { if (int rc = locate_alloc(&buf.fwire, 8 * wt * all_segments)) return rc; }
  VkInputWs ws;
  if (prepared) {
    if (int rc = locate_alloc(&buf.wpart, vk_inputs_partials_bytes(all_segments, scalars, ipl))) return rc;
    if (int rc = locate_alloc(&buf.wsums, vk_inputs_sums_bytes(all_segments))) return rc;
    if (int rc = locate_alloc(&buf.wpre, vk_inputs_pre_bytes(all_segments))) return rc;
    ws.partials = reinterpret_cast<uint32_t*>(buf.wpart);
    ws.sums = reinterpret_cast<uint32_t*>(buf.wsums);
    ws.pre = reinterpret_cast<uint32_t*>(buf.wpre);
  }
  char* segb = reinterpret_cast<char*>(buf.seg);
  uint32_t *s_wire = reinterpret_cast<uint32_t*>(segb), *t_wire = reinterpret_cast<uint32_t*>(segb + off_t), *rho_ints = reinterpret_cast<uint32_t*>(segb + off_r),
           *dev_accepted = reinterpret_cast<uint32_t*>(segb + off_acc), *sints = reinterpret_cast<uint32_t*>(buf.sints),
           *partials = reinterpret_cast<uint32_t*>(buf.partials);
  FoldExp* rho_exp = reinterpret_cast<FoldExp*>(segb + off_e);
  uint8_t* dev_bad = reinterpret_cast<uint8_t*>(buf.flags);
  uint8_t* dev_status = reinterpret_cast<uint8_t*>(segb + off_st);
  const uint32_t* key = reinterpret_cast<const uint32_t*>(vk->dev_key);

  Fr r2;
  memcpy(r2.l, FPC[FR].r2_64, sizeof(r2.l));
  std::vector<uint64_t> rhom;                        // rho_i of a chunk as elements of Fr, wire (Montgomery) form
  std::vector<FoldExp> exps(all_segments);           // rho_s: the exponent of e(alpha, beta)
  std::vector<uint64_t> rints(12 * all_segments, 0); // and the integer that scales ABC[0]
  std::vector<uint32_t> acc32(all_segments);
  std::vector<uint8_t> accepted(all_segments, 0);
  mnt753_fold_locate_report rep;
  memset(&rep, 0, sizeof(rep));
  rep.segments = all_segments;
  memset(verdicts, 0, n);
  // rho_s = the sum of the segment's coefficients: below 2^128 g < 2^136
  int max_bits = 1;
  for (size_t s = 0; s < all_segments; ++s) {
    const FoldRange r = fold_segment_range(s, n, g);
    uint64_t sum[3] = {0, 0, 0};
    for (size_t k = r.first; k < r.first + r.count; ++k) {
      unsigned __int128 carry = 0;
      for (int w = 0; w < 3; ++w) {
        carry += (unsigned __int128)sum[w] + (w < 2 ? coef[2 * k + w] : 0);
        sum[w] = (uint64_t)carry;
        carry >>= 64;
      }
    }
    memcpy(&rints[12 * s], sum, sizeof(sum));
    for (int w = 0; w < 8; ++w) {
      exps[s].w[w] = w < 6 ? (uint32_t)(sum[w >> 1] >> (32 * (w & 1))) : 0u;
      if (exps[s].w[w]) {
        const int bits = 32 * w + 32 - __builtin_clz(exps[s].w[w]);
        if (bits > max_bits) max_bits = bits;
      }
    }
    if (parts && parts->rho) {
      Fr v = Fr::from_words(&rints[12 * s]) * r2;
      memcpy(parts->rho + 12 * s, v.l, 96);
    }
  }
  HIP_TRY(hipMemcpyAsync(rho_exp, exps.data(), sizeof(FoldExp) * all_segments, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(rho_ints, rints.data(), 96 * all_segments, hipMemcpyHostToDevice, st));
  LocateEvents ev;
  const dim3 b(256);
  size_t seg0 = 0, chunks = 0;
  for (size_t first = 0; first < n; first += chunk, seg0 += max_seg, ++chunks) {
    const size_t cnt = n - first < chunk ? n - first : chunk;
    const size_t segs = fold_segments(cnt, g);
    const uint64_t* dp = proofs + first * pw;
    const uint64_t* di = ni ? inputs + first * ni * 12 : nullptr;
    const uint64_t* ck = coef + 2 * first;
    if (!on_device) {
      HIP_TRY(hipMemcpyAsync(buf.proofs, dp, 8 * pw * cnt, hipMemcpyHostToDevice, st));
      dp = reinterpret_cast<const uint64_t*>(buf.proofs);
      if (ni) {
        HIP_TRY(hipMemcpyAsync(buf.inputs, di, 96 * ni * cnt, hipMemcpyHostToDevice, st));
        di = reinterpret_cast<const uint64_t*>(buf.inputs);
      }
    }
    HIP_TRY(hipMemcpyAsync(buf.coef, ck, 16 * cnt, hipMemcpyHostToDevice, st));
    const dim3 g1((unsigned)((cnt + 255) / 256));
    const uint32_t* p32 = reinterpret_cast<const uint32_t*>(dp);
    if (ni) {
      rhom.assign(12 * cnt, 0);
      for (size_t k = 0; k < cnt; ++k) {
        Fr v = Fr::zero();
        v.l[0] = ck[2 * k]; v.l[1] = ck[2 * k + 1];
        v = v * r2;
        memcpy(&rhom[12 * k], v.l, 96);
      }
      HIP_TRY(hipMemcpyAsync(buf.rhom, rhom.data(), 96 * cnt, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL((k_inputs_to_integer<FR>), g1, b, 0, st, reinterpret_cast<const uint32_t*>(di), reinterpret_cast<uint32_t*>(buf.ints), dev_bad,
                         (uint32_t)cnt, (uint32_t)ni);
    } else {
      HIP_TRY(hipMemsetAsync(dev_bad, 0, cnt, st));
    }
    // scale: U_i and rho_i C_i; then T_s per segment
    ev.mark(0, st);
    hipLaunchKernelGGL((k_fold_scale<C1>), g1, b, 0, st, p32, (uint32_t)(2 * pw), reinterpret_cast<const uint32_t*>(buf.coef), key, dev_bad,
                       reinterpret_cast<uint32_t*>(buf.u), reinterpret_cast<uint32_t*>(buf.c), (uint32_t)cnt);
    hipLaunchKernelGGL((k_fold_segment_point_sum<C1>), dim3((unsigned)segs), b, 0, st, reinterpret_cast<uint32_t*>(buf.c), (uint32_t)cnt, (uint32_t)g,
                       t_wire + 48 * seg0);
    // Miller: partials[seg0 + s] = F_s (a chunk starts on a segment boundary, and a workgroup of k_fold_miller is one segment)
    ev.mark(1, st);
    hipLaunchKernelGGL((k_fold_miller<C, C1>), dim3((unsigned)segs), b, 0, st, p32, reinterpret_cast<const uint32_t*>(buf.u), key, dev_bad, dev_status + first,
                       partials + (size_t)G::TW * seg0, (uint32_t)cnt);
    ev.mark(2, st);
    HIP_TRY(hipGetLastError());
    // the scalars of S_s: they read the chunk's inputs and coefficients
    const uint32_t dot_lanes = (uint32_t)segs * scalars;
    hipLaunchKernelGGL((k_fold_segment_dots<FR>), dim3((dot_lanes + 255u) / 256u), b, 0, st, reinterpret_cast<const uint32_t*>(buf.rhom),
                       reinterpret_cast<const uint32_t*>(di), (const uint32_t*)(rho_ints + 24 * seg0), (uint32_t)cnt, (uint32_t)ni, (uint32_t)g, (uint32_t)segs,
                       sints + (size_t)24 * scalars * seg0);
    ev.mark(3, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));                // the staging buffers and rhom serve the next chunk
    ev.add(rep.ms_scale, 0, 1);
    ev.add(rep.ms_miller, 1, 2);
    ev.add(rep.ms_tails, 2, 3);
  }
  t_locate_chunks = chunks;
  // S_s and the tails of ALL segments of the call, one launch each
  ev.mark(0, st);
  if (prepared) {
    // as `all_segments` proofs of num_inputs + 1 scalars against the tables of ABC[0 ..]: rho_s itself is an integer below r
    if (int rc = vk_inputs_enqueue(vk, sints, all_segments, scalars, 0u, nullptr, ipl, ws, s_wire, st)) return rc;
  } else {
    hipLaunchKernelGGL((k_fold_segment_s<C1>), dim3((unsigned)((all_segments + 255) / 256)), b, 0, st, reinterpret_cast<const uint32_t*>(vk->dev_abc),
                       (const uint32_t*)sints, s_wire, (uint32_t)all_segments, scalars, (uint32_t)(ni ? 753 : max_bits));
  }
  hipLaunchKernelGGL((k_fold_segment_tail<C, C1>), dim3(blocks_for<F>(all_segments)), b, 0, st, (const uint32_t*)partials, (const uint32_t*)s_wire,
                     (const uint32_t*)t_wire, key, (const uint32_t*)vk->dev_coeffs, (const FoldExp*)rho_exp, max_bits, (const uint8_t*)dev_status, (uint32_t)n,
                     (uint32_t)g, (uint32_t)all_segments, dev_accepted);
  ev.mark(1, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(acc32.data(), dev_accepted, 4 * all_segments, hipMemcpyDeviceToHost, st));
  if (parts) {
    if (parts->f) {
      hipLaunchKernelGGL((k_fold_segment_export<C>), dim3(blocks_for<F>(all_segments)), b, 0, st, (const uint32_t*)partials, (uint32_t)all_segments,
                         reinterpret_cast<uint32_t*>(buf.fwire));
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(parts->f, buf.fwire, 8 * wt * all_segments, hipMemcpyDeviceToHost, st));
    }
    if (parts->s) HIP_TRY(hipMemcpyAsync(parts->s, s_wire, 192 * all_segments, hipMemcpyDeviceToHost, st));
    if (parts->t) HIP_TRY(hipMemcpyAsync(parts->t, t_wire, 192 * all_segments, hipMemcpyDeviceToHost, st));
    if (parts->status) HIP_TRY(hipMemcpyAsync(parts->status, dev_status, n, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  ev.add(rep.ms_tails, 0, 1);
  for (size_t s = 0; s < all_segments; ++s) accepted[s] = acc32[s] ? 1 : 0;
  if (parts && parts->accepted) memcpy(parts->accepted, accepted.data(), all_segments);
  // The recheck: the per-proof verifier with the subgroup test on the rejected segments.  One run of adjacent segments is verified where
  // it lies, in the caller's memory.  Several runs are gathered into one batch first and their verdicts scattered: every call of the
  // per-proof verifier is one serial chain deep whatever its size, so a call per run pays that depth once per run.
  const auto t0 = std::chrono::steady_clock::now();
  for (uint8_t a : accepted) rep.segments_rejected += a ? 0 : 1;
  const std::vector<FoldRange> runs = fold_rejected_runs(accepted, n, g);
  size_t total = 0;
  for (const FoldRange& r : runs) total += r.count;
  // (the gathered copy counts against the key's cap: where it does not fit, every run is verified where it lies)
  const bool gather = runs.size() > 1 && (!vk->workspace_cap || total * (8 * pw + 96 * ni) <= vk->workspace_cap);
  if (!gather) {
    for (const FoldRange& r : runs) {
      const int rc = mnt753_groth16_verify_ex(vk, proofs + r.first * pw, ni ? inputs + r.first * ni * 12 : nullptr, r.count, on_device, MNT753_VERIFY_CHECK_SUBGROUP,
                                              verdicts + r.first, st);
      if (rc < 0) return rc;
    }
    rep.proofs_rechecked = total;
  } else {
    GatheredBatch gb;
    std::vector<uint64_t> hp, hi;
    const uint64_t *gp = nullptr, *gi = nullptr;
    if (on_device) {
      if (int rc = locate_alloc(&gb.proofs, 8 * pw * total)) return rc;
      if (ni) { if (int rc = locate_alloc(&gb.inputs, 96 * ni * total)) return rc; }
      gp = reinterpret_cast<const uint64_t*>(gb.proofs);
      gi = reinterpret_cast<const uint64_t*>(gb.inputs);
    } else {
      hp.resize(pw * total);
      hi.resize(12 * ni * total);
      gp = hp.data();
      gi = ni ? hi.data() : nullptr;
    }
    size_t at = 0;
    for (const FoldRange& r : runs) {
      if (on_device) {
        HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(gb.proofs) + 8 * pw * at, proofs + r.first * pw, 8 * pw * r.count, hipMemcpyDeviceToDevice, st));
        if (ni) HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(gb.inputs) + 96 * ni * at, inputs + r.first * ni * 12, 96 * ni * r.count, hipMemcpyDeviceToDevice, st));
      } else {
        memcpy(hp.data() + pw * at, proofs + r.first * pw, 8 * pw * r.count);
        if (ni) memcpy(hi.data() + 12 * ni * at, inputs + r.first * ni * 12, 96 * ni * r.count);
      }
      at += r.count;
    }
    std::vector<uint8_t> gathered(total);
    const int rc = mnt753_groth16_verify_ex(vk, gp, gi, total, on_device, MNT753_VERIFY_CHECK_SUBGROUP, gathered.data(), st);
    if (rc < 0) return rc;
    at = 0;
    for (const FoldRange& r : runs) {
      memcpy(verdicts + r.first, gathered.data() + at, r.count);
      at += r.count;
    }
    rep.proofs_rechecked = total;
  }
  if (rep.proofs_rechecked) rep.ms_recheck = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (report) *report = rep;
  size_t rejected = 0;
  for (size_t k = 0; k < n; ++k) rejected += verdicts[k] != 0;
  return (int)rejected;
}

}  // namespace

int groth16_verify_folded_locate_parts(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int on_device, const uint64_t* coefficients,
                                       uint8_t* verdicts, mnt753_fold_locate_report* report, void* stream, const FoldLocateParts* parts) {
  if (!vk || (n && (!proofs || !coefficients || !verdicts || (vk->num_inputs && !inputs))) || n > LOCATE_MAX)
    return set_error(MNT753_EINVAL, "groth16_verify_folded_locate: bad argument");
  for (size_t k = 0; k < n; ++k)
    if (!(coefficients[2 * k] | coefficients[2 * k + 1])) return set_error(MNT753_EINVAL, "groth16_verify_folded_locate: a coefficient is zero");
  if (int rc = require_device()) return rc;
  if (report) memset(report, 0, sizeof(*report));
  if (!n) return 0;
  OnDevice guard(vk->device);
  if (on_device && (!locate_on_device_of(proofs, vk->device) || (vk->num_inputs && !locate_on_device_of(inputs, vk->device))))
    return set_error(MNT753_EINVAL, "groth16_verify_folded_locate: proofs and inputs must lie on the device of the key");
  hipStream_t st = (hipStream_t)stream;
  if (vk->curve == MNT753_CURVE_MNT4753) return locate_t<Mnt4G2S, Mnt4G1, MOD_A>(vk, proofs, inputs, n, on_device, coefficients, verdicts, report, st, parts);
  return locate_t<Mnt6G2S, Mnt6G1, MOD_B>(vk, proofs, inputs, n, on_device, coefficients, verdicts, report, st, parts);
}

size_t groth16_fold_locate_last_chunks() { return t_locate_chunks; }

}  // namespace mnt753

extern "C" size_t mnt753_fold_segment_proofs(int curve) {
  if (curve == MNT753_CURVE_MNT4753) return (size_t)mnt753::FoldGroups<mnt753::Mnt4G2S::F>::GROUPS;
  if (curve == MNT753_CURVE_MNT6753) return (size_t)mnt753::FoldGroups<mnt753::Mnt6G2S::F>::GROUPS;
  return 0;
}

extern "C" int mnt753_groth16_verify_folded_locate(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int on_device,
                                                   const uint64_t* coefficients, uint8_t* verdicts, mnt753_fold_locate_report* report, void* stream) {
  return mnt753::groth16_verify_folded_locate_parts(vk, proofs, inputs, n, on_device, coefficients, verdicts, report, stream, nullptr);
}
