// C ABI of the folded Groth16 verification: mnt753_groth16_verify_folded (include/mnt753_hip.h).
// Kernels: fold_kernels.hip.h.  The key object and its stored coefficients are mnt753_pairing.hip's.
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include "common_host.hpp"
#include "fold_api.hpp"
#include "fold_kernels.hip.h"
#include "host_field.hpp"
#include "vk_inputs_api.hpp"
#include "vk_object.hpp"

namespace mnt753 {
namespace {

constexpr size_t FOLD_CHUNK = (size_t)1 << 16;      // proofs per launch, as for mnt753_groth16_verify
constexpr size_t FOLD_MAX = (size_t)1 << 24;        // logical lanes are 32-bit; rho = sum rho_i stays below 2^152

// device memory of one call
struct FoldBuffers {
  void *proofs = nullptr, *inputs = nullptr, *coef = nullptr, *rhom = nullptr, *ints = nullptr, *u = nullptr, *c = nullptr, *flags = nullptr,
       *partials = nullptr, *small = nullptr;
  // a prepared key: the carried sums c_j, the num_inputs + 1 scalars of S as integers, and the workspace of their walk
  void *cacc = nullptr, *sints = nullptr, *wpart = nullptr, *wsums = nullptr, *wpre = nullptr;
  ~FoldBuffers() {
    for (void* p : {proofs, inputs, coef, rhom, ints, u, c, flags, partials, small, cacc, sints, wpart, wsums, wpre})
      if (p) (void)hipFree(p);
  }
};
int fold_alloc(void** p, size_t bytes) {
  if (hipMalloc(p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return set_error(MNT753_ENOMEM, "groth16_verify_folded: device allocation failed");
  }
  return 0;
}
// HIP events around the stages of a call, and the milliseconds of the last call on this thread: scale (the ladders and the point sum),
// Miller and fold (with the product of the partial products), tail.  For tools/bench_fold.py through the test library.
struct FoldEvents {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ok = true;
  FoldEvents() { for (auto& v : e) if (hipEventCreate(&v) != hipSuccess) { (void)hipGetLastError(); v = nullptr; ok = false; } }
  ~FoldEvents() { for (auto v : e) if (v) (void)hipEventDestroy(v); }
  void mark(int k, hipStream_t st) { if (ok) (void)hipEventRecord(e[k], st); }
  void add(float& to, int a, int b) {   // after the stream has been synchronised
    float ms = 0.f;
    if (ok && hipEventElapsedTime(&ms, e[a], e[b]) == hipSuccess) to += ms; else (void)hipGetLastError();
  }
};
thread_local float t_fold_ms[3] = {0.f, 0.f, 0.f};

bool fold_on_device_of(const void* p, int device) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.device == device;
}

// C: the lane-split G2 configuration, C1: G1, FR: the modulus id of the scalar field
template <class C, class C1, int FR>
int fold_t(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int on_device, const uint64_t* coef, uint8_t* status,
           int* accepted, hipStream_t st, const FoldParts* parts) {
  using F = typename C::F;
  using G = FoldGroups<F>;
  typedef host::HFp<FR> Fr;
  const int curve = vk->curve;
  const size_t ni = vk->num_inputs, w2 = mnt753_affine_words(curve, MNT753_G2), pw = 48 + w2, wt = mnt753_gt_words(curve);
  constexpr size_t PB = 4 * (size_t)proj_words<C1>(), TB = 4 * (size_t)G::TW;   // bytes of a projective G1 point / a tower element, storage form
  // what one proof of a chunk takes: rho_i A_i, rho_i C_i, flag and status, its coefficient; with inputs their integers
  // (k_inputs_to_integer; the room then serves the gathered columns) and rho_i as an element of Fr; its staged copy if it arrives in
  // host memory.  One tower element per workgroup of the Miller kernel comes on top.
  const size_t per_proof = 192 + PB + 2 + 16 + (ni ? 96 * ni + 96 : 0) + (on_device ? 0 : 8 * pw + 96 * ni);
  size_t chunk = n < FOLD_CHUNK ? n : FOLD_CHUNK;
  if (vk->workspace_cap && vk->workspace_cap / per_proof < chunk) chunk = vk->workspace_cap / per_proof ? vk->workspace_cap / per_proof : 1;
  const size_t max_wg = (chunk + G::GROUPS - 1) / G::GROUPS;
  FoldBuffers buf;
  if (!on_device) {
    if (int rc = fold_alloc(&buf.proofs, 8 * pw * chunk)) return rc;
    if (ni) { if (int rc = fold_alloc(&buf.inputs, 96 * ni * chunk)) return rc; }
  }
  if (ni) {
    if (int rc = fold_alloc(&buf.ints, 96 * ni * chunk)) return rc;
    if (int rc = fold_alloc(&buf.rhom, 96 * chunk)) return rc;
  }
  if (int rc = fold_alloc(&buf.coef, 16 * chunk)) return rc;
  if (int rc = fold_alloc(&buf.u, 192 * chunk)) return rc;
  if (int rc = fold_alloc(&buf.c, PB * chunk)) return rc;
  if (int rc = fold_alloc(&buf.flags, 2 * chunk)) return rc;
  if (int rc = fold_alloc(&buf.partials, TB * max_wg)) return rc;
  // small: 256 point sums of workgroups | T | F | S, T in wire form | F in wire form | the verdict
  const size_t off_t = 256 * PB, off_f = off_t + PB, off_st = off_f + TB, off_fw = off_st + 2 * 192, off_acc = off_fw + 8 * wt;
  if (int rc = fold_alloc(&buf.small, off_acc + 16)) return rc;
  const bool prepared = vk_inputs_prepared(vk);
  const uint32_t s_ipl = prepared ? vk_inputs_per_lane(vk, 1, (uint32_t)ni + 1u) : 0u;
  VkInputWs ws;
  if (prepared) {
    if (int rc = fold_alloc(&buf.cacc, 4 * (size_t)FPS_WORDS * ni)) return rc;
    if (int rc = fold_alloc(&buf.sints, 96 * (ni + 1))) return rc;
    if (int rc = fold_alloc(&buf.wpart, vk_inputs_partials_bytes(1, (uint32_t)ni + 1u, s_ipl))) return rc;
    if (int rc = fold_alloc(&buf.wsums, vk_inputs_sums_bytes(1))) return rc;
    if (int rc = fold_alloc(&buf.wpre, vk_inputs_pre_bytes(1))) return rc;
    ws.partials = reinterpret_cast<uint32_t*>(buf.wpart);
    ws.sums = reinterpret_cast<uint32_t*>(buf.wsums);
    ws.pre = reinterpret_cast<uint32_t*>(buf.wpre);
  }
  char* small = reinterpret_cast<char*>(buf.small);
  uint32_t *pt_part = reinterpret_cast<uint32_t*>(small), *t_acc = reinterpret_cast<uint32_t*>(small + off_t), *f_acc = reinterpret_cast<uint32_t*>(small + off_f),
           *st_wire = reinterpret_cast<uint32_t*>(small + off_st), *f_wire = reinterpret_cast<uint32_t*>(small + off_fw),
           *dev_accepted = reinterpret_cast<uint32_t*>(small + off_acc);
  uint8_t* dev_bad = reinterpret_cast<uint8_t*>(buf.flags);
  uint8_t* dev_status = dev_bad + chunk;
  const uint32_t* key = reinterpret_cast<const uint32_t*>(vk->dev_key);

  std::vector<uint8_t> own_status;
  if (!status) { own_status.resize(n); status = own_status.data(); }
  uint64_t rho[12] = {0};                            // sum rho_i as an integer: below 2^152, so below r
  std::vector<Fr> cj(ni, Fr::zero());                // c_j = sum_i rho_i x_ij in Fr
  std::vector<uint64_t> rhom;                        // rho_i of a chunk as elements of Fr, wire (Montgomery) form
  Fr r2;
  memcpy(r2.l, FPC[FR].r2_64, sizeof(r2.l));
  size_t flagged = 0;
  FoldEvents ev;
  float ms[3] = {0.f, 0.f, 0.f};
  for (size_t first = 0; first < n; first += chunk) {
    const size_t cnt = n - first < chunk ? n - first : chunk;
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
    for (size_t k = 0; k < cnt; ++k) {
      unsigned __int128 carry = 0;
      for (int w = 0; w < 4; ++w) {
        carry += (unsigned __int128)rho[w] + (w < 2 ? ck[2 * k + w] : 0);
        rho[w] = (uint64_t)carry;
        carry >>= 64;
      }
    }
    const dim3 g1((unsigned)((cnt + 255) / 256)), b(256);
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
    // scale: U_i and rho_i C_i; then T += sum rho_i C_i
    ev.mark(0, st);
    hipLaunchKernelGGL((k_fold_scale<C1>), g1, b, 0, st, p32, (uint32_t)(2 * pw), reinterpret_cast<const uint32_t*>(buf.coef), key, dev_bad,
                       reinterpret_cast<uint32_t*>(buf.u), reinterpret_cast<uint32_t*>(buf.c), (uint32_t)cnt);
    const unsigned sum_wg = g1.x < 256u ? g1.x : 256u;
    hipLaunchKernelGGL((k_fold_point_sum<C1>), dim3(sum_wg), b, 0, st, reinterpret_cast<uint32_t*>(buf.c), (uint32_t)cnt, (const uint32_t*)nullptr, pt_part);
    hipLaunchKernelGGL((k_fold_point_sum<C1>), dim3(1), b, 0, st, pt_part, (uint32_t)sum_wg, first ? (const uint32_t*)t_acc : (const uint32_t*)nullptr, t_acc);
    // Miller and fold: F *= prod ML(U_i, B_i)
    ev.mark(1, st);
    const unsigned wg = blocks_for<F>(cnt);
    hipLaunchKernelGGL((k_fold_miller<C, C1>), dim3(wg), b, 0, st, p32, reinterpret_cast<const uint32_t*>(buf.u), key, dev_bad, dev_status,
                       reinterpret_cast<uint32_t*>(buf.partials), (uint32_t)cnt);
    hipLaunchKernelGGL((k_fold_reduce<C>), dim3(1), b, 0, st, reinterpret_cast<const uint32_t*>(buf.partials), (uint32_t)wg, f_acc, first ? 0 : 1);
    ev.mark(2, st);
    HIP_TRY(hipGetLastError());
    // c_j += sum_i rho_i x_ij: one reduction over Fr per public input (mnt753_vec_dot); the column of input j is the input vector
    // itself for one input, else gathered into the room k_inputs_to_integer no longer needs
    // A prepared key: all columns in one launch, the sums carried on the device from chunk to chunk.
    if (prepared) {
      if (int rc = vk_inputs_dots_enqueue(curve, reinterpret_cast<const uint32_t*>(buf.rhom), reinterpret_cast<const uint32_t*>(di), cnt, (uint32_t)ni,
                                          reinterpret_cast<uint32_t*>(buf.cacc), first ? 1 : 0, st)) return rc;
    }
    for (size_t j = 0; j < ni && !prepared; ++j) {
      const uint64_t* col = di;
      if (ni > 1) {
        HIP_TRY(hipMemcpy2DAsync(buf.ints, 96, reinterpret_cast<const char*>(di) + 96 * j, 96 * ni, 96, cnt, hipMemcpyDeviceToDevice, st));
        col = reinterpret_cast<const uint64_t*>(buf.ints);
      }
      uint64_t part[12];
      if (int rc = mnt753_vec_dot(curve, reinterpret_cast<const uint64_t*>(buf.rhom), col, cnt, part, st)) return rc;
      cj[j] = cj[j] + Fr::from_words(part);
    }
    HIP_TRY(hipMemcpyAsync(status + first, dev_status, cnt, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t k = 0; k < cnt; ++k) flagged += status[first + k] != 0;
    ev.add(ms[0], 0, 1);
    ev.add(ms[1], 1, 2);
  }
  // S = rho ABC[0] + sum_j c_j ABC[j + 1]: on the device through the tables of a prepared key, else on the host by num_inputs + 1
  // scalings of single points (mnt753_point_scale / _add)
  Fr rho_fr = Fr::from_words(rho) * r2;
  uint64_t s_aff[24];
  if (prepared) {
    // on the device, as ONE proof of num_inputs + 1 scalars against the tables of ABC[0 ..]: rho itself is an integer below r
    uint32_t* sints = reinterpret_cast<uint32_t*>(buf.sints);
    HIP_TRY(hipMemcpyAsync(sints, rho, 96, hipMemcpyHostToDevice, st));
    if (int rc = vk_inputs_fold_scalars_enqueue(curve, reinterpret_cast<const uint32_t*>(buf.cacc), (uint32_t)ni, sints + 24, st)) return rc;
    if (int rc = vk_inputs_enqueue(vk, sints, 1, (uint32_t)ni + 1u, 0u, nullptr, s_ipl, ws, st_wire, st)) return rc;
    if (parts && parts->s) HIP_TRY(hipMemcpyAsync(s_aff, st_wire, 192, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));               // rho and s_aff are the stack's
  } else {
    std::vector<uint64_t> p(36), q(36), sum(36);
    for (size_t j = 0; j <= ni; ++j) {
      if (int rc = mnt753_point_from_affine(curve, MNT753_G1, vk->abc.data() + 24 * j, p.data())) return rc;
      if (int rc = mnt753_point_scale(curve, MNT753_G1, j == 0 ? rho_fr.l : cj[j - 1].l, p.data(), q.data())) return rc;
      if (j == 0) sum = q;
      else if (int rc = mnt753_point_add(curve, MNT753_G1, sum.data(), q.data(), sum.data())) return rc;
    }
    if (int rc = mnt753_point_to_affine(curve, MNT753_G1, sum.data(), s_aff)) return rc;
  }
  if (!prepared) HIP_TRY(hipMemcpyAsync(st_wire, s_aff, 192, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL((k_fold_point_affine<C1>), dim3(1), dim3(64), 0, st, (const uint32_t*)t_acc, st_wire + 48);
  *accepted = 0;
  if (!flagged) {
    // the tail, once per call: the two stored pairs of the key, the final exponentiation, e(alpha, beta)^rho
    FoldExp e;
    int bits = 0;
    for (int w = 0; w < 8; ++w) {
      e.w[w] = (uint32_t)(rho[w >> 1] >> (32 * (w & 1)));
      if (e.w[w]) bits = 32 * w + 32 - __builtin_clz(e.w[w]);
    }
    ev.mark(0, st);
    hipLaunchKernelGGL((k_fold_tail<C, C1>), dim3(1), dim3(64), 0, st, (const uint32_t*)f_acc, (const uint32_t*)st_wire, (const uint32_t*)(st_wire + 48), key,
                       (const uint32_t*)vk->dev_coeffs, e, bits, dev_accepted);
    ev.mark(1, st);
    HIP_TRY(hipGetLastError());
    uint32_t ok = 0;
    HIP_TRY(hipMemcpyAsync(&ok, dev_accepted, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *accepted = ok ? 1 : 0;
    ev.add(ms[2], 0, 1);
  }
  if (parts) {
    if (parts->f) {
      hipLaunchKernelGGL((k_fold_export<C>), dim3(1), dim3(64), 0, st, (const uint32_t*)f_acc, f_wire);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(parts->f, f_wire, 8 * wt, hipMemcpyDeviceToHost, st));
    }
    if (parts->s) memcpy(parts->s, s_aff, 192);
    if (parts->t) HIP_TRY(hipMemcpyAsync(parts->t, st_wire + 48, 192, hipMemcpyDeviceToHost, st));
    if (parts->rho) memcpy(parts->rho, rho_fr.l, 96);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));                 // the call's buffers go when it returns
  for (int k = 0; k < 3; ++k) t_fold_ms[k] = ms[k];
  return 0;
}

}  // namespace

int groth16_verify_folded_parts(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int on_device, const uint64_t* coefficients,
                                uint8_t* status, int* accepted, void* stream, const FoldParts* parts) {
  if (!vk || !accepted || (n && (!proofs || !coefficients || (vk->num_inputs && !inputs))) || n > FOLD_MAX)
    return set_error(MNT753_EINVAL, "groth16_verify_folded: bad argument");
  for (size_t k = 0; k < n; ++k)
    if (!(coefficients[2 * k] | coefficients[2 * k + 1])) return set_error(MNT753_EINVAL, "groth16_verify_folded: a coefficient is zero");
  if (int rc = require_device()) return rc;
  if (!n) { *accepted = 1; return 0; }
  OnDevice guard(vk->device);
  if (on_device && (!fold_on_device_of(proofs, vk->device) || (vk->num_inputs && !fold_on_device_of(inputs, vk->device))))
    return set_error(MNT753_EINVAL, "groth16_verify_folded: proofs and inputs must lie on the device of the key");
  hipStream_t st = (hipStream_t)stream;
  if (vk->curve == MNT753_CURVE_MNT4753) return fold_t<Mnt4G2S, Mnt4G1, MOD_A>(vk, proofs, inputs, n, on_device, coefficients, status, accepted, st, parts);
  return fold_t<Mnt6G2S, Mnt6G1, MOD_B>(vk, proofs, inputs, n, on_device, coefficients, status, accepted, st, parts);
}

void groth16_fold_last_timing(float out_ms[3]) {
  for (int k = 0; k < 3; ++k) out_ms[k] = t_fold_ms[k];
}

}  // namespace mnt753

extern "C" int mnt753_groth16_verify_folded(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int on_device,
                                            const uint64_t* coefficients, uint8_t* status, int* accepted, void* stream) {
  return mnt753::groth16_verify_folded_parts(vk, proofs, inputs, n, on_device, coefficients, status, accepted, stream, nullptr);
}
