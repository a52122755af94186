// C ABI of the pairing and of Groth16 verification: mnt753_gt_words, mnt753_pairing, mnt753_vk_*, mnt753_groth16_verify[_ex], and of
// the subgroup test of a point set, mnt753_check_subgroup (include/mnt753_hip.h).  Kernels: pairing_kernels.hip.h.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include "common_host.hpp"
#include "compress_api.hpp"
#include "mnt753_generators.h"
#include "pairing_kernels.hip.h"
#include "vk_inputs_api.hpp"
#include "vk_object.hpp"

namespace mnt753 {
namespace {

// device memory of one call
struct PairingBuffers {
  void *g1 = nullptr, *g2 = nullptr, *out = nullptr, *stand = nullptr, *ints = nullptr;
  void *part = nullptr, *sums = nullptr, *pre = nullptr;   // a prepared key's walk: the partials, the sums, the prefix products (VkInputWs)
  ~PairingBuffers() {
    for (void* p : {g1, g2, out, stand, ints, part, sums, pre})
      if (p) (void)hipFree(p);
  }
};

// device memory of mnt753_groth16_verify_compressed beside those
struct CompressedStage {
  void *x = nullptr, *flags = nullptr, *rec = nullptr;
  ~CompressedStage() {
    for (void* p : {x, flags, rec})
      if (p) (void)hipFree(p);
  }
};

int alloc(void** p, size_t bytes) {
  if (hipMalloc(p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return set_error(MNT753_ENOMEM, "pairing: device allocation failed");
  }
  return 0;
}

// the workspace of a prepared key's walk for chunks of `chunk` proofs at ipl inputs per lane
int alloc_input_ws(PairingBuffers& buf, const mnt753_vk* vk, size_t chunk, uint32_t ipl, VkInputWs* ws) {
  if (int rc = alloc(&buf.part, vk_inputs_partials_bytes(chunk, (uint32_t)vk->num_inputs, ipl))) return rc;
  if (int rc = alloc(&buf.sums, vk_inputs_sums_bytes(chunk))) return rc;
  if (int rc = alloc(&buf.pre, vk_inputs_pre_bytes(chunk))) return rc;
  ws->partials = reinterpret_cast<uint32_t*>(buf.part);
  ws->sums = reinterpret_cast<uint32_t*>(buf.sums);
  ws->pre = reinterpret_cast<uint32_t*>(buf.pre);
  return 0;
}

bool y_is_zero(const uint64_t* pt, size_t words) {
  for (size_t k = words / 2; k < words; ++k)
    if (pt[k]) return false;
  return true;
}

constexpr size_t VERIFY_CHUNK = (size_t)1 << 16;   // proofs per launch: bounds the workspace of a batch

constexpr size_t MAX_PAIRINGS = (size_t)1 << 24;   // logical lanes are 32-bit, and the grid is n / 128 (n / 84) workgroups

}  // namespace
}  // namespace mnt753

using namespace mnt753;

extern "C" {

size_t mnt753_gt_words(int curve) { return curve == MNT753_CURVE_MNT4753 ? 48 : (curve == MNT753_CURVE_MNT6753 ? 72 : 0); }

int mnt753_pairing(int curve, const uint64_t* g1_affine, const uint64_t* g2_affine, size_t n, int on_device, uint64_t* out_gt, void* stream) {
  if (curve < 0 || curve > 1 || (n && (!g1_affine || !g2_affine || !out_gt)) || n > MAX_PAIRINGS) return set_error(MNT753_EINVAL, "pairing: bad argument");
  if (int rc = require_device()) return rc;
  if (!n) return 0;
  hipStream_t st = (hipStream_t)stream;
  const size_t w2 = mnt753_affine_words(curve, MNT753_G2), wt = mnt753_gt_words(curve);
  PairingBuffers buf;
  uint64_t* dev_out = out_gt;
  if (!on_device) {
    if (int rc = alloc(&buf.g1, 8 * 24 * n)) return rc;
    if (int rc = alloc(&buf.g2, 8 * w2 * n)) return rc;
    if (int rc = alloc(&buf.out, 8 * wt * n)) return rc;
    HIP_TRY(hipMemcpyAsync(buf.g1, g1_affine, 8 * 24 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(buf.g2, g2_affine, 8 * w2 * n, hipMemcpyHostToDevice, st));
    g1_affine = reinterpret_cast<const uint64_t*>(buf.g1);
    g2_affine = reinterpret_cast<const uint64_t*>(buf.g2);
    dev_out = reinterpret_cast<uint64_t*>(buf.out);
  }
  // is_well_formed() of both arguments: a malformed point is an error of the call, nothing is computed
  for (int group = MNT753_G1; group <= MNT753_G2; ++group) {
    mnt753_check_report rep;
    if (int rc = mnt753_check_points(curve, group, group == MNT753_G1 ? g1_affine : g2_affine, 1, n, &rep, stream)) return rc;
    if (rep.n_bad) return set_error(MNT753_EINPUT, group == MNT753_G1 ? "pairing: a G1 point is non-canonical or off the curve"
                                                                       : "pairing: a G2 point is non-canonical or off the curve");
  }
  // the stand-in pair of a lane group whose argument is the identity: the generators
  if (int rc = alloc(&buf.stand, 8 * (24 + w2))) return rc;
  HIP_TRY(hipMemcpyAsync(buf.stand, curve == MNT753_CURVE_MNT4753 ? GEN_MNT4_G1 : GEN_MNT6_G1, 8 * 24, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(reinterpret_cast<uint64_t*>(buf.stand) + 24, curve == MNT753_CURVE_MNT4753 ? GEN_MNT4_G2 : GEN_MNT6_G2, 8 * w2,
                         hipMemcpyHostToDevice, st));
  const uint32_t* s1 = reinterpret_cast<const uint32_t*>(buf.stand);
  const uint32_t* s2 = s1 + 48;
  const uint32_t *p1 = reinterpret_cast<const uint32_t*>(g1_affine), *p2 = reinterpret_cast<const uint32_t*>(g2_affine);
  uint32_t* po = reinterpret_cast<uint32_t*>(dev_out);
  if (curve == MNT753_CURVE_MNT4753)
    hipLaunchKernelGGL((k_pairing<Mnt4G2S>), dim3(blocks_for<Mnt4G2S::F>(n)), dim3(256), 0, st, p1, p2, s1, s2, po, (uint32_t)n, 0);
  else
    hipLaunchKernelGGL((k_pairing<Mnt6G2S>), dim3(blocks_for<Mnt6G2S::F>(n)), dim3(256), 0, st, p1, p2, s1, s2, po, (uint32_t)n, 0);
  HIP_TRY(hipGetLastError());
  if (!on_device) HIP_TRY(hipMemcpyAsync(out_gt, dev_out, 8 * wt * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));             // the call's buffers go when it returns
  return 0;
}

int mnt753_vk_create(int curve, const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* delta_g2, const uint64_t* abc_g1, size_t num_inputs,
                     mnt753_vk** out) {
  if (curve < 0 || curve > 1 || !alpha_g1 || !beta_g2 || !delta_g2 || !abc_g1 || !out || num_inputs > ((size_t)1 << 20))
    return set_error(MNT753_EINVAL, "vk_create: bad argument");
  if (int rc = require_device()) return rc;
  const size_t w2 = mnt753_affine_words(curve, MNT753_G2), wt = mnt753_gt_words(curve);
  // every element of a key is a point of its curve other than the identity
  struct { const uint64_t* p; int group; size_t n; } parts[4] = {{alpha_g1, MNT753_G1, 1}, {beta_g2, MNT753_G2, 1}, {delta_g2, MNT753_G2, 1},
                                                                {abc_g1, MNT753_G1, num_inputs + 1}};
  for (const auto& part : parts) {
    const size_t w = part.group == MNT753_G1 ? 24 : w2;
    for (size_t k = 0; k < part.n; ++k)
      if (y_is_zero(part.p + k * w, w)) return set_error(MNT753_EINVAL, "vk_create: an element of the key is the identity");
    mnt753_check_report rep;
    if (int rc = mnt753_check_points(curve, part.group, part.p, 0, part.n, &rep, nullptr)) return rc;
    if (rep.n_bad) return set_error(MNT753_EINPUT, "vk_create: an element of the key is non-canonical or off its curve");
  }
  mnt753_vk* vk = new mnt753_vk;
  vk->curve = curve;
  vk->device = current_physical_device();
  vk->num_inputs = num_inputs;
  vk->delta.assign(delta_g2, delta_g2 + w2);
  vk->abc.assign(abc_g1, abc_g1 + 24 * (num_inputs + 1));
  vk->gt.resize(wt);
  int rc = mnt753_pairing(curve, alpha_g1, beta_g2, 1, 0, vk->gt.data(), nullptr);
  if (!rc) {
    std::vector<uint64_t> key(24 + 2 * w2 + wt);
    memcpy(key.data(), curve == MNT753_CURVE_MNT4753 ? GEN_MNT4_G1 : GEN_MNT6_G1, 8 * 24);
    memcpy(key.data() + 24, curve == MNT753_CURVE_MNT4753 ? GEN_MNT4_G2 : GEN_MNT6_G2, 8 * w2);
    memcpy(key.data() + 24 + w2, delta_g2, 8 * w2);
    memcpy(key.data() + 24 + 2 * w2, vk->gt.data(), 8 * wt);
    if (hipMalloc(&vk->dev_key, 8 * key.size()) != hipSuccess || hipMalloc(&vk->dev_abc, 8 * vk->abc.size()) != hipSuccess) {
      (void)hipGetLastError();
      rc = set_error(MNT753_ENOMEM, "vk_create: device allocation failed");
    } else if (hipMemcpy(vk->dev_key, key.data(), 8 * key.size(), hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(vk->dev_abc, vk->abc.data(), 8 * vk->abc.size(), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      rc = set_error(MNT753_EHIP, "vk_create: copy to the device failed");
    } else {
      // ate_precompute_G2 of G2::one() and delta_g2, once: one lane group each, into the key object
      const size_t cw = curve == MNT753_CURVE_MNT4753 ? ate_coeff_words<Mnt4G2S>() : ate_coeff_words<Mnt6G2S>();
      if (hipMalloc(&vk->dev_coeffs, 4 * 2 * cw) != hipSuccess) {
        (void)hipGetLastError();
        rc = set_error(MNT753_ENOMEM, "vk_create: device allocation failed");
      } else {
        const uint32_t* k32 = reinterpret_cast<const uint32_t*>(vk->dev_key);
        for (int which = 0; which < 2; ++which) {
          const uint32_t* q = k32 + 48 + which * 2 * w2;          // G2::one(), then delta_g2
          if (curve == MNT753_CURVE_MNT4753) hipLaunchKernelGGL((k_g2_precompute<Mnt4G2S>), dim3(1), dim3(256), 0, 0, q, vk->dev_coeffs + which * cw);
          else hipLaunchKernelGGL((k_g2_precompute<Mnt6G2S>), dim3(1), dim3(256), 0, 0, q, vk->dev_coeffs + which * cw);
        }
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
          (void)hipGetLastError();
          rc = set_error(MNT753_EHIP, "vk_create: the precomputation of the key's G2 points failed");
        }
      }
    }
  }
  if (rc) { mnt753_vk_destroy(vk); return rc; }
  *out = vk;
  return 0;
}

int mnt753_vk_destroy(mnt753_vk* vk) {
  if (!vk) return 0;
  OnDevice guard(vk->device);
  (void)mnt753_vk_release_inputs(vk);
  if (vk->dev_key) (void)hipFree(vk->dev_key);
  if (vk->dev_abc) (void)hipFree(vk->dev_abc);
  if (vk->dev_coeffs) (void)hipFree(vk->dev_coeffs);
  delete vk;
  return 0;
}

size_t mnt753_vk_num_inputs(const mnt753_vk* vk) { return vk ? vk->num_inputs : 0; }

size_t mnt753_vk_coefficient_bytes(const mnt753_vk* vk) {
  if (!vk) return 0;
  return 4 * 2 * (size_t)(vk->curve == MNT753_CURVE_MNT4753 ? ate_coeff_words<Mnt4G2S>() : ate_coeff_words<Mnt6G2S>());
}

int mnt753_vk_set_workspace_cap(mnt753_vk* vk, size_t bytes) {
  if (!vk) return set_error(MNT753_EINVAL, "vk_set_workspace_cap: bad argument");
  vk->workspace_cap = bytes;
  return 0;
}

int mnt753_vk_gt(const mnt753_vk* vk, uint64_t* out) {
  if (!vk || !out) return set_error(MNT753_EINVAL, "vk_gt: bad argument");
  memcpy(out, vk->gt.data(), 8 * vk->gt.size());
  return 0;
}

int mnt753_vk_serialize(const mnt753_vk* vk, uint8_t* buf, size_t cap, size_t* len) {
  if (!vk || !len) return set_error(MNT753_EINVAL, "vk_serialize: bad argument");
  std::vector<uint8_t> o;
  auto raw = [&](const uint64_t* p, size_t words) { o.insert(o.end(), (const uint8_t*)p, (const uint8_t*)p + 8 * words); };
  auto num = [&](size_t v) { char t[32]; const int k = snprintf(t, sizeof(t), "%zu\n", v); o.insert(o.end(), t, t + k); };
  // operator<< of r1cs_gg_ppzksnark_verification_key: alpha_g1_beta_g2, delta_g2, ABC_g1 (an accumulation_vector: first, then the
  // sparse_vector of the rest); a point under NO_PT_COMPRESSION is the byte '0' (not the identity) and X | Y
  raw(vk->gt.data(), vk->gt.size());
  o.push_back('0'); raw(vk->delta.data(), vk->delta.size());
  o.push_back('0'); raw(vk->abc.data(), 24);
  const size_t n = vk->num_inputs;
  num(n); num(n);
  for (size_t i = 0; i < n; ++i) num(i);
  num(n);
  for (size_t j = 1; j <= n; ++j) { o.push_back('0'); raw(vk->abc.data() + 24 * j, 24); }
  *len = o.size();
  if (!buf) return 0;                            // the size only
  if (cap < o.size()) return set_error(MNT753_EINVAL, "vk_serialize: buffer too small");
  memcpy(buf, o.data(), o.size());
  return 0;
}

namespace {
// inputs (device, n x num_inputs Fr) -> dev_acc (n G1 points, affine wire form), dev_bad[t] = 1 where an input is >= r.  ints: room for
// the inputs as integers, 96 num_inputs n bytes (unused without inputs).  Enqueues only.  A prepared key (ws, ipl: its workspace and the
// inputs per lane of this call's chunks) walks its input tables instead of k_vk_accumulate: the same words in dev_acc.
int accumulate_on_device(const mnt753_vk* vk, const uint64_t* dev_inputs, size_t n, uint64_t* dev_acc, uint8_t* dev_bad, uint32_t* ints, const VkInputWs* ws,
                         uint32_t ipl, hipStream_t st) {
  const size_t ni = vk->num_inputs;
  if (!ni) HIP_TRY(hipMemsetAsync(dev_bad, 0, n, st));
  const dim3 g((unsigned)((n + 255) / 256)), b(256);
  const uint32_t* in = reinterpret_cast<const uint32_t*>(dev_inputs);
  const uint32_t* abc = reinterpret_cast<const uint32_t*>(vk->dev_abc);
  uint32_t* out = reinterpret_cast<uint32_t*>(dev_acc);
  const bool mnt4 = vk->curve == MNT753_CURVE_MNT4753;
  if (ni) {
    if (mnt4) hipLaunchKernelGGL((k_inputs_to_integer<MOD_A>), g, b, 0, st, in, ints, dev_bad, (uint32_t)n, (uint32_t)ni);
    else hipLaunchKernelGGL((k_inputs_to_integer<MOD_B>), g, b, 0, st, in, ints, dev_bad, (uint32_t)n, (uint32_t)ni);
  }
  // the one difference between the two paths: the tables of a prepared key (which has inputs), or one lane per proof
  if (vk_inputs_prepared(vk)) {
    HIP_TRY(hipGetLastError());
    return vk_inputs_enqueue(vk, ints, n, (uint32_t)ni, 1u, abc, ipl, *ws, out, st);
  }
  if (mnt4) hipLaunchKernelGGL((k_vk_accumulate<Mnt4G1>), g, b, 0, st, abc, ints, out, (uint32_t)n, (uint32_t)ni);
  else hipLaunchKernelGGL((k_vk_accumulate<Mnt6G1>), g, b, 0, st, abc, ints, out, (uint32_t)n, (uint32_t)ni);
  HIP_TRY(hipGetLastError());
  return 0;
}
// a device pointer of the caller lies on the key's device
bool on_device_of(const void* p, int device) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.device == device;
}
}  // namespace

int mnt753_vk_accumulate(const mnt753_vk* vk, const uint64_t* inputs, size_t n, uint64_t* out_affine) {
  if (!vk || (n && (!out_affine || (vk->num_inputs && !inputs))) || n > MAX_PAIRINGS) return set_error(MNT753_EINVAL, "vk_accumulate: bad argument");
  if (int rc = require_device()) return rc;
  if (!n) return 0;
  OnDevice guard(vk->device);
  PairingBuffers buf;   // g1: the inputs, out: the points, g2: the flags
  const size_t ni = vk->num_inputs;
  if (ni) {
    if (int rc = alloc(&buf.g1, 96 * ni * n)) return rc;
    if (int rc = alloc(&buf.ints, 96 * ni * n)) return rc;
    HIP_TRY(hipMemcpy(buf.g1, inputs, 96 * ni * n, hipMemcpyHostToDevice));
  }
  if (int rc = alloc(&buf.out, 192 * n)) return rc;
  if (int rc = alloc(&buf.g2, n)) return rc;
  VkInputWs ws;
  uint32_t ipl = 0;
  if (vk_inputs_prepared(vk)) {
    ipl = vk_inputs_per_lane(vk, n, (uint32_t)ni);
    if (int rc = alloc_input_ws(buf, vk, n, ipl, &ws)) return rc;
  }
  if (int rc = accumulate_on_device(vk, reinterpret_cast<const uint64_t*>(buf.g1), n, reinterpret_cast<uint64_t*>(buf.out),
                                    reinterpret_cast<uint8_t*>(buf.g2), reinterpret_cast<uint32_t*>(buf.ints), &ws, ipl, nullptr)) return rc;
  HIP_TRY(hipStreamSynchronize(nullptr));
  std::vector<uint8_t> bad(n);
  HIP_TRY(hipMemcpy(bad.data(), buf.g2, n, hipMemcpyDeviceToHost));
  for (uint8_t b : bad)
    if (b) return set_error(MNT753_EINPUT, "vk_accumulate: an input is not below r");
  HIP_TRY(hipMemcpy(out_affine, buf.out, 192 * n, hipMemcpyDeviceToHost));
  return 0;
}

int mnt753_groth16_verify(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int on_device, uint8_t* verdicts, void* stream) {
  return mnt753_groth16_verify_ex(vk, proofs, inputs, n, on_device, 0u, verdicts, stream);
}

namespace {
// mnt753_groth16_verify_ex (cx == nullptr: proofs holds affine proofs) and mnt753_groth16_verify_compressed (cx, cflags: the packed
// compressed proofs, n x (x_A | x_B | x_C) and n x 3 flag bytes; proofs unused): the same chunks, buffers and kernels, with a chunk of
// compressed proofs decompressed into the affine staging buffer first.  A point that does not decompress, and an identity flag, leave
// zero words there, which the verifier reads as the identity: verdict 1.
int verify_chunks(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* cx, const uint8_t* cflags, const uint64_t* inputs, size_t n, int on_device,
                  unsigned flags, uint8_t* verdicts, void* stream) {
  const bool compressed = cx != nullptr;
  if (!vk || (n && ((!compressed && !proofs) || (compressed && !cflags) || !verdicts || (vk->num_inputs && !inputs))) || n > MAX_PAIRINGS ||
      (flags & ~MNT753_VERIFY_CHECK_SUBGROUP))
    return set_error(MNT753_EINVAL, "groth16_verify: bad argument");
  const bool sub = (flags & MNT753_VERIFY_CHECK_SUBGROUP) != 0;
  if (int rc = require_device()) return rc;
  if (!n) return 0;
  OnDevice guard(vk->device);
  hipStream_t st = (hipStream_t)stream;
  const size_t ni = vk->num_inputs, w2 = mnt753_affine_words(vk->curve, MNT753_G2), pw = 48 + w2;   // words of one proof
  const size_t xw = 24 + w2 / 2;                  // words of one compressed proof
  if (on_device && (!on_device_of(compressed ? (const void*)cx : (const void*)proofs, vk->device) || (compressed && !on_device_of(cflags, vk->device)) ||
                    (ni && !on_device_of(inputs, vk->device))))
    return set_error(MNT753_EINVAL, "groth16_verify: proofs and inputs must lie on the device of the key");
  // what one proof of a chunk takes: the accumulated point, the inputs as integers, flag and verdict, and its staged copy if it
  // arrives in host memory; a compressed proof: its decompressed words as well.  The cap of the key bounds the chunk (at least one
  // proof, at most 2^16).
  // A prepared key: the partials, the sum and the prefix product of its walk as well, at the inputs per lane of the uncapped chunk.
  // The inputs per lane belong to the chunk that runs: a cap that shrinks the chunk asks for more slices per proof, whose partials
  // shrink it again -- settled in a few rounds (the chunk only falls, the slices only rise; the last round's pair is kept).
  size_t chunk = n < VERIFY_CHUNK ? n : VERIFY_CHUNK;
  const bool prepared = vk_inputs_prepared(vk);
  const size_t base_per_proof = 194 + 96 * ni + (compressed ? 8 * pw : 0) + (on_device ? 0 : (compressed ? 8 * xw + 3 : 8 * pw) + 96 * ni);
  uint32_t ipl = prepared ? vk_inputs_per_lane(vk, chunk, (uint32_t)ni) : 0u;
  for (int round = 0; round < 8; ++round) {
    const size_t per_proof = base_per_proof + (prepared ? (size_t)vki_workspace_per_proof((uint32_t)ni, ipl) : 0);
    size_t fits = chunk;
    if (vk->workspace_cap && vk->workspace_cap / per_proof < chunk) fits = vk->workspace_cap / per_proof ? vk->workspace_cap / per_proof : 1;
    const uint32_t next = prepared ? vk_inputs_per_lane(vk, fits, (uint32_t)ni) : 0u;
    const bool settled = fits == chunk && next == ipl;
    chunk = fits;
    if (settled || !prepared) break;
    if (next < ipl) ipl = next;          // more slices for the smaller chunk; never fewer, so that the rounds end
    else break;
  }
  if (prepared && vk->workspace_cap) {   // (rounds that did not settle: the chunk of the last pair still has to fit its own slices)
    const size_t per_proof = base_per_proof + (size_t)vki_workspace_per_proof((uint32_t)ni, ipl);
    if (vk->workspace_cap / per_proof < chunk) chunk = vk->workspace_cap / per_proof ? vk->workspace_cap / per_proof : 1;
  }
  PairingBuffers buf;   // g1: staged (or decompressed) proofs, g2: staged inputs, out: accumulated points, stand: flags then verdicts, ints: inputs as integers
  CompressedStage cs;   // the staged compressed proofs of a host batch, and the record of the decompression (not read: the verdicts tell)
  if (!on_device || compressed) {
    if (int rc = alloc(&buf.g1, 8 * pw * chunk)) return rc;
  }
  if (!on_device) {
    if (ni) { if (int rc = alloc(&buf.g2, 96 * ni * chunk)) return rc; }
  }
  if (compressed) {
    if (!on_device) {
      if (int rc = alloc(&cs.x, 8 * xw * chunk)) return rc;
      if (int rc = alloc(&cs.flags, 3 * chunk)) return rc;
    }
    if (int rc = alloc(&cs.rec, decompress_report_bytes())) return rc;
    if (int rc = decompress_report_init(cs.rec, st)) return rc;
  }
  if (ni) { if (int rc = alloc(&buf.ints, 96 * ni * chunk)) return rc; }
  if (int rc = alloc(&buf.out, 192 * chunk)) return rc;
  if (int rc = alloc(&buf.stand, 2 * chunk)) return rc;
  VkInputWs ws;
  if (prepared) { if (int rc = alloc_input_ws(buf, vk, chunk, ipl, &ws)) return rc; }
  uint8_t* dev_bad = reinterpret_cast<uint8_t*>(buf.stand);
  uint8_t* dev_verdicts = dev_bad + chunk;
  size_t rejected = 0;
  for (size_t first = 0; first < n; first += chunk) {
    const size_t cnt = n - first < chunk ? n - first : chunk;
    const uint64_t* dp = compressed ? nullptr : proofs + first * pw;
    const uint64_t* di = ni ? inputs + first * ni * 12 : nullptr;
    if (compressed) {
      const uint64_t* dx = cx + first * xw;
      const uint8_t* df = cflags + first * 3;
      if (!on_device) {
        HIP_TRY(hipMemcpyAsync(cs.x, dx, 8 * xw * cnt, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(cs.flags, df, 3 * cnt, hipMemcpyHostToDevice, st));
        dx = reinterpret_cast<const uint64_t*>(cs.x);
        df = reinterpret_cast<const uint8_t*>(cs.flags);
      }
      // A, B, C of every proof into its A | B | C row; the stand-in x: the generators at the head of the key
      const uint32_t *x32 = reinterpret_cast<const uint32_t*>(dx), *key32 = reinterpret_cast<const uint32_t*>(vk->dev_key);
      uint32_t* o32 = reinterpret_cast<uint32_t*>(buf.g1);
      if (int rc = decompress_enqueue(vk->curve, MNT753_G1, x32, 2 * xw, df, 3, key32, o32, 2 * pw, cnt, first, cs.rec, st)) return rc;
      if (int rc = decompress_enqueue(vk->curve, MNT753_G2, x32 + 24, 2 * xw, df + 1, 3, key32 + 48, o32 + 48, 2 * pw, cnt, first, cs.rec, st)) return rc;
      if (int rc = decompress_enqueue(vk->curve, MNT753_G1, x32 + 24 + w2, 2 * xw, df + 2, 3, key32, o32 + 48 + 2 * w2, 2 * pw, cnt, first, cs.rec, st)) return rc;
      dp = reinterpret_cast<const uint64_t*>(buf.g1);
    }
    if (!on_device) {
      if (!compressed) {
        HIP_TRY(hipMemcpyAsync(buf.g1, dp, 8 * pw * cnt, hipMemcpyHostToDevice, st));
        dp = reinterpret_cast<const uint64_t*>(buf.g1);
      }
      if (ni) {
        HIP_TRY(hipMemcpyAsync(buf.g2, di, 96 * ni * cnt, hipMemcpyHostToDevice, st));
        di = reinterpret_cast<const uint64_t*>(buf.g2);
      }
    }
    if (int rc = accumulate_on_device(vk, di, cnt, reinterpret_cast<uint64_t*>(buf.out), dev_bad, reinterpret_cast<uint32_t*>(buf.ints), &ws, ipl, st)) return rc;
    const uint32_t *p = reinterpret_cast<const uint32_t*>(dp), *acc = reinterpret_cast<const uint32_t*>(buf.out),
                   *key = reinterpret_cast<const uint32_t*>(vk->dev_key);
    if (vk->curve == MNT753_CURVE_MNT4753) {
      const dim3 g(blocks_for<Mnt4G2S::F>(cnt)), b(256);
      if (sub) hipLaunchKernelGGL((k_groth16_verify<Mnt4G2S, Mnt4G1, true>), g, b, 0, st, p, acc, key, vk->dev_coeffs, dev_bad, dev_verdicts, (uint32_t)cnt);
      else hipLaunchKernelGGL((k_groth16_verify<Mnt4G2S, Mnt4G1>), g, b, 0, st, p, acc, key, vk->dev_coeffs, dev_bad, dev_verdicts, (uint32_t)cnt);
    } else {
      const dim3 g(blocks_for<Mnt6G2S::F>(cnt)), b(256);
      if (sub) hipLaunchKernelGGL((k_groth16_verify<Mnt6G2S, Mnt6G1, true>), g, b, 0, st, p, acc, key, vk->dev_coeffs, dev_bad, dev_verdicts, (uint32_t)cnt);
      else hipLaunchKernelGGL((k_groth16_verify<Mnt6G2S, Mnt6G1>), g, b, 0, st, p, acc, key, vk->dev_coeffs, dev_bad, dev_verdicts, (uint32_t)cnt);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(verdicts + first, dev_verdicts, cnt, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t k = 0; k < cnt; ++k) rejected += verdicts[first + k] != 0;
  }
  return (int)rejected;
}
}  // namespace

int mnt753_groth16_verify_ex(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int on_device, unsigned flags, uint8_t* verdicts,
                             void* stream) {
  return verify_chunks(vk, proofs, nullptr, nullptr, inputs, n, on_device, flags, verdicts, stream);
}

int mnt753_groth16_verify_compressed(const mnt753_vk* vk, const uint64_t* x, const uint8_t* flags, const uint64_t* inputs, size_t n, int on_device,
                                     unsigned verify_flags, uint8_t* verdicts, void* stream) {
  if (n && !x) return set_error(MNT753_EINVAL, "groth16_verify_compressed: bad argument");
  if (!n) {                                        // (verify_chunks tells the forms apart by x)
    if (!vk || (verify_flags & ~MNT753_VERIFY_CHECK_SUBGROUP)) return set_error(MNT753_EINVAL, "groth16_verify_compressed: bad argument");
    return require_device();
  }
  return verify_chunks(vk, nullptr, x, flags, inputs, n, on_device, verify_flags, verdicts, stream);
}

// Subgroup membership of n points.  G1 has cofactor 1 on both curves: mnt753_check_points' record is the answer.  G2: k_g2_subgroup,
// one lane group per point, in launches of at most MAX_PAIRINGS points (logical lanes are 32-bit); the record carries the index.
int mnt753_check_subgroup(int curve, int group, const uint64_t* affine, int on_device, size_t n, mnt753_check_report* out, void* stream) {
  if (curve < 0 || curve > 1 || (group != MNT753_G1 && group != MNT753_G2) || !out || (n && !affine) || n > ((size_t)1 << 38))
    return set_error(MNT753_EINVAL, "check_subgroup: bad argument");
  if (group == MNT753_G1) return mnt753_check_points(curve, group, affine, on_device, n, out, stream);
  if (int rc = require_device()) return rc;
  *out = mnt753_check_report{0, 0, MNT753_BAD_NONE, 0};
  if (!n) return 0;
  hipStream_t st = (hipStream_t)stream;
  const size_t w2 = mnt753_affine_words(curve, MNT753_G2);
  PairingBuffers buf;   // g2: the staged points, stand: the stand-in (the generator), out: the record
  if (!on_device) {
    if (int rc = alloc(&buf.g2, 8 * w2 * n)) return rc;
    HIP_TRY(hipMemcpyAsync(buf.g2, affine, 8 * w2 * n, hipMemcpyHostToDevice, st));
    affine = reinterpret_cast<const uint64_t*>(buf.g2);
  }
  if (int rc = alloc(&buf.stand, 8 * w2)) return rc;
  if (int rc = alloc(&buf.out, sizeof(SubgroupReport))) return rc;
  HIP_TRY(hipMemcpyAsync(buf.stand, curve == MNT753_CURVE_MNT4753 ? GEN_MNT4_G2 : GEN_MNT6_G2, 8 * w2, hipMemcpyHostToDevice, st));
  SubgroupReport* rec = reinterpret_cast<SubgroupReport*>(buf.out);
  hipLaunchKernelGGL(k_subgroup_report_init, dim3(1), dim3(1), 0, st, rec);
  const uint32_t* stand = reinterpret_cast<const uint32_t*>(buf.stand);
  for (size_t first = 0; first < n; first += MAX_PAIRINGS) {
    const size_t cnt = n - first < MAX_PAIRINGS ? n - first : MAX_PAIRINGS;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(affine + first * w2);
    if (curve == MNT753_CURVE_MNT4753)
      hipLaunchKernelGGL((k_g2_subgroup<Mnt4G2S>), dim3(blocks_for<Mnt4G2S::F>(cnt)), dim3(256), 0, st, p, stand, (uint32_t)cnt, (unsigned long long)first, rec);
    else
      hipLaunchKernelGGL((k_g2_subgroup<Mnt6G2S>), dim3(blocks_for<Mnt6G2S::F>(cnt)), dim3(256), 0, st, p, stand, (uint32_t)cnt, (unsigned long long)first, rec);
  }
  HIP_TRY(hipGetLastError());
  SubgroupReport host;
  HIP_TRY(hipMemcpyAsync(&host, rec, sizeof(host), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  out->n_bad = host.n_bad;
  out->first_bad = host.n_bad ? (uint64_t)(host.key >> 3) : 0;
  out->first_reason = host.n_bad ? (uint32_t)(host.key & 7u) : (uint32_t)MNT753_BAD_NONE;
  return 0;
}

}  // extern "C"
