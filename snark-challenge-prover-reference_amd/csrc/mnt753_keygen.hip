// The Groth16 generator from given randomness: r1cs_gg_ppzksnark_generator (libsnark/zk_proof_systems/ppzksnark/r1cs_gg_ppzksnark/
// r1cs_gg_ppzksnark.tcc:212-362) with t, alpha, beta, delta and the G1 generator as arguments.  This unit
// holds what the generator adds to the pieces that existed -- the ABC | Lt combination, the compaction of a vector's non-zero
// elements and the scatter of their rows (csrc/keygen_kernels.hip.h) -- and the orchestration over mnt753_r1cs_qap_at,
// mnt753_fixed_base_* / mnt753_batch_exp and mnt753_point_scale.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "batch_exp_api.hpp"
#include "common_host.hpp"
#include "host_field.hpp"
#include "keygen_kernels.hip.h"
#include "mnt753_generators.h"
#include "r1cs_api.hpp"

using namespace mnt753;

namespace {
constexpr int frm_of(int curve) { return curve == MNT753_CURVE_MNT4753 ? MOD_A : MOD_B; }
bool fr_geq_r(int curve, const uint64_t* x) { return curve == MNT753_CURVE_MNT4753 ? host::HFp<MOD_A>::geq_p(x) : host::HFp<MOD_B>::geq_p(x); }
bool words_zero(const uint64_t* x, size_t n) {
  uint64_t o = 0;
  for (size_t i = 0; i < n; ++i) o |= x[i];
  return o == 0;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
// out = 1 / a and out2 = b / a in Fr of the curve (wire form)
template <int M>
void fr_inv_and(const uint64_t* a, const uint64_t* b, uint64_t* inv, uint64_t* b_over_a) {
  const host::HFp<M> i = host::HFp<M>::from_words(a).inverse();
  memcpy(inv, i.l, 96);
  const host::HFp<M> q = host::HFp<M>::from_words(b) * i;
  memcpy(b_over_a, q.l, 96);
}

// device allocations and fixed-base objects of one call, released on every way out
struct Scratch {
  std::vector<void*> mem;
  mnt753_fixed_base* fb[2] = {nullptr, nullptr};
  template <class T>
  bool alloc(T** p, size_t bytes) {
    void* q = nullptr;
    if (hipMalloc(&q, bytes ? bytes : 16) != hipSuccess) { (void)hipGetLastError(); return false; }
    mem.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return true;
  }
  ~Scratch() {
    for (mnt753_fixed_base* f : fb) if (f) (void)mnt753_fixed_base_free(f);
    for (void* q : mem) (void)hipFree(q);
  }
};

const uint64_t* generator_words(int curve, int group) {
  return curve == MNT753_CURVE_MNT4753 ? (group == MNT753_G1 ? GEN_MNT4_G1 : GEN_MNT4_G2) : (group == MNT753_G1 ? GEN_MNT6_G1 : GEN_MNT6_G2);
}

// scalar * P for an affine P in host memory, affine out: mnt753_point_scale between the two conversions
int scale_affine(int curve, int group, const uint64_t* scalar, const uint64_t* affine, uint64_t* out_affine) {
  uint64_t p[108], q[108];
  if (int rc = mnt753_point_from_affine(curve, group, affine, p)) return rc;
  if (int rc = mnt753_point_scale(curve, group, scalar, p, q)) return rc;
  return mnt753_point_to_affine(curve, group, q, out_affine);
}
}  // namespace

extern "C" {

int mnt753_group_generator(int curve, int group, uint64_t* out_affine) {
  if (curve < 0 || curve > 1 || (group != MNT753_G1 && group != MNT753_G2) || !out_affine) return set_error(MNT753_EINVAL, "group_generator: bad argument");
  memcpy(out_affine, generator_words(curve, group), 8 * mnt753_affine_words(curve, group));
  return 0;
}

int mnt753_keygen_combine(int curve, const uint64_t* dev_At, const uint64_t* dev_Bt, const uint64_t* dev_Ct, size_t n, size_t num_inputs,
                          const uint64_t* host_beta, const uint64_t* host_alpha, const uint64_t* host_dinv, uint64_t* dev_out, void* stream) {
  if (curve < 0 || curve > 1 || !host_beta || !host_alpha || !host_dinv || (n && (!dev_At || !dev_Bt || !dev_Ct || !dev_out)))
    return set_error(MNT753_EINVAL, "keygen_combine: bad argument");
  if (fr_geq_r(curve, host_beta) || fr_geq_r(curve, host_alpha) || fr_geq_r(curve, host_dinv))
    return set_error(MNT753_EINVAL, "keygen_combine: a factor is not a canonical element of Fr");
  if (int rc = require_device()) return rc;
  if (n == 0) return 0;
  WireElem b, a, di;
  memcpy(b.w, host_beta, 96);
  memcpy(a.w, host_alpha, 96);
  memcpy(di.w, host_dinv, 96);
  const uint32_t *at = reinterpret_cast<const uint32_t*>(dev_At), *bt = reinterpret_cast<const uint32_t*>(dev_Bt), *ct = reinterpret_cast<const uint32_t*>(dev_Ct);
  uint32_t* o = reinterpret_cast<uint32_t*>(dev_out);
  const unsigned g = (unsigned)((n + 255) / 256);
  if (curve == MNT753_CURVE_MNT4753) hipLaunchKernelGGL((k_keygen_combine<MOD_A>), dim3(g), dim3(256), 0, (hipStream_t)stream, at, bt, ct, o, b, a, di, n, num_inputs);
  else hipLaunchKernelGGL((k_keygen_combine<MOD_B>), dim3(g), dim3(256), 0, (hipStream_t)stream, at, bt, ct, o, b, a, di, n, num_inputs);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mnt753_compact_nonzero(const uint64_t* dev_scalars, size_t n, uint64_t* dev_compact, uint32_t* dev_index, size_t* host_count, void* stream) {
  if (!host_count || (n && !dev_scalars) || (!dev_compact != !dev_index)) return set_error(MNT753_EINVAL, "compact_nonzero: bad argument");
  if (n >= ((size_t)1 << 32)) return set_error(MNT753_EINVAL, "compact_nonzero: n must be below 2^32 (32-bit indices)");
  if (!aligned16(dev_scalars) || !aligned16(dev_compact)) return set_error(MNT753_EINVAL, "compact_nonzero: vectors must be 16-byte aligned");
  if (int rc = require_device()) return rc;
  *host_count = 0;
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t nb = (uint32_t)((n + NZ_BLOCK - 1) / NZ_BLOCK);
  Scratch s;
  uint32_t* counts = nullptr;
  if (!s.alloc(&counts, 4 * ((size_t)nb + 1))) return set_error(MNT753_ENOMEM, "compact_nonzero: device allocation failed");
  hipLaunchKernelGGL(k_nz_count, dim3(nb), dim3(NZ_BLOCK), 0, st, dev_scalars, n, counts);
  hipLaunchKernelGGL(k_nz_scan, dim3(1), dim3(256), 0, st, counts, nb);
  if (dev_compact) hipLaunchKernelGGL(k_nz_write, dim3(nb), dim3(NZ_BLOCK), 0, st, dev_scalars, n, counts, dev_compact, dev_index);
  HIP_TRY(hipGetLastError());
  uint32_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, counts + nb, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *host_count = total;
  return 0;
}

int mnt753_scatter_rows(const uint64_t* dev_rows, const uint32_t* dev_index, size_t count, size_t row_words, uint64_t* dev_out, size_t n, void* stream) {
  if (row_words == 0 || (row_words & 1u) || row_words > 1024 || count > n || (n && !dev_out) || (count && (!dev_rows || !dev_index)))
    return set_error(MNT753_EINVAL, "scatter_rows: bad argument (rows are an even number of u64 words, count <= n)");
  if (n >= ((size_t)1 << 32)) return set_error(MNT753_EINVAL, "scatter_rows: n must be below 2^32 (32-bit indices)");
  if (!aligned16(dev_rows) || !aligned16(dev_out)) return set_error(MNT753_EINVAL, "scatter_rows: vectors must be 16-byte aligned");
  if (int rc = require_device()) return rc;
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(dev_out, 0, 8 * row_words * n, st));
  if (count == 0) return 0;
  const uint32_t pairs = (uint32_t)(row_words / 2);
  const size_t slice = (size_t)1 << 22;   // rows per launch: the threads of one launch stay far below 2^32
  for (size_t off = 0; off < count; off += slice) {
    const size_t cnt = count - off < slice ? count - off : slice;
    hipLaunchKernelGGL(k_scatter_rows, dim3((unsigned)((cnt * pairs + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const ulonglong2*>(dev_rows) + off * pairs,
                       dev_index + off, cnt, pairs, reinterpret_cast<ulonglong2*>(dev_out));
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int mnt753_batch_exp_sparse(mnt753_fixed_base* fb, const uint64_t* dev_scalars, size_t n, const uint64_t* host_coeff, uint64_t* dev_out_affine,
                            size_t* host_count, void* stream) {
  if (host_count) *host_count = 0;
  if (!fb) return set_error(MNT753_EINVAL, "batch_exp_sparse: null object");
  if (n && (!dev_scalars || !dev_out_affine)) return set_error(MNT753_EINVAL, "batch_exp_sparse: null argument");
  if (int rc = require_device()) return rc;
  if (n == 0) return 0;
  const size_t aw = mnt753_affine_words(fb->curve, fb->group);
  OnDevice on(fb->device);
  hipStream_t st = (hipStream_t)stream;
  Scratch s;
  uint64_t* comp = nullptr;
  uint32_t* idx = nullptr;
  if (!s.alloc(&comp, 96 * n) || !s.alloc(&idx, 4 * n)) return set_error(MNT753_ENOMEM, "batch_exp_sparse: device allocation failed");
  size_t count = 0;
  if (int rc = mnt753_compact_nonzero(dev_scalars, n, comp, idx, &count, stream)) return rc;
  if (host_count) *host_count = count;
  if (count == n) {      // nothing to leave out: the vector as it lies
    if (int rc = mnt753_batch_exp(fb, dev_scalars, 1, n, host_coeff, dev_out_affine, 1, stream)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  }
  uint64_t* rows = nullptr;
  if (count && !s.alloc(&rows, 8 * aw * count)) return set_error(MNT753_ENOMEM, "batch_exp_sparse: device allocation failed");
  if (count)
    if (int rc = mnt753_batch_exp(fb, comp, 1, count, host_coeff, rows, 1, stream)) return rc;
  if (int rc = mnt753_scatter_rows(rows, idx, count, aw, dev_out_affine, n, stream)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

int mnt753_groth16_sizes(const mnt753_r1cs* r, const mnt753_domain* d, mnt753_keygen_sizes* out) {
  if (!r || !d || !out) return set_error(MNT753_EINVAL, "groth16_sizes: null argument");
  const uint64_t m = mnt753_r1cs_num_variables(r), ni = mnt753_r1cs_num_inputs(r), dm = mnt753_domain_size(d);
  if (dm < mnt753_r1cs_domain_size(r)) return set_error(MNT753_EINVAL, "groth16_sizes: domain below constraints + inputs + 1");
  out->a_query = out->b_g1_query = out->b_g2_query = m + 1;
  out->l_query = m - ni;
  out->h_query = dm - 1;
  out->abc_g1 = ni + 1;
  return 0;
}

int mnt753_groth16_generate(mnt753_r1cs* r, mnt753_domain* d, const uint64_t* host_t, const uint64_t* host_alpha, const uint64_t* host_beta,
                            const uint64_t* host_delta, const uint64_t* host_g1_generator, const mnt753_keygen_opts* opts,
                            const mnt753_keygen_out* out, mnt753_keygen_report* report, void* stream) {
  if (!r || !d || !host_t || !host_alpha || !host_beta || !host_delta || !host_g1_generator || !out) return set_error(MNT753_EINVAL, "groth16_generate: null argument");
  if (!out->dev_a_query || !out->dev_b_g1_query || !out->dev_b_g2_query || !out->dev_h_query || !out->dev_abc_g1 || !out->host_alpha_g1 ||
      !out->host_beta_g1 || !out->host_beta_g2 || !out->host_delta_g1 || !out->host_delta_g2)
    return set_error(MNT753_EINVAL, "groth16_generate: null output");
  const int curve = r1cs_curve(r);
  if (domain_curve(d) != curve) return set_error(MNT753_EINVAL, "groth16_generate: the domain belongs to the other curve");
  const size_t m = mnt753_r1cs_num_variables(r), ni = mnt753_r1cs_num_inputs(r), dm = mnt753_domain_size(d);
  if (dm < mnt753_r1cs_domain_size(r)) return set_error(MNT753_EINVAL, "groth16_generate: domain below constraints + inputs + 1");
  if (m > ni && !out->dev_l_query) return set_error(MNT753_EINVAL, "groth16_generate: null output");
  if (m + 1 >= ((size_t)1 << 32) || dm >= ((size_t)1 << 32)) return set_error(MNT753_EINVAL, "groth16_generate: system too large (32-bit indices)");
  const mnt753_keygen_opts zero_opts = {0, 0, 0, 0, 0u, 0u};
  const mnt753_keygen_opts& o = opts ? *opts : zero_opts;
  if (o.flags & ~(MNT753_KEYGEN_DENSE_G1 | MNT753_KEYGEN_DENSE_G2)) return set_error(MNT753_EINVAL, "groth16_generate: unknown flag");
  // the refusals the reference does not make (include/mnt753_hip.h)
  for (const uint64_t* x : {host_t, host_alpha, host_beta, host_delta})
    if (fr_geq_r(curve, x)) return set_error(MNT753_EINVAL, "groth16_generate: t, alpha, beta and delta must be canonical elements of Fr");
  for (const uint64_t* x : {host_alpha, host_beta, host_delta})
    if (words_zero(x, 12)) return set_error(MNT753_EINVAL, "groth16_generate: alpha, beta and delta must not be zero");
  if (int rc = require_device()) return rc;
  int logical = -1;
  const int device = r1cs_device(r, &logical);
  if (mnt753_domain_device(d) != logical) return set_error(MNT753_EINVAL, "groth16_generate: the domain and the system live on different devices");
  uint64_t zt[12];
  if (int rc = mnt753_domain_vanishing_at(d, host_t, zt)) return rc;
  if (words_zero(zt, 12)) return set_error(MNT753_EINVAL, "groth16_generate: Z(t) = 0, t lies in the domain");
  if (words_zero(host_g1_generator + 12, 12)) return set_error(MNT753_EINVAL, "groth16_generate: the G1 generator is the identity");
  OnDevice on(device);
  {
    mnt753_check_report rep;
    if (int rc = mnt753_check_points(curve, MNT753_G1, host_g1_generator, 0, 1, &rep, stream)) return rc;
    if (rep.n_bad) return set_error(MNT753_EINVAL, "groth16_generate: the G1 generator is not a point of the curve in canonical form");
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t w2 = mnt753_affine_words(curve, MNT753_G2);
  // everything that can fail for want of memory or a bad width comes before the system is touched
  Scratch s;
  if (int rc = mnt753_fixed_base_create(curve, MNT753_G1, host_g1_generator, o.g1_window_bits, o.g1_tile, &s.fb[0])) return rc;
  if (int rc = mnt753_fixed_base_create(curve, MNT753_G2, generator_words(curve, MNT753_G2), o.g2_window_bits, o.g2_tile, &s.fb[1])) return rc;
  uint64_t *At = nullptr, *Bt = nullptr, *Ct = nullptr, *Ht = nullptr, *comb = nullptr;
  if (!s.alloc(&At, 96 * (m + 1)) || !s.alloc(&Bt, 96 * (m + 1)) || !s.alloc(&Ct, 96 * (m + 1)) || !s.alloc(&Ht, 96 * (dm + 1)) || !s.alloc(&comb, 96 * (m + 1)))
    return set_error(MNT753_ENOMEM, "groth16_generate: device allocation failed");
  uint64_t dinv[12], h_coeff[12];
  if (curve == MNT753_CURVE_MNT4753) fr_inv_and<frm_of(MNT753_CURVE_MNT4753)>(host_delta, zt, dinv, h_coeff);
  else fr_inv_and<frm_of(MNT753_CURVE_MNT6753)>(host_delta, zt, dinv, h_coeff);

  int swapped = 0;
  if (int rc = mnt753_r1cs_swap_ab_if_beneficial(r, &swapped)) return rc;                                   // :213
  if (report) { report->swapped = swapped; report->non_zero_at = report->non_zero_bt = 0; report->reserved = 0; }
  uint64_t zt2[12];
  if (int rc = mnt753_r1cs_qap_at(r, d, host_t, At, Bt, Ct, Ht, zt2, stream)) return rc;                    // :223
  if (int rc = mnt753_keygen_combine(curve, At, Bt, Ct, m + 1, ni, host_beta, host_alpha, dinv, comb, stream)) return rc;   // :252-274
  // :310-314, on the host while the device works
  if (int rc = scale_affine(curve, MNT753_G1, host_alpha, host_g1_generator, out->host_alpha_g1)) return rc;
  if (int rc = scale_affine(curve, MNT753_G1, host_beta, host_g1_generator, out->host_beta_g1)) return rc;
  if (int rc = scale_affine(curve, MNT753_G2, host_beta, generator_words(curve, MNT753_G2), out->host_beta_g2)) return rc;
  if (int rc = scale_affine(curve, MNT753_G1, host_delta, host_g1_generator, out->host_delta_g1)) return rc;
  if (int rc = scale_affine(curve, MNT753_G2, host_delta, generator_words(curve, MNT753_G2), out->host_delta_g2)) return rc;
  // :318-352.  The densities (:230-244) are the counts of the compactions, or of a count alone where a query walks the vector as it lies
  size_t nz_a = 0, nz_b = 0;
  const bool sparse_g1 = !(o.flags & MNT753_KEYGEN_DENSE_G1), sparse_g2 = !(o.flags & MNT753_KEYGEN_DENSE_G2);
  if (sparse_g1) {
    if (int rc = mnt753_batch_exp_sparse(s.fb[0], At, m + 1, nullptr, out->dev_a_query, &nz_a, stream)) return rc;
    if (int rc = mnt753_batch_exp_sparse(s.fb[0], Bt, m + 1, nullptr, out->dev_b_g1_query, &nz_b, stream)) return rc;
  } else {
    if (int rc = mnt753_compact_nonzero(At, m + 1, nullptr, nullptr, &nz_a, stream)) return rc;
    if (int rc = mnt753_batch_exp(s.fb[0], At, 1, m + 1, nullptr, out->dev_a_query, 1, stream)) return rc;
    if (int rc = mnt753_batch_exp(s.fb[0], Bt, 1, m + 1, nullptr, out->dev_b_g1_query, 1, stream)) return rc;
  }
  if (sparse_g2) {
    if (int rc = mnt753_batch_exp_sparse(s.fb[1], Bt, m + 1, nullptr, out->dev_b_g2_query, &nz_b, stream)) return rc;
  } else {
    if (!sparse_g1)
      if (int rc = mnt753_compact_nonzero(Bt, m + 1, nullptr, nullptr, &nz_b, stream)) return rc;
    if (int rc = mnt753_batch_exp(s.fb[1], Bt, 1, m + 1, nullptr, out->dev_b_g2_query, 1, stream)) return rc;
  }
  if (int rc = mnt753_batch_exp(s.fb[0], comb, 1, ni + 1, nullptr, out->dev_abc_g1, 1, stream)) return rc;
  if (m > ni)
    if (int rc = mnt753_batch_exp(s.fb[0], comb + 12 * (ni + 1), 1, m - ni, nullptr, out->dev_l_query, 1, stream)) return rc;
  if (dm > 1)                                                                                              // :281, :331
    if (int rc = mnt753_batch_exp(s.fb[0], Ht, 1, dm - 1, h_coeff, out->dev_h_query, 1, stream)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (report) { report->non_zero_at = nz_a; report->non_zero_bt = nz_b; }
  return 0;
}

}  // extern "C"
