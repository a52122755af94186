// Witness-map front end: the evaluations of the constraint system on the assignment that
// compute_H starts from.  The reference computes them on the CPU before the prover runs -- libsnark/generate_parameters.cpp:44-57
// writes them into the input file as ca / cb / cc; they are the first loop of r1cs_to_qap_witness_map
// (libsnark/reductions/r1cs_to_qap/r1cs_to_qap.tcc:223-237):
//     ca[i] = <a_i, (1, w)>,  cb[i] = <b_i, (1, w)>,  cc[i] = <c_i, (1, w)>         for the nc constraints
//     ca[nc + i] = (1, w)[i]                                                        for i = 0 .. num_inputs  (input consistency rows)
// and zero above.  Here the constraint system stays on the device as three CSR matrices; the assignment is the vector w of the input
// file (w[0] = 1), so a term with variable index k multiplies w[k].  Built for circuit scale (round 3):
//   * one thread per (matrix, row), rows taken in order of DECREASING length (a work list built once at create time): the 64 rows
//     of a wave have the same number of terms to within one, so ragged systems do not idle lanes behind their longest row;
//   * ONE product per term and none per row: coefficients are stored in the device radix (c R'), the assignment is used as it
//     lies in the file (w R, unpacked to 28-bit limbs with shifts), and mul'(c R', w R) = c w R is already the wire form of the
//     term -- no conversion of w, none of the result (the trick of the NTT twiddles);
//   * terms are summed limb-wise without carries, one normalisation (fp_norm) per two terms, one canonicalisation per row.
// HBM-bound by design: per term 96 B of w gathered + 112 B coefficient + 4 B index, per row 96 B written; bench.py (extras) times a
// 2^20-row system and reports the achieved GB/s.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "common_host.hpp"
#include "host_field.hpp"
#include "msm_kernels.hip.h"
#include "qap_kernels.hip.h"
#include "qap_transpose.hpp"
#include "r1cs_api.hpp"

using namespace mnt753;

struct mnt753_r1cs {
  int curve = 0, frm = 0;
  uint64_t num_inputs = 0, m = 0, nc = 0;
  uint64_t* row_ptr[3] = {nullptr, nullptr, nullptr};   // device, nc + 1 each
  uint32_t* col[3] = {nullptr, nullptr, nullptr};       // device
  uint32_t* coeff[3] = {nullptr, nullptr, nullptr};     // device radix, FPS_WORDS per term
  uint64_t nnz[3] = {0, 0, 0};
  uint64_t* work = nullptr;                             // device, 3 nc items (which * nc + row), longest rows first
  int device = 0, logical_device = 0;                   // physical HIP ordinal / logical device the system lives on (the creating thread's current device)
  // the column-major view of mnt753_r1cs_qap_at (qap_transpose.hpp): built by the first call that needs it, never by the prover path.
  // mutable: the view is a cache of the (const) system, which mnt753_r1cs_qap_plan may have to fill
  mutable std::mutex qap_mutex;
  mutable bool qap_built = false;
  mutable mnt753_qap_plan qap_plan = {};
  mutable uint32_t *qap_perm_row = nullptr, *qap_perm_k = nullptr, *qap_chunk_len = nullptr, *qap_order = nullptr;   // device
  mutable uint64_t *qap_chunk_start = nullptr, *qap_col_chunk = nullptr;                                            // device
  mutable uint32_t* qap_partial = nullptr;              // device, one partial sum (FPS_WORDS) per chunk
  mutable uint64_t qap_base[4] = {0, 0, 0, 0};
  uint32_t* qap_u = nullptr;                            // device, the Lagrange coefficients of the last call's domain (wire form)
  size_t qap_u_cap = 0;
  hipEvent_t qap_free = nullptr;                        // recorded behind every qap_at: the next one (any stream) waits for it before it touches qap_u / qap_partial
  bool ab_swapped = false;                              // a and b stand exchanged relative to creation (mnt753_r1cs_swap_ab_if_beneficial)
};

namespace {
template <int M>
__global__ void __launch_bounds__(256) k_coeff_to_internal(const uint32_t* __restrict__ wire, uint32_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[24];
  load_wire24(w, wire + 24 * i);
  Fp<M> v;
  fp_from_wire(v, w);
  fp_store(out + i * FPS_WORDS, v);
}
// work[t] = which * nc + row for the t-th longest row of the three matrices (rows < nc); threads beyond the list fill the tail of the
// three outputs: rows [nc, nc + num_inputs] of ca copy w, everything else above nc is zero
template <int M>
__global__ void __launch_bounds__(256) k_r1cs_evaluate(const uint64_t* __restrict__ rp_a, const uint32_t* __restrict__ col_a, const uint32_t* __restrict__ cf_a,
                                                      const uint64_t* __restrict__ rp_b, const uint32_t* __restrict__ col_b, const uint32_t* __restrict__ cf_b,
                                                      const uint64_t* __restrict__ rp_c, const uint32_t* __restrict__ col_c, const uint32_t* __restrict__ cf_c,
                                                      const uint64_t* __restrict__ work, const uint32_t* __restrict__ w_wire, uint32_t* __restrict__ ca,
                                                      uint32_t* __restrict__ cb, uint32_t* __restrict__ cc, uint64_t nc, uint64_t num_inputs, uint64_t out_len) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t wv[24];
  if (t >= 3 * nc) {                       // tail rows: t - 3 nc enumerates (which, row - nc)
    const uint64_t u = t - 3 * nc, tail = out_len - nc;
    if (u >= 3 * tail) return;
    const int which = (int)(u / tail);
    const uint64_t row = nc + (u - (uint64_t)which * tail);
    uint32_t* dst = (which == 0 ? ca : (which == 1 ? cb : cc)) + 24 * row;
    if (which == 0 && row <= nc + num_inputs) {
      load_wire24(wv, w_wire + 24 * (row - nc));
    } else {
#pragma unroll
      for (int j = 0; j < 24; ++j) wv[j] = 0;
    }
    store_wire24(dst, wv);
    return;
  }
  const uint64_t item = work[t];
  const int which = (int)(item / nc);
  const uint64_t row = item - (uint64_t)which * nc;
  uint32_t* dst = (which == 0 ? ca : (which == 1 ? cb : cc)) + 24 * row;
  const uint64_t* rp = which == 0 ? rp_a : (which == 1 ? rp_b : rp_c);
  const uint32_t* col = which == 0 ? col_a : (which == 1 ? col_b : col_c);
  const uint32_t* cf = which == 0 ? cf_a : (which == 1 ? cf_b : cf_c);
  // The range of the lazy sum.  c is what k_coeff_to_internal stored (fp_from_wire: < 2r), x a canonical wire integer (< r), so by fp_mul's
  // contract p < r (2r / 2^756 + 1) < 1.2211 r with normalised limbs.  Before an fp_norm the accumulator holds a flushed value
  // (< 1.51 r) and two products: < 3.9522 r, limbs < 3 2^28, |q| <= 3 -- inside fp_norm's contract (|value| < 5 r, |limb| + 2^28 |q| <
  // 2^31 - 2^4).  tools/host_r1cs_check.cpp is this loop compiled for the host -- THE TWO MIRROR EACH OTHER, change them together -- and
  // asserts those bounds after every step on every pair of the designed operands of tests/r1cs_designed.py; the largest it saw:
  // product 1.027 r (MNT4753) / 1.103 r (MNT6753), accumulator before fp_norm 3.443 r / 3.372 r, limb 3.000 2^28, |q| 2.
  Fp<M> acc, c, x, p;
  fp_zero(acc);
  uint32_t pending = 0;
  for (uint64_t k = rp[row]; k < rp[row + 1]; ++k) {
    load_wire24(wv, w_wire + 24 * (size_t)col[k]);
    fp_unpack(x, wv);                      // w R as an integer < r, 28-bit limbs
    fp_load(c, cf + k * FPS_WORDS);        // c R'
    fp_mul(p, c, x);                       // c w R, lazily in [0, 1.2211 r)
#pragma unroll
    for (int i = 0; i < NL; ++i) acc.l[i] += p.l[i];
    if (++pending == 2u) { fp_norm(acc, acc); pending = 0; }   // value < 1.51 r + 2 * 1.2211 r: inside fp_norm's range
  }
  if (pending) fp_norm(acc, acc);
  Fp<M> canon;
  fp_canon(canon, acc);
  fp_pack(wv, canon);
  store_wire24(dst, wv);
}
// a and b change roles in the work list: item which * nc + row of a becomes b's and the reverse; the order by length stays valid
__global__ void __launch_bounds__(256) k_r1cs_work_swap_ab(uint64_t* __restrict__ work, uint64_t nc) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * nc) return;
  const uint64_t item = work[t];
  if (item < nc) work[t] = item + nc;
  else if (item < 2 * nc) work[t] = item - nc;
}
// the column-major view, once per system: the row-major index arrays come back from the device (mnt753_r1cs_create keeps no host
// copy: a prover pays nothing for this), the permutation is built on the host and uploaded
int qap_prepare(const mnt753_r1cs* r) {
  OnDevice on(r->device);
  std::lock_guard<std::mutex> lock(r->qap_mutex);
  if (r->qap_built) return 0;
  std::vector<uint64_t> rp[3];
  std::vector<uint32_t> cl[3];
  const uint64_t* rpp[3];
  const uint32_t* clp[3];
  for (int k = 0; k < 3; ++k) {
    rp[k].resize(r->nc + 1);
    cl[k].resize(r->nnz[k] + 1);
    HIP_TRY(hipMemcpy(rp[k].data(), r->row_ptr[k], 8 * (r->nc + 1), hipMemcpyDeviceToHost));
    if (r->nnz[k]) HIP_TRY(hipMemcpy(cl[k].data(), r->col[k], 4 * r->nnz[k], hipMemcpyDeviceToHost));
    rpp[k] = rp[k].data();
    clp[k] = cl[k].data();
  }
  QapTranspose tr;
  if (!qap_build_transpose(r->nc, r->m + 1, rpp, clp, QAP_CHUNK_TERMS, tr)) return set_error(MNT753_EINVAL, "r1cs_qap_at: the system is too large for 32-bit term indices");
  const size_t n_chunks = tr.order.size(), total = tr.perm_row.size();
  auto up = [](auto** dst, const auto& v) -> hipError_t {
    typedef typename std::remove_reference<decltype(v[0])>::type T;
    hipError_t e = hipMalloc(dst, sizeof(T) * (v.size() + 1));
    if (e == hipSuccess && !v.empty()) e = hipMemcpy(*dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
    return e;
  };
  hipError_t e = up(&r->qap_perm_row, tr.perm_row);
  if (e == hipSuccess) e = up(&r->qap_perm_k, tr.perm_k);
  if (e == hipSuccess) e = up(&r->qap_chunk_start, tr.chunk_start);
  if (e == hipSuccess) e = up(&r->qap_chunk_len, tr.chunk_len);
  if (e == hipSuccess) e = up(&r->qap_col_chunk, tr.col_chunk);
  if (e == hipSuccess) e = up(&r->qap_order, tr.order);
  if (e == hipSuccess) e = hipMalloc(&r->qap_partial, 4 * FPS_WORDS * (n_chunks + 1));
  if (e != hipSuccess) {
    void** qap[] = {(void**)&r->qap_perm_row, (void**)&r->qap_perm_k, (void**)&r->qap_chunk_len, (void**)&r->qap_order, (void**)&r->qap_chunk_start,
                    (void**)&r->qap_col_chunk, (void**)&r->qap_partial};
    for (void** p : qap) { if (*p) (void)hipFree(*p); *p = nullptr; }
    return set_hip_error(e, "r1cs_qap_at: column-major view", __FILE__, __LINE__);
  }
  for (int k = 0; k < 4; ++k) r->qap_base[k] = tr.base[k];
  r->qap_plan.chunk_terms = tr.L;
  r->qap_plan.terms = total;
  r->qap_plan.work_items = n_chunks;
  r->qap_plan.split_columns = tr.split_columns;
  r->qap_plan.longest_column = tr.longest_column;
  r->qap_plan.transpose_bytes = tr.device_bytes();
  r->qap_plan.partial_bytes = 4 * FPS_WORDS * n_chunks;
  r->qap_built = true;
  return 0;
}
}  // namespace

namespace mnt753 {
int r1cs_curve(const mnt753_r1cs* r) { return r ? r->curve : -1; }
int r1cs_device(const mnt753_r1cs* r, int* logical) {
  if (logical) *logical = r ? r->logical_device : -1;
  return r ? r->device : -1;
}
}  // namespace mnt753

extern "C" {

int mnt753_r1cs_create(int curve, uint64_t num_inputs, uint64_t m, uint64_t nc, const uint64_t* const row_ptr[3], const uint32_t* const col[3],
                       const uint64_t* const coeff[3], mnt753_r1cs** out) {
  if (curve < 0 || curve > 1 || !out || !row_ptr || !col || !coeff) return set_error(MNT753_EINVAL, "r1cs_create: bad argument");
  if (int rc = require_device()) return rc;
  if (num_inputs > m) return set_error(MNT753_EINVAL, "r1cs_create: more inputs than variables");
  for (int k = 0; k < 3; ++k) {
    if (!row_ptr[k] || row_ptr[k][0] != 0) return set_error(MNT753_EINVAL, "r1cs_create: row_ptr must start at 0");
    for (uint64_t i = 0; i < nc; ++i)
      if (row_ptr[k][i + 1] < row_ptr[k][i]) return set_error(MNT753_EINVAL, "r1cs_create: row_ptr not monotone");
    const uint64_t nnz = row_ptr[k][nc];
    if (nnz && (!col[k] || !coeff[k])) return set_error(MNT753_EINVAL, "r1cs_create: null matrix");
    for (uint64_t i = 0; i < nnz; ++i)
      if (col[k][i] > m) return set_error(MNT753_EINVAL, "r1cs_create: variable index out of range");
  }
  mnt753_r1cs* r = new (std::nothrow) mnt753_r1cs();
  if (!r) return set_error(MNT753_ENOMEM, "r1cs_create: host allocation failed");
  r->curve = curve; r->frm = curve == MNT753_CURVE_MNT4753 ? MOD_A : MOD_B;
  r->num_inputs = num_inputs; r->m = m; r->nc = nc;
  r->device = current_physical_device(); r->logical_device = mnt753_get_device();
  for (int k = 0; k < 3; ++k) {
    const uint64_t nnz = row_ptr[k][nc];
    r->nnz[k] = nnz;
    uint32_t* staged = nullptr;
    if (hipMalloc(&r->row_ptr[k], 8 * (nc + 1)) != hipSuccess || hipMalloc(&r->col[k], 4 * (nnz + 1)) != hipSuccess ||
        hipMalloc(&r->coeff[k], 4 * FPS_WORDS * (nnz + 1)) != hipSuccess || hipMalloc(&staged, 96 * (nnz + 1)) != hipSuccess) {
      (void)hipGetLastError();
      mnt753_r1cs_free(r);
      return set_error(MNT753_ENOMEM, "r1cs_create: device allocation failed");
    }
    // any failure below frees the staging buffer and the partly built system before it returns
    hipError_t e = hipMemcpy(r->row_ptr[k], row_ptr[k], 8 * (nc + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) {
      e = hipMemcpy(r->col[k], col[k], 4 * nnz, hipMemcpyHostToDevice);
      if (e == hipSuccess) e = hipMemcpy(staged, coeff[k], 96 * nnz, hipMemcpyHostToDevice);
      if (e == hipSuccess) {
        const unsigned g = (unsigned)((nnz + 255) / 256);
        if (r->frm == MOD_A) hipLaunchKernelGGL((k_coeff_to_internal<MOD_A>), dim3(g), dim3(256), 0, 0, staged, r->coeff[k], (size_t)nnz);
        else hipLaunchKernelGGL((k_coeff_to_internal<MOD_B>), dim3(g), dim3(256), 0, 0, staged, r->coeff[k], (size_t)nnz);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
      }
    }
    (void)hipFree(staged);
    if (e != hipSuccess) {
      mnt753_r1cs_free(r);
      return set_hip_error(e, "r1cs_create: upload / conversion", __FILE__, __LINE__);
    }
  }
  // work list: the rows of the three matrices by decreasing number of terms (counting sort over the lengths: O(rows))
  {
    std::vector<uint64_t> order((size_t)3 * nc);
    uint64_t longest = 0;
    for (int k = 0; k < 3; ++k) for (uint64_t i = 0; i < nc; ++i) longest = std::max(longest, row_ptr[k][i + 1] - row_ptr[k][i]);
    std::vector<uint64_t> start(longest + 2, 0);
    for (int k = 0; k < 3; ++k) for (uint64_t i = 0; i < nc; ++i) ++start[longest - (row_ptr[k][i + 1] - row_ptr[k][i]) + 1];
    for (uint64_t l = 1; l <= longest + 1; ++l) start[l] += start[l - 1];
    for (int k = 0; k < 3; ++k) for (uint64_t i = 0; i < nc; ++i) order[start[longest - (row_ptr[k][i + 1] - row_ptr[k][i])]++] = (uint64_t)k * nc + i;
    hipError_t e = hipMalloc(&r->work, 8 * ((size_t)3 * nc + 1));
    if (e == hipSuccess && nc) e = hipMemcpy(r->work, order.data(), 8 * (size_t)3 * nc, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      mnt753_r1cs_free(r);
      return set_hip_error(e, "r1cs_create: work list", __FILE__, __LINE__);
    }
  }
  *out = r;
  return 0;
}

int mnt753_r1cs_free(mnt753_r1cs* r) {
  if (!r) return 0;
  if (r->work) (void)hipFree(r->work);
  void* qap[] = {r->qap_perm_row, r->qap_perm_k, r->qap_chunk_len, r->qap_order, r->qap_chunk_start, r->qap_col_chunk, r->qap_partial, r->qap_u};
  for (void* p : qap) if (p) (void)hipFree(p);
  if (r->qap_free) (void)hipEventDestroy(r->qap_free);
  for (int k = 0; k < 3; ++k) {
    if (r->row_ptr[k]) (void)hipFree(r->row_ptr[k]);
    if (r->col[k]) (void)hipFree(r->col[k]);
    if (r->coeff[k]) (void)hipFree(r->coeff[k]);
  }
  delete r;
  return 0;
}

size_t mnt753_r1cs_domain_size(const mnt753_r1cs* r) { return r ? (size_t)(r->nc + r->num_inputs + 1) : 0; }
size_t mnt753_r1cs_num_variables(const mnt753_r1cs* r) { return r ? (size_t)r->m : 0; }
size_t mnt753_r1cs_num_inputs(const mnt753_r1cs* r) { return r ? (size_t)r->num_inputs : 0; }

int mnt753_r1cs_evaluate(mnt753_r1cs* r, const uint64_t* dev_w, uint64_t* dev_ca, uint64_t* dev_cb, uint64_t* dev_cc, size_t out_len, void* stream) {
  if (!r || !dev_w || !dev_ca || !dev_cb || !dev_cc) return set_error(MNT753_EINVAL, "r1cs_evaluate: null argument");
  if (out_len < r->nc + r->num_inputs + 1) return set_error(MNT753_EINVAL, "r1cs_evaluate: out_len below constraints + inputs + 1");
  if (int rc = require_device()) return rc;
  const unsigned g = (unsigned)((3 * (uint64_t)out_len + 255) / 256);   // 3 nc work items + 3 (out_len - nc) tail rows
  const uint32_t* w = reinterpret_cast<const uint32_t*>(dev_w);
  uint32_t *a = reinterpret_cast<uint32_t*>(dev_ca), *b = reinterpret_cast<uint32_t*>(dev_cb), *c = reinterpret_cast<uint32_t*>(dev_cc);
  if (r->frm == MOD_A)
    hipLaunchKernelGGL((k_r1cs_evaluate<MOD_A>), dim3(g), dim3(256), 0, (hipStream_t)stream, r->row_ptr[0], r->col[0], r->coeff[0], r->row_ptr[1], r->col[1],
                       r->coeff[1], r->row_ptr[2], r->col[2], r->coeff[2], r->work, w, a, b, c, r->nc, r->num_inputs, (uint64_t)out_len);
  else
    hipLaunchKernelGGL((k_r1cs_evaluate<MOD_B>), dim3(g), dim3(256), 0, (hipStream_t)stream, r->row_ptr[0], r->col[0], r->coeff[0], r->row_ptr[1], r->col[1],
                       r->coeff[1], r->row_ptr[2], r->col[2], r->coeff[2], r->work, w, a, b, c, r->nc, r->num_inputs, (uint64_t)out_len);
  HIP_TRY(hipGetLastError());
  return 0;
}

// cs.is_satisfied (r1cs_to_qap.tcc:216): the evaluation above into scratch vectors of nc + num_inputs + 1 entries, then the row check
// of csrc/mnt753_validate.hip on them.  The rows behind the constraints hold (w_i, 0, 0) and pass, so a bad index is a constraint row.
int mnt753_r1cs_check(mnt753_r1cs* r, const uint64_t* dev_w, mnt753_check_report* out, void* stream) {
  if (!r || !dev_w || !out) return set_error(MNT753_EINVAL, "r1cs_check: null argument");
  if (int rc = require_device()) return rc;
  const size_t n = (size_t)(r->nc + r->num_inputs + 1);
  uint64_t* scratch = nullptr;
  if (hipMalloc(&scratch, 3 * 96 * n) != hipSuccess) { (void)hipGetLastError(); return set_error(MNT753_ENOMEM, "r1cs_check: device allocation failed"); }
  int rc = mnt753_r1cs_evaluate(r, dev_w, scratch, scratch + 12 * n, scratch + 24 * n, n, stream);
  if (rc == 0) rc = mnt753_check_products(r->curve, scratch, scratch + 12 * n, scratch + 24 * n, n, out, stream);
  (void)hipFree(scratch);
  return rc;
}

// swap_AB_if_beneficial (r1cs.tcc:194-243)
int mnt753_r1cs_swap_ab_if_beneficial(mnt753_r1cs* r, int* swapped) {
  if (swapped) *swapped = 0;
  if (!r) return set_error(MNT753_EINVAL, "r1cs_swap_ab_if_beneficial: null argument");
  if (int rc = require_device()) return rc;
  OnDevice on(r->device);
  // r1cs.tcc:199-219: the variables a term of a / of b names, whatever its coefficient
  uint64_t touched[2] = {0, 0};
  {
    std::vector<uint8_t> seen;
    std::vector<uint32_t> cl;
    HIP_TRY(hipDeviceSynchronize());     // the arrays may be in use by work enqueued on any stream
    for (int k = 0; k < 2; ++k) {
      seen.assign(r->m + 1, 0);
      cl.resize(r->nnz[k] + 1);
      if (r->nnz[k]) HIP_TRY(hipMemcpy(cl.data(), r->col[k], 4 * r->nnz[k], hipMemcpyDeviceToHost));
      for (uint64_t i = 0; i < r->nnz[k]; ++i) seen[cl[i]] = 1;
      for (uint8_t v : seen) touched[k] += v;
    }
  }
  if (touched[1] <= touched[0]) return 0;       // :228: strictly more
  if (r->nc) {
    hipLaunchKernelGGL(k_r1cs_work_swap_ab, dim3((unsigned)((3 * r->nc + 255) / 256)), dim3(256), 0, 0, r->work, r->nc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  std::swap(r->row_ptr[0], r->row_ptr[1]);
  std::swap(r->col[0], r->col[1]);
  std::swap(r->coeff[0], r->coeff[1]);
  std::swap(r->nnz[0], r->nnz[1]);
  r->ab_swapped = !r->ab_swapped;
  {
    // the column-major view lists a's terms in front of b's: the next mnt753_r1cs_qap_at builds it again
    std::lock_guard<std::mutex> lock(r->qap_mutex);
    if (r->qap_built) {
      void** qap[] = {(void**)&r->qap_perm_row, (void**)&r->qap_perm_k, (void**)&r->qap_chunk_len, (void**)&r->qap_order, (void**)&r->qap_chunk_start,
                      (void**)&r->qap_col_chunk, (void**)&r->qap_partial};
      for (void** p : qap) { if (*p) (void)hipFree(*p); *p = nullptr; }
      r->qap_built = false;
    }
  }
  if (swapped) *swapped = 1;
  return 0;
}

int mnt753_r1cs_is_swapped(const mnt753_r1cs* r) { return r && r->ab_swapped ? 1 : 0; }

int mnt753_r1cs_qap_plan(const mnt753_r1cs* r, mnt753_qap_plan* out) {
  if (!r || !out) return set_error(MNT753_EINVAL, "r1cs_qap_plan: null argument");
  if (int rc = require_device()) return rc;
  if (int rc = qap_prepare(r)) return rc;
  *out = r->qap_plan;
  return 0;
}

// r1cs_to_qap_instance_map_with_evaluation (r1cs_to_qap.tcc:110-159) on the device
int mnt753_r1cs_qap_at(mnt753_r1cs* r, mnt753_domain* d, const uint64_t* host_t, uint64_t* dev_At, uint64_t* dev_Bt, uint64_t* dev_Ct, uint64_t* dev_Ht,
                       uint64_t* host_Zt, void* stream) {
  if (!r || !d || !host_t || !dev_At || !dev_Bt || !dev_Ct || !dev_Ht || !host_Zt) return set_error(MNT753_EINVAL, "r1cs_qap_at: null argument");
  if (domain_curve(d) != r->curve) return set_error(MNT753_EINVAL, "r1cs_qap_at: the domain belongs to the other curve");
  const size_t dm = mnt753_domain_size(d);
  if (dm < r->nc + r->num_inputs + 1) return set_error(MNT753_EINVAL, "r1cs_qap_at: domain below constraints + inputs + 1");
  if (r->frm == MOD_A ? host::HFp<MOD_A>::geq_p(host_t) : host::HFp<MOD_B>::geq_p(host_t)) return set_error(MNT753_EINVAL, "r1cs_qap_at: t is not a canonical element of Fr");
  if (int rc = require_device()) return rc;
  if (mnt753_domain_device(d) != r->logical_device) return set_error(MNT753_EINVAL, "r1cs_qap_at: the domain and the system live on different devices");
  if (int rc = qap_prepare(r)) return rc;
  OnDevice on(r->device);
  hipStream_t st = (hipStream_t)stream;
  // qap_u and qap_partial are shared by the calls on this system: a call on another stream starts behind the previous one
  if (!r->qap_free) HIP_TRY(hipEventCreateWithFlags(&r->qap_free, hipEventDisableTiming));
  else HIP_TRY(hipStreamWaitEvent(st, r->qap_free, 0));
  if (r->qap_u_cap < dm) {
    if (r->qap_u) (void)hipFree(r->qap_u);
    r->qap_u = nullptr; r->qap_u_cap = 0;
    if (hipMalloc(&r->qap_u, 96 * dm) != hipSuccess) { (void)hipGetLastError(); r->qap_u = nullptr; return set_error(MNT753_ENOMEM, "r1cs_qap_at: device allocation failed"); }
    r->qap_u_cap = dm;
  }
  uint64_t zt[12];
  if (int rc = mnt753_domain_vanishing_at(d, host_t, zt)) return rc;
  if (int rc = mnt753_domain_lagrange_at(d, host_t, reinterpret_cast<uint64_t*>(r->qap_u), stream)) return rc;
  if (int rc = mnt753_vec_powers(r->curve, host_t, dev_Ht, dm + 1, stream)) return rc;
  const uint64_t n_chunks = r->qap_plan.work_items, ncols = r->m + 1;
  const QapMatrices mats = {{r->coeff[0], r->coeff[1], r->coeff[2]}, r->qap_base[1], r->qap_base[2]};
  uint32_t *at = reinterpret_cast<uint32_t*>(dev_At), *bt = reinterpret_cast<uint32_t*>(dev_Bt), *ct = reinterpret_cast<uint32_t*>(dev_Ct);
  const unsigned gc = (unsigned)((n_chunks + 255) / 256), gf = (unsigned)((3 * ncols + 255) / 256);
  if (r->frm == MOD_A) {
    if (n_chunks) hipLaunchKernelGGL((k_qap_chunks<MOD_A>), dim3(gc), dim3(256), 0, st, mats, r->qap_perm_row, r->qap_perm_k, r->qap_chunk_start, r->qap_chunk_len, r->qap_order, r->qap_u, r->qap_partial, n_chunks);
    hipLaunchKernelGGL((k_qap_fold<MOD_A>), dim3(gf), dim3(256), 0, st, r->qap_partial, r->qap_col_chunk, r->qap_u, at, bt, ct, ncols, r->nc, r->num_inputs);
  } else {
    if (n_chunks) hipLaunchKernelGGL((k_qap_chunks<MOD_B>), dim3(gc), dim3(256), 0, st, mats, r->qap_perm_row, r->qap_perm_k, r->qap_chunk_start, r->qap_chunk_len, r->qap_order, r->qap_u, r->qap_partial, n_chunks);
    hipLaunchKernelGGL((k_qap_fold<MOD_B>), dim3(gf), dim3(256), 0, st, r->qap_partial, r->qap_col_chunk, r->qap_u, at, bt, ct, ncols, r->nc, r->num_inputs);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(r->qap_free, st));
  memcpy(host_Zt, zt, 96);
  return 0;
}

}  // extern "C"
