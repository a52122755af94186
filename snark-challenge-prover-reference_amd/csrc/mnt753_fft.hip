// FFT part of the C ABI (include/mnt753_hip.h): evaluation domains, the four transform kinds,
// divide_by_Z_on_coset, the element-wise vector ops and the device-resident compute_H.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>
#include <sys/random.h>

#include "common_host.hpp"
#include "host_field.hpp"
#include "ntt_kernels.hip.h"
#include "qap_kernels.hip.h"
#include "reduce_kernels.hip.h"
#include "reduce_api.hpp"

using namespace mnt753;
using namespace mnt753::host;

struct mnt753_domain {
  int curve = 0, frm = 0;
  int device = 0, logical_device = 0;                  // physical HIP ordinal / logical device the tables live on (the creating thread's current device)
  size_t m = 0;
  int logm = 0;
  uint32_t *tw_fwd = nullptr, *tw_inv = nullptr;       // omega^i, omega^-i            (m/2 each)
  uint32_t *cos_fwd = nullptr;                         // g^i                         (m)
  uint32_t *cos_fwd_s = nullptr;                       // g^i / m                     (m)  iFFT scale fused with the coset shift
  uint32_t *cos_inv_s = nullptr;                       // g^-i / m                    (m)
  uint32_t *consts = nullptr;                          // [0] 1/m  [1] 2^12 (k1)  [2] Z^-1 * 2^-12 (k2)  [3] Z^-1
  uint32_t *work = nullptr;                            // m wire elements
  hipEvent_t work_free = nullptr;                      // recorded after every transform: the next user of `work` (any stream) waits for it
  uint32_t *stage = nullptr;                           // the seeds the tables were generated from (freed with the domain:
                                                       // hipFree is a device-wide sync and would wait for MSMs in flight)
  // step (m = big_m + small_m) and extended (m = 2 small_m, big_m = small_m) domains: two inner basic domains and the tables of
  // the passes around them (ntt_kernels.hip.h).  Of the fields above they use m, work, work_free and stage only.
  int kind = MNT753_DOMAIN_BASIC;
  size_t big_m = 0, small_m = 0;
  mnt753_domain *sub_big = nullptr, *sub_small = nullptr;   // sizes big_m and small_m (sub_small: null where small_m is 1; extended: both the same object)
  uint32_t *x_fwd = nullptr;                           // step: omega^k (big_m)                 extended: shift^i (small_m)
  uint32_t *x_inv = nullptr;                           // step: omega^k / (2 big_m) (big_m)     extended: sconst shift^-i (small_m)
  uint32_t *x_inv2 = nullptr;                          // step: omega^-i (small_m)
  uint32_t *xcos_fwd = nullptr, *xcos_inv = nullptr;   // g^k, g^-k (m each)
  uint32_t *xconsts = nullptr;                         // step: 1/(2 big_m), 1/(2 small_m), 1/big_m, 2^12    extended: shift^s, sconst, -, 2^12
  uint32_t *zt = nullptr, *zt12 = nullptr;             // 1/Z on the coset and 2^-12 times it: z_mask + 2 entries each (z_index)
  size_t z_split = 0, z_mask = 0;
  // mixed-radix domain (m = q_n t_n, q_n = 5^q_pow, t_n a power of two): sub_big is the inner basic domain of size t_n (null where
  // t_n is 1).  x_fwd / x_inv: omega^k / omega^-k (m each), xcos_fwd / xcos_inv as above, xconsts: zeta^e, zeta^-e, zeta^-e / m
  // (e < 5 each), consts as in a basic domain (Z is one constant).  The step / extended fields above stay unused.
  unsigned q_n = 0, q_pow = 0;
  size_t t_n = 0;
  uint32_t *lag_pre = nullptr;                         // mnt753_domain_lagrange_at: the prefix products of its inversion runs (m entries), allocated by the first call
};

namespace {

// inner: the domain serves a step or extended domain, which brings its own coset tables
template <int M>
int build_tables(mnt753_domain* d, bool inner = false) {
  typedef HFp<M> Fr;
  const size_t m = d->m;
  const int logm = d->logm;
  // omega: primitive m-th root = (2^s-th root)^(2^(s-logm))   (libff get_root_of_unity, field_utils.tcc:40-89)
  Fr omega = Fr::from_words(FRD[M].root_of_unity);
  for (int i = FRD[M].two_adicity; i > logm; --i) omega = omega.squared();
  Fr omega_inv = omega.inverse();
  Fr g = Fr::from_words(FRD[M].mult_gen), g_inv = g.inverse();
  Fr minv = Fr::from_uint((uint64_t)m).inverse();
  Fr z = g.pow_u64((uint64_t)m) - Fr::one();     // vanishing polynomial on the coset, basic_radix2_domain.tcc:113-116
  Fr zinv = z.inverse();
  Fr two12 = Fr::from_uint(4096), two12_inv = two12.inverse();

  // staging buffer (host): 4 power tables of 32 entries + 4 scales + 4 constants, all wire form
  std::vector<uint64_t> stage((4 * 32 + 4 + 4) * 12);
  auto put = [&](size_t slot, const Fr& v) { memcpy(&stage[slot * 12], v.l, 96); };
  const Fr bases[4] = {omega, omega_inv, g, g_inv};
  for (int t = 0; t < 4; ++t) {
    Fr p = bases[t];
    for (int k = 0; k < 32; ++k) { put(t * 32 + k, p); p = p.squared(); }
  }
  put(128, Fr::one()); put(129, minv);                   // scales
  put(132, minv); put(133, two12); put(134, zinv * two12_inv); put(135, zinv);
  HIP_TRY(hipMalloc(&d->stage, stage.size() * 8));
  uint32_t* d_stage = d->stage;
  HIP_TRY(hipMemcpy(d_stage, stage.data(), stage.size() * 8, hipMemcpyHostToDevice));
  const size_t half = m / 2 ? m / 2 : 1;
  HIP_TRY(hipMalloc(&d->tw_fwd, half * FPS_WORDS * 4));
  HIP_TRY(hipMalloc(&d->tw_inv, half * FPS_WORDS * 4));
  if (!inner) {
    HIP_TRY(hipMalloc(&d->cos_fwd, m * FPS_WORDS * 4));
    HIP_TRY(hipMalloc(&d->cos_fwd_s, m * FPS_WORDS * 4));
    HIP_TRY(hipMalloc(&d->cos_inv_s, m * FPS_WORDS * 4));
  }
  HIP_TRY(hipMalloc(&d->consts, 4 * FPS_WORDS * 4));
  HIP_TRY(hipMalloc(&d->work, m * 96));
  auto table = [&](uint32_t* out, int base_slot, int scale_slot, size_t n) {
    hipLaunchKernelGGL((k_pow_table<M>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, out, d_stage + (size_t)base_slot * 32 * 24,
                       d_stage + (size_t)scale_slot * 24, n, logm);
  };
  table(d->tw_fwd, 0, 128, half);
  table(d->tw_inv, 1, 128, half);
  if (!inner) {
    table(d->cos_fwd, 2, 128, m);
    table(d->cos_fwd_s, 2, 129, m);
    table(d->cos_inv_s, 3, 129, m);
  }
  hipLaunchKernelGGL((k_consts_to_internal<M>), dim3(1), dim3(64), 0, 0, d->consts, d_stage + (size_t)132 * 24, 4);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));   // the tables are built on the default stream; MSM streams are not waited for
  return 0;
}

// bit-reversal + log2 m butterfly stages, in place on `vec` (via the domain's work buffer)
// in_scale / out_scale: tables the elements are multiplied by on the way into the first group / out of the last (k_ntt_group)
// (from / vec: the transform reads `from` and leaves its result in `vec`; they are the same vector or do not overlap)
template <int M>
int run_stages(mnt753_domain* d, const uint32_t* from, uint32_t* vec, const uint32_t* tw, hipStream_t st, const uint32_t* in_scale = nullptr, const uint32_t* out_scale = nullptr) {
  const int logm = d->logm;
  const bool in_place = from == vec;
  if (logm == 0) return 0;
  int n_groups = (logm + NTT_MAX_NS - 1) / NTT_MAX_NS;
  int s0 = 0;
  for (int gi = 0; gi < n_groups; ++gi) {
    int ns = (logm - s0 + (n_groups - gi) - 1) / (n_groups - gi);   // balanced split
    const uint32_t* src = gi == 0 ? from : d->work;
    uint32_t* dst = (gi == n_groups - 1 && (n_groups > 1 || !in_place)) ? vec : d->work;
    const size_t n_tiles = (size_t)1 << (logm - ns);
    const int tiles_per_block = NTT_BLOCK / (1 << (ns - 1));
    const unsigned blocks = (unsigned)((n_tiles + tiles_per_block - 1) / tiles_per_block);
    const uint32_t* is = gi == 0 ? in_scale : nullptr;
    const uint32_t* os = gi == n_groups - 1 ? out_scale : nullptr;
    const int bitrev = gi == 0 ? 1 : 0;
    // (no transform of the path scales on both sides: callers pass in_scale or out_scale, never both)
    if (is && os) return set_error(MNT753_EINVAL, "ntt: a transform scales on the way in or on the way out, not both");
    else if (is) hipLaunchKernelGGL((k_ntt_group<M, true, false>), dim3(blocks), dim3(NTT_BLOCK), 0, st, src, dst, tw, logm, s0, ns, bitrev, is, os);
    else if (os) hipLaunchKernelGGL((k_ntt_group<M, false, true>), dim3(blocks), dim3(NTT_BLOCK), 0, st, src, dst, tw, logm, s0, ns, bitrev, is, os);
    else hipLaunchKernelGGL((k_ntt_group<M, false, false>), dim3(blocks), dim3(NTT_BLOCK), 0, st, src, dst, tw, logm, s0, ns, bitrev, is, os);
    s0 += ns;
  }
  if (n_groups == 1 && in_place) HIP_TRY(hipMemcpyAsync(vec, d->work, d->m * 96, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- step and extended domains: the passes of ntt_kernels.hip.h around the inner transforms --------------------------------------
struct StepGrid { unsigned blocks, threads; int ti_n, tj_n; };
// k_step_pre / k_step_post: ti_n = min(small_m, 64) outputs per block, tj_n = min(compr, 256 / ti_n) partial sums per output
inline StepGrid step_grid(const mnt753_domain* d) {
  const size_t compr = d->big_m / d->small_m;
  const int ti_n = (int)(d->small_m < 64 ? d->small_m : 64);
  const int tj_n = (int)(compr < (size_t)(256 / ti_n) ? compr : (size_t)(256 / ti_n));
  return StepGrid{(unsigned)(d->small_m / ti_n), (unsigned)(ti_n * tj_n), ti_n, tj_n};
}
// the two inner transforms, from one buffer into the other (a size-1 transform is a copy)
template <int M>
int x_inner(mnt753_domain* d, const uint32_t* from, uint32_t* to, bool inverse, hipStream_t st) {
  mnt753_domain *b = d->sub_big, *sm = d->sub_small;
  if (int rc = run_stages<M>(b, from, to, inverse ? b->tw_inv : b->tw_fwd, st)) return rc;
  if (sm) return run_stages<M>(sm, from + d->big_m * 24, to + d->big_m * 24, inverse ? sm->tw_inv : sm->tw_fwd, st);
  HIP_TRY(hipMemcpyAsync(to + d->big_m * 24, from + d->big_m * 24, 96, hipMemcpyDeviceToDevice, st));
  return 0;
}
// mixed-radix domain, all four kinds: digit split (out of place, vec -> work), q_n inner radix-2 transforms (work -> vec), q_pow
// radix-5 levels in place on vec (ntt_kernels.hip.h).  The inverse is the same schedule over omega^-1; its 1 / m rides on the last
// level's constants and icosetFFT's g^-k on that level's stores.
template <int M>
int mixed_transform(mnt753_domain* d, uint32_t* vec, bool inverse, bool coset, hipStream_t st) {
  const size_t m = d->m, t_n = d->t_n;
  const unsigned gb = (unsigned)((m + 255) / 256);
  if (coset && !inverse) hipLaunchKernelGGL((k_mixed_pre<M, true>), dim3(gb), dim3(256), 0, st, vec, d->work, d->xcos_fwd, m, d->q_n, t_n);
  else hipLaunchKernelGGL((k_mixed_pre<M, false>), dim3(gb), dim3(256), 0, st, vec, d->work, d->xcos_fwd, m, d->q_n, t_n);
  HIP_TRY(hipGetLastError());
  if (mnt753_domain* in = d->sub_big) {
    for (unsigned s = 0; s < d->q_n; ++s)
      if (int rc = run_stages<M>(in, d->work + s * t_n * 24, vec + s * t_n * 24, inverse ? in->tw_inv : in->tw_fwd, st)) return rc;
  } else {
    HIP_TRY(hipMemcpyAsync(vec, d->work, m * 96, hipMemcpyDeviceToDevice, st));      // t_n == 1: the inner transforms are the identity
  }
  const size_t n_cols = m / 5;
  const unsigned blocks = (unsigned)((n_cols + R5_COLS - 1) / R5_COLS);
  const uint32_t* tw = inverse ? d->x_inv : d->x_fwd;
  size_t width = t_n;
  for (unsigned lvl = 0; lvl < d->q_pow; ++lvl, width *= 5) {
    const bool last = lvl + 1 == d->q_pow;
    const size_t tw_stride = m / (5 * width);
    if (inverse && last) {
      const uint32_t* zc = d->xconsts + 10 * FPS_WORDS;
      if (coset) hipLaunchKernelGGL((k_radix5_merge<M, true, true>), dim3(blocks), dim3(R5_BLOCK), 0, st, vec, tw, zc, d->xcos_inv, n_cols, width, tw_stride);
      else hipLaunchKernelGGL((k_radix5_merge<M, true, false>), dim3(blocks), dim3(R5_BLOCK), 0, st, vec, tw, zc, d->xcos_inv, n_cols, width, tw_stride);
    } else {
      const uint32_t* zc = d->xconsts + (inverse ? 5 : 0) * FPS_WORDS;
      hipLaunchKernelGGL((k_radix5_merge<M, false, false>), dim3(blocks), dim3(R5_BLOCK), 0, st, vec, tw, zc, d->xcos_inv, n_cols, width, tw_stride);
    }
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// FFT (coset: cosetFFT), in place on vec through the domain's work buffer
template <int M>
int x_forward(mnt753_domain* d, uint32_t* vec, bool coset, hipStream_t st) {
  if (d->kind == MNT753_DOMAIN_MIXED) return mixed_transform<M>(d, vec, false, coset, st);
  if (d->kind == MNT753_DOMAIN_STEP) {
    const StepGrid g = step_grid(d);
    if (coset) hipLaunchKernelGGL((k_step_pre<M, true>), dim3(g.blocks), dim3(g.threads), 0, st, vec, d->work, d->x_fwd, d->xcos_fwd, d->big_m, d->small_m, g.ti_n, g.tj_n);
    else hipLaunchKernelGGL((k_step_pre<M, false>), dim3(g.blocks), dim3(g.threads), 0, st, vec, d->work, d->x_fwd, d->xcos_fwd, d->big_m, d->small_m, g.ti_n, g.tj_n);
  } else {
    const unsigned gb = (unsigned)((d->small_m + 255) / 256);
    if (coset) hipLaunchKernelGGL((k_ext_pre<M, true>), dim3(gb), dim3(256), 0, st, vec, d->work, d->x_fwd, d->xcos_fwd, d->xconsts, d->small_m);
    else hipLaunchKernelGGL((k_ext_pre<M, false>), dim3(gb), dim3(256), 0, st, vec, d->work, d->x_fwd, d->xcos_fwd, d->xconsts, d->small_m);
  }
  HIP_TRY(hipGetLastError());
  return x_inner<M>(d, d->work, vec, false, st);
}
// iFFT (coset: icosetFFT)
template <int M>
int x_inverse(mnt753_domain* d, uint32_t* vec, bool coset, hipStream_t st) {
  if (d->kind == MNT753_DOMAIN_MIXED) return mixed_transform<M>(d, vec, true, coset, st);
  if (int rc = x_inner<M>(d, vec, d->work, true, st)) return rc;
  if (d->kind == MNT753_DOMAIN_STEP) {
    const StepGrid g = step_grid(d);
    if (coset) hipLaunchKernelGGL((k_step_post<M, true>), dim3(g.blocks), dim3(g.threads), 0, st, d->work, vec, d->x_inv, d->x_inv2, d->xcos_inv, d->xconsts, d->big_m, d->small_m, g.ti_n, g.tj_n);
    else hipLaunchKernelGGL((k_step_post<M, false>), dim3(g.blocks), dim3(g.threads), 0, st, d->work, vec, d->x_inv, d->x_inv2, d->xcos_inv, d->xconsts, d->big_m, d->small_m, g.ti_n, g.tj_n);
  } else {
    const unsigned gb = (unsigned)((d->small_m + 255) / 256);
    if (coset) hipLaunchKernelGGL((k_ext_post<M, true>), dim3(gb), dim3(256), 0, st, d->work, vec, d->x_inv, d->xcos_inv, d->xconsts, d->small_m);
    else hipLaunchKernelGGL((k_ext_post<M, false>), dim3(gb), dim3(256), 0, st, d->work, vec, d->x_inv, d->xcos_inv, d->xconsts, d->small_m);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

template <int M>
int fft_t(mnt753_domain* d, int kind, uint32_t* vec, hipStream_t st) {
  const size_t m = d->m;
  if (d->kind != MNT753_DOMAIN_BASIC) {
    switch (kind) {
      case MNT753_FFT: return x_forward<M>(d, vec, false, st);
      case MNT753_IFFT: return x_inverse<M>(d, vec, false, st);
      case MNT753_COSET_FFT: return x_forward<M>(d, vec, true, st);
      case MNT753_ICOSET_FFT: return x_inverse<M>(d, vec, true, st);
      default: return set_error(MNT753_EINVAL, "fft: unknown kind");
    }
  }
  const unsigned gb = (unsigned)((m + 255) / 256);
  switch (kind) {
    case MNT753_FFT:
      return run_stages<M>(d, vec, vec, d->tw_fwd, st);
    case MNT753_IFFT:
      if (int rc = run_stages<M>(d, vec, vec, d->tw_inv, st)) return rc;
      hipLaunchKernelGGL((k_vec_mul_const<M>), dim3(gb), dim3(256), 0, st, vec, d->consts, m);
      break;
    case MNT753_COSET_FFT:
      return run_stages<M>(d, vec, vec, d->tw_fwd, st, d->cos_fwd, nullptr);
    case MNT753_ICOSET_FFT:
      return run_stages<M>(d, vec, vec, d->tw_inv, st, nullptr, d->cos_inv_s);
    default:
      return set_error(MNT753_EINVAL, "fft: unknown kind");
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// compute_H (cuda_prover_piecewise.cu:18-53), all on the device:
//   x -> cosetFFT(iFFT(x)) for x in {a, b, c} = stages(inv), *(g^i/m), stages(fwd)
//   a = (a*b - c)/Z ; a = icosetFFT(a) ; h = a | 0
// x -> cosetFFT(iFFT(x)) = stages(inv), *(g^i/m), stages(fwd)
template <int M>
int h_chain_t(mnt753_domain* d, uint32_t* vec, hipStream_t st) {
  if (d->kind != MNT753_DOMAIN_BASIC) {
    if (int rc = x_inverse<M>(d, vec, false, st)) return rc;
    return x_forward<M>(d, vec, true, st);
  }
  if (int rc = run_stages<M>(d, vec, vec, d->tw_inv, st)) return rc;
  return run_stages<M>(d, vec, vec, d->tw_fwd, st, d->cos_fwd_s, nullptr);      // (g^i / m) rides on the forward transform's first pass
}
// a = (a*b - c)/Z ; a = icosetFFT(a) ; h = a | 0
template <int M>
int h_finish_t(mnt753_domain* d, uint32_t* ca, const uint32_t* cb, const uint32_t* cc, uint32_t* h, hipStream_t st) {
  const size_t m = d->m;
  const unsigned gb = (unsigned)((m + 255) / 256);
  if (d->kind == MNT753_DOMAIN_MIXED) {       // Z on the coset is the one constant g^m - 1, as in the basic domain
    hipLaunchKernelGGL((k_h_pointwise<M>), dim3(gb), dim3(256), 0, st, ca, cb, cc, d->consts + 1 * FPS_WORDS, d->consts + 2 * FPS_WORDS, m);
    if (int rc = x_inverse<M>(d, ca, true, st)) return rc;
  } else if (d->kind != MNT753_DOMAIN_BASIC) {
    hipLaunchKernelGGL((k_h_pointwise_ztab<M>), dim3(gb), dim3(256), 0, st, ca, cb, cc, d->xconsts + 3 * FPS_WORDS, d->zt12, d->z_split, d->z_mask, m);
    if (int rc = x_inverse<M>(d, ca, true, st)) return rc;
  } else {
    hipLaunchKernelGGL((k_h_pointwise<M>), dim3(gb), dim3(256), 0, st, ca, cb, cc, d->consts + 1 * FPS_WORDS, d->consts + 2 * FPS_WORDS, m);
    if (int rc = run_stages<M>(d, ca, ca, d->tw_inv, st, nullptr, d->cos_inv_s)) return rc;
  }
  const size_t quads = m * 6 + 6;
  hipLaunchKernelGGL(k_copy_h, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, h, ca, m);
  HIP_TRY(hipGetLastError());
  return 0;
}
template <int M>
int compute_h_t(mnt753_domain* d, uint32_t* ca, uint32_t* cb, uint32_t* cc, uint32_t* h, hipStream_t st) {
  uint32_t* vecs[3] = {ca, cb, cc};
  for (int v = 0; v < 3; ++v)
    if (int rc = h_chain_t<M>(d, vecs[v], st)) return rc;
  return h_finish_t<M>(d, ca, cb, cc, h, st);
}

int ceil_log2(size_t n) {            // libff::log2
  int r = 0;
  while (r < 64 && ((size_t)1 << r) < n) ++r;
  return r;
}
bool is_pow2(size_t n) { return n && !(n & (n - 1)); }

int create_basic(int curve, int frm, size_t m, bool inner, mnt753_domain** out) {
  mnt753_domain* d = new (std::nothrow) mnt753_domain();
  if (!d) return set_error(MNT753_ENOMEM, "domain_create: host allocation failed");
  d->curve = curve; d->frm = frm; d->m = m; d->logm = ceil_log2(m);
  d->device = current_physical_device(); d->logical_device = mnt753_get_device();
  OnDevice on(d->device);
  int rc = frm == MOD_A ? build_tables<MOD_A>(d, inner) : build_tables<MOD_B>(d, inner);
  if (rc) { mnt753_domain_free(d); return rc; }
  *out = d;
  return 0;
}

// tables of a step / extended domain (d->kind, big_m, small_m set; the inner domains exist)
template <int M>
int build_outer(mnt753_domain* d) {
  typedef HFp<M> Fr;
  const size_t m = d->m, big_m = d->big_m, small_m = d->small_m;
  const bool step = d->kind == MNT753_DOMAIN_STEP;
  const Fr one = Fr::one();
  const Fr g = Fr::from_words(FRD[M].mult_gen), g_inv = g.inverse();
  const Fr two12 = Fr::from_uint(4096), two12_inv = two12.inverse();
  Fr base_fwd, base_inv, scale_inv, k[4];
  std::vector<Fr> z;                    // Z on the coset: z_mask + 2 values (z_index)
  if (step) {
    // omega: the primitive 2^ceil(log2 m)-th root, order 2 big_m (step_radix2_domain.tcc:21-53)
    Fr omega = Fr::from_words(FRD[M].root_of_unity);
    for (int i = FRD[M].two_adicity; i > ceil_log2(m); --i) omega = omega.squared();
    const Fr half = Fr::from_uint(2).inverse();
    const Fr binv = Fr::from_uint((uint64_t)big_m).inverse(), sinv = Fr::from_uint((uint64_t)small_m).inverse();
    base_fwd = omega; base_inv = omega.inverse(); scale_inv = half * binv;
    k[0] = half * binv; k[1] = half * sinv; k[2] = binv; k[3] = two12;
    // Z(g x) = (g^big_m - 1)(g^small_m x^small_m - omega^small_m) on x = omega^(2i): x^small_m = (omega^(2 small_m))^i takes
    // compr values; on x = omega omega_small^i: ((g omega)^big_m - 1)((g omega)^small_m - omega^small_m)     (:252-276)
    const size_t compr = big_m / small_m;
    const Fr z0 = g.pow_u64((uint64_t)big_m) - one, gs = g.pow_u64((uint64_t)small_m), os = omega.pow_u64((uint64_t)small_m);
    const Fr step_w = os.squared(), go = g * omega;
    Fr elt = one;
    for (size_t i = 0; i < compr; ++i) { z.push_back(z0 * (gs * elt - os)); elt = elt * step_w; }
    z.push_back((go.pow_u64((uint64_t)big_m) - one) * (go.pow_u64((uint64_t)small_m) - os));
    d->z_split = big_m; d->z_mask = compr - 1;
  } else {
    // shift = g^2 (libff coset_shift), S = shift^small_m, sconst = 1 / (small_m (1 - S))      (extended_radix2_domain.tcc:48-104)
    const Fr shift = g.squared(), S = shift.pow_u64((uint64_t)small_m);
    const Fr sconst = (Fr::from_uint((uint64_t)small_m) * (one - S)).inverse();
    base_fwd = shift; base_inv = shift.inverse(); scale_inv = sconst;
    k[0] = S; k[1] = sconst; k[2] = one; k[3] = two12;
    const Fr gs = g.pow_u64((uint64_t)small_m);             // (:172-191)
    z.push_back((gs - one) * (gs - S));
    z.push_back((gs * S - one) * (gs * S - S));
    d->z_split = small_m; d->z_mask = 0;
  }
  // 1 / Z: one inversion for the whole table (Montgomery's trick), on the host, once per domain
  const size_t nz = z.size();
  std::vector<Fr> zi(nz);
  {
    std::vector<Fr> pre(nz);
    Fr acc = one;
    for (size_t i = 0; i < nz; ++i) { pre[i] = acc; acc = acc * z[i]; }
    Fr inv = acc.inverse();
    for (size_t i = nz; i-- > 0;) { zi[i] = inv * pre[i]; inv = inv * z[i]; }
  }
  // staging (host, wire form): 4 power tables of 32 entries, 2 scales, 4 constants, then 1/Z and 2^-12/Z
  const size_t z_slot = 4 * 32 + 2 + 4;
  std::vector<uint64_t> stage((z_slot + 2 * nz) * 12);
  auto put = [&](size_t slot, const Fr& v) { memcpy(&stage[slot * 12], v.l, 96); };
  const Fr bases[4] = {base_fwd, base_inv, g, g_inv};
  for (int t = 0; t < 4; ++t) {
    Fr p = bases[t];
    for (int b = 0; b < 32; ++b) { put(t * 32 + b, p); p = p.squared(); }
  }
  put(128, one); put(129, scale_inv);
  for (int i = 0; i < 4; ++i) put(130 + i, k[i]);
  for (size_t i = 0; i < nz; ++i) { put(z_slot + i, zi[i]); put(z_slot + nz + i, zi[i] * two12_inv); }
  HIP_TRY(hipMalloc(&d->stage, stage.size() * 8));
  uint32_t* d_stage = d->stage;
  HIP_TRY(hipMemcpy(d_stage, stage.data(), stage.size() * 8, hipMemcpyHostToDevice));
  const size_t n_x = step ? big_m : small_m;
  HIP_TRY(hipMalloc(&d->x_fwd, n_x * FPS_WORDS * 4));
  HIP_TRY(hipMalloc(&d->x_inv, n_x * FPS_WORDS * 4));
  if (step) HIP_TRY(hipMalloc(&d->x_inv2, small_m * FPS_WORDS * 4));
  HIP_TRY(hipMalloc(&d->xcos_fwd, m * FPS_WORDS * 4));
  HIP_TRY(hipMalloc(&d->xcos_inv, m * FPS_WORDS * 4));
  HIP_TRY(hipMalloc(&d->xconsts, 4 * FPS_WORDS * 4));
  HIP_TRY(hipMalloc(&d->zt, nz * FPS_WORDS * 4));
  HIP_TRY(hipMalloc(&d->zt12, nz * FPS_WORDS * 4));
  HIP_TRY(hipMalloc(&d->work, m * 96));
  const int nbits = ceil_log2(m);
  auto table = [&](uint32_t* out, int base_slot, int scale_slot, size_t n) {
    hipLaunchKernelGGL((k_pow_table<M>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, out, d_stage + (size_t)base_slot * 32 * 24,
                       d_stage + (size_t)scale_slot * 24, n, nbits);
  };
  table(d->x_fwd, 0, 128, n_x);
  if (step) { table(d->x_inv, 0, 129, n_x); table(d->x_inv2, 1, 128, small_m); }
  else table(d->x_inv, 1, 129, n_x);
  table(d->xcos_fwd, 2, 128, m);
  table(d->xcos_inv, 3, 128, m);
  auto internal = [&](uint32_t* out, size_t slot, size_t n) {
    hipLaunchKernelGGL((k_consts_to_internal<M>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, out, d_stage + slot * 24, (int)n);
  };
  internal(d->xconsts, 130, 4);
  internal(d->zt, z_slot, nz);
  internal(d->zt12, z_slot + nz, nz);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  return 0;
}

int create_outer(int curve, int frm, int kind, size_t m, mnt753_domain** out) {
  mnt753_domain* d = new (std::nothrow) mnt753_domain();
  if (!d) return set_error(MNT753_ENOMEM, "domain_create_for: host allocation failed");
  d->curve = curve; d->frm = frm; d->m = m; d->kind = kind;
  d->big_m = kind == MNT753_DOMAIN_STEP ? (size_t)1 << (ceil_log2(m) - 1) : m / 2;
  d->small_m = m - d->big_m;
  d->device = current_physical_device(); d->logical_device = mnt753_get_device();
  OnDevice on(d->device);
  int rc = create_basic(curve, frm, d->big_m, true, &d->sub_big);
  if (!rc) {
    if (kind == MNT753_DOMAIN_EXTENDED) d->sub_small = d->sub_big;      // both halves are size-small_m transforms, one after the other
    else if (d->small_m > 1) rc = create_basic(curve, frm, d->small_m, true, &d->sub_small);
  }
  if (!rc) rc = frm == MOD_A ? build_outer<MOD_A>(d) : build_outer<MOD_B>(d);
  if (rc) { mnt753_domain_free(d); return rc; }
  *out = d;
  return 0;
}

// tables of a mixed-radix domain (q_n, q_pow, t_n set; the inner domain exists where t_n > 1)
template <int M>
int build_mixed(mnt753_domain* d) {
  typedef HFp<M> Fr;
  const size_t m = d->m;
  const Fr one = Fr::one();
  // omega = get_root_of_unity(m): full_root_of_unity to the 5th power (2 - b) times, then squared (s - a) times (field_utils.tcc:59-70)
  Fr omega = Fr::from_words(FR_FULL_ROOT_B);
  for (unsigned i = d->q_pow; i < (unsigned)FR_SMALL_SUBGROUP_POWER_B; ++i) omega = omega.pow_u64(FR_SMALL_SUBGROUP_BASE_B);
  for (int i = FRD[M].two_adicity; i > ceil_log2(d->t_n); --i) omega = omega.squared();
  const Fr omega_inv = omega.inverse();
  const Fr g = Fr::from_words(FRD[M].mult_gen), g_inv = g.inverse();
  const Fr minv = Fr::from_uint((uint64_t)m).inverse();
  const Fr zinv = (g.pow_u64((uint64_t)m) - one).inverse();      // basic_radix2_domain.tcc:113-116
  const Fr two12 = Fr::from_uint(4096), two12_inv = two12.inverse();
  const Fr zeta = omega.pow_u64((uint64_t)(m / 5)), zeta_inv = zeta.inverse();
  // staging (host, wire form): 4 power tables of 32 entries, the scale 1, 15 radix-5 constants, the 4 constants of a basic domain
  std::vector<uint64_t> stage((4 * 32 + 1 + 15 + 4) * 12);
  auto put = [&](size_t slot, const Fr& v) { memcpy(&stage[slot * 12], v.l, 96); };
  const Fr bases[4] = {omega, omega_inv, g, g_inv};
  for (int t = 0; t < 4; ++t) {
    Fr p = bases[t];
    for (int b = 0; b < 32; ++b) { put(t * 32 + b, p); p = p.squared(); }
  }
  put(128, one);
  Fr zf = one, zi = one;
  for (int e = 0; e < 5; ++e) { put(129 + e, zf); put(134 + e, zi); put(139 + e, zi * minv); zf = zf * zeta; zi = zi * zeta_inv; }
  put(144, minv); put(145, two12); put(146, zinv * two12_inv); put(147, zinv);
  HIP_TRY(hipMalloc(&d->stage, stage.size() * 8));
  uint32_t* d_stage = d->stage;
  HIP_TRY(hipMemcpy(d_stage, stage.data(), stage.size() * 8, hipMemcpyHostToDevice));
  uint32_t** tables[4] = {&d->x_fwd, &d->x_inv, &d->xcos_fwd, &d->xcos_inv};
  for (auto t : tables) HIP_TRY(hipMalloc(t, m * FPS_WORDS * 4));
  HIP_TRY(hipMalloc(&d->xconsts, 15 * FPS_WORDS * 4));
  HIP_TRY(hipMalloc(&d->consts, 4 * FPS_WORDS * 4));
  HIP_TRY(hipMalloc(&d->work, m * 96));
  const int nbits = ceil_log2(m);
  for (int t = 0; t < 4; ++t)
    hipLaunchKernelGGL((k_pow_table<M>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, *tables[t], d_stage + (size_t)t * 32 * 24,
                       d_stage + (size_t)128 * 24, m, nbits);
  hipLaunchKernelGGL((k_consts_to_internal<M>), dim3(1), dim3(64), 0, 0, d->xconsts, d_stage + (size_t)129 * 24, 15);
  hipLaunchKernelGGL((k_consts_to_internal<M>), dim3(1), dim3(64), 0, 0, d->consts, d_stage + (size_t)144 * 24, 4);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  return 0;
}

// m = 2^a 5^b with a <= s and 1 <= b <= 2 on MNT6753 (the callers have checked)
int create_mixed(int curve, int frm, size_t m, mnt753_domain** out) {
  mnt753_domain* d = new (std::nothrow) mnt753_domain();
  if (!d) return set_error(MNT753_ENOMEM, "domain_create_mixed: host allocation failed");
  d->curve = curve; d->frm = frm; d->m = m; d->kind = MNT753_DOMAIN_MIXED;
  d->q_n = 1; d->t_n = m;
  while (d->t_n % 5 == 0) { d->t_n /= 5; d->q_n *= 5; ++d->q_pow; }
  d->device = current_physical_device(); d->logical_device = mnt753_get_device();
  OnDevice on(d->device);
  int rc = 0;
  if (d->t_n > 1) rc = create_basic(curve, frm, d->t_n, true, &d->sub_big);      // omega^q_n is that domain's own root
  if (!rc) rc = build_mixed<MOD_B>(d);
  if (rc) { mnt753_domain_free(d); return rc; }
  *out = d;
  return 0;
}

// ---- which domain libfqfft's get_evaluation_domain(min_size) builds (get_evaluation_domain.tcc:58-135) -----------------------------
// Each candidate is accepted by its constructor's own test.  MNT6753's Fr has a small subgroup of order 5^2 defined
// (mnt6753_init.cpp:73-75): there basic_radix2_domain accepts every 2^a 5^b, a <= 15, b <= 2, and get_root_of_unity likewise.
// A candidate the reference accepts and this library does not build ends the walk with MNT753_EDOMAIN.  The mixed-radix basic
// domains (candidates 1, 4 and 7 at a size 2^a 5^b, b >= 1) are built where the caller allows them (MNT753_DOMAIN_ALLOW_MIXED).
struct Pick { int kind; size_t m; };           // kind < 0: refused, the message is set
constexpr int Q_BASE = 5, Q_POWER = 2;         // MNT6753 Fr: small_subgroup_base, small_subgroup_power
bool small_subgroup(int frm) { return frm == MOD_B; }
void split_2q(size_t n, int& a, int& b, size_t& rest) {
  a = b = 0;
  while (n % 2 == 0) { n /= 2; ++a; }
  while (n % Q_BASE == 0) { n /= Q_BASE; ++b; }
  rest = n;
}
// libff get_root_of_unity(n) succeeds (field_utils.tcc:40-89)
bool has_root(int frm, size_t n) {
  if (n == 0) return false;
  if (small_subgroup(frm)) {
    int a, b; size_t rest;
    split_2q(n, a, b, rest);
    return rest == 1 && a <= FRD[frm].two_adicity && b <= Q_POWER;
  }
  return is_pow2(n) && ceil_log2(n) <= FRD[frm].two_adicity;
}
bool basic_accepts(int frm, size_t m) {        // basic_radix2_domain.tcc:26-60
  if (m <= 1) return false;
  if (small_subgroup(frm)) {
    int a, b; size_t rest;
    split_2q(m, a, b, rest);
    return rest == 1 && has_root(frm, m);
  }
  return ceil_log2(m) <= FRD[frm].two_adicity && has_root(frm, m);
}
bool extended_accepts(int frm, size_t m) {     // extended_radix2_domain.tcc:21-46
  return m > 1 && ceil_log2(m) == FRD[frm].two_adicity + 1 && has_root(frm, m / 2);
}
bool step_accepts(int frm, size_t m) {         // step_radix2_domain.tcc:21-53
  if (m <= 1) return false;
  const int l = ceil_log2(m);
  if (l >= 63) return false;
  const size_t big_m = (size_t)1 << (l - 1), small_m = m - big_m;
  return is_pow2(small_m) && has_root(frm, (size_t)1 << l) && has_root(frm, small_m);
}
Pick refuse(const char* curve_name, size_t min_size, const char* fmt, size_t a) {
  char what[160], msg[320];
  snprintf(what, sizeof what, fmt, a);
  snprintf(msg, sizeof msg, "domain_create_for: %s, min_size %zu: the reference uses %s, which this library does not build", curve_name, min_size, what);
  set_error(MNT753_EDOMAIN, msg);
  return Pick{-1, 0};
}
Pick select_domain(int frm, size_t min_size, unsigned flags) {
  const bool allow_mixed = flags & MNT753_DOMAIN_ALLOW_MIXED;
  const char* name = frm == MOD_A ? "MNT4753" : "MNT6753";
  if (min_size <= 1) {
    set_error(MNT753_EDOMAIN, "domain_create_for: min_size must be above 1 (no domain of the reference accepts 0 or 1)");
    return Pick{-1, 0};
  }
  if (ceil_log2(min_size) >= 62) return refuse(name, min_size, "no radix-2 domain (size %zu is beyond every root of unity)", min_size);
  const size_t big = (size_t)1 << (ceil_log2(min_size) - 1), small = min_size - big;
  const size_t sizes[2] = {min_size, big + ((size_t)1 << ceil_log2(small))};
  for (int pass = 0; pass < 2; ++pass) {       // candidates 1-3 at min_size, 4-6 at big + rounded_small
    const size_t m = sizes[pass];
    if (basic_accepts(frm, m)) {
      if (is_pow2(m)) return Pick{MNT753_DOMAIN_BASIC, m};
      if (allow_mixed) return Pick{MNT753_DOMAIN_MIXED, m};
      return refuse(name, min_size, "a mixed-radix basic_radix2_domain of size %zu (2^a 5^b)", m);
    }
    if (extended_accepts(frm, m)) {
      if (m % 2 == 0 && is_pow2(m / 2)) return Pick{MNT753_DOMAIN_EXTENDED, m};
      return refuse(name, min_size, "an extended_radix2_domain of size %zu over a mixed-radix half", m);
    }
    if (step_accepts(frm, m)) return Pick{MNT753_DOMAIN_STEP, m};      // big_m and small_m are powers of two: plain radix 2
  }
  if (small_subgroup(frm)) {                   // candidate 7: the smallest 2^a 5^b >= min_size, a <= s, b <= 2
    size_t best = SIZE_MAX;
    for (int b = 0; b <= Q_POWER; ++b) {
      size_t r = 1;
      for (int i = 0; i < b; ++i) r *= Q_BASE;
      int a = 0;
      while (r < min_size) { r *= 2; ++a; }
      if (a <= FRD[frm].two_adicity && r < best) best = r;
    }
    if (best != SIZE_MAX && basic_accepts(frm, best)) {
      if (is_pow2(best)) return Pick{MNT753_DOMAIN_BASIC, best};
      if (allow_mixed) return Pick{MNT753_DOMAIN_MIXED, best};
      return refuse(name, min_size, "a mixed-radix basic_radix2_domain of size %zu (2^a 5^b, candidate 7)", best);
    }
  }
  return refuse(name, min_size, "a geometric or arithmetic sequence domain of size %zu (past candidate 7)", min_size);
}

// ---- the Lagrange coefficients and Z at a point ----------------------------------------------------------
// The handful of scalars of a call (t^n, Z, 1 / n, the coefficients of the two halves of an extended or step domain) are computed
// here, on the host, and travel as kernel arguments; the work per element is qap_kernels.hip.h.
template <int M>
WireElem wire_of(const HFp<M>& v) { WireElem w; memcpy(w.w, v.l, 96); return w; }
template <int M>
HFp<M> step_omega(const mnt753_domain* d) {          // the root of order 2 big_m of a step domain (step_radix2_domain.tcc:21-53)
  HFp<M> omega = HFp<M>::from_words(FRD[M].root_of_unity);
  for (int i = FRD[M].two_adicity; i > ceil_log2(d->m); --i) omega = omega.squared();
  return omega;
}
template <int M>
HFp<M> vanishing_t(const mnt753_domain* d, const HFp<M>& t) {
  typedef HFp<M> Fr;
  const Fr one = Fr::one();
  if (d->kind == MNT753_DOMAIN_EXTENDED) {           // extended_radix2_domain.tcc:155-158
    const Fr g = Fr::from_words(FRD[M].mult_gen), ts = t.pow_u64((uint64_t)d->small_m);
    return (ts - one) * (ts - g.squared().pow_u64((uint64_t)d->small_m));
  }
  if (d->kind == MNT753_DOMAIN_STEP)                 // step_radix2_domain.tcc:230-233
    return (t.pow_u64((uint64_t)d->big_m) - one) * (t.pow_u64((uint64_t)d->small_m) - step_omega<M>(d).pow_u64((uint64_t)d->small_m));
  return t.pow_u64((uint64_t)d->m) - one;            // basic and mixed: t^m - 1
}
// _basic_radix2_evaluate_all_lagrange_polynomials(n, t) times `coeff` into elements [off, off + n) of out
// (basic_radix2_domain_aux.tcc:333-395).  tab: omega^j of the subgroup (half: j < n / 2 only), null for n == 1.  os != null: the big
// half of a step domain, whose element i is also divided by omega_big^(i stride) - *os.
template <int M>
int lagrange_sub(mnt753_domain* d, const uint32_t* tab, size_t n, bool half, uint32_t* out, size_t off, const HFp<M>& t, const HFp<M>& coeff,
                 const HFp<M>* os, size_t stride, hipStream_t st) {
  typedef HFp<M> Fr;
  const Fr one = Fr::one();
  const Fr tn = t.pow_u64((uint64_t)n);
  if (n == 1 || tn == one) {
    // t is an element of the subgroup: Z = 0 and nothing may be inverted.  The indicator vector, times the factors the outer formulas
    // put on the matching element (omega_big^(i stride) = t^stride there).
    Fr value = coeff;
    if (os) value = value * (t.pow_u64((uint64_t)stride) - *os).inverse();
    hipLaunchKernelGGL((k_lagrange_indicator<M>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n == 1 ? nullptr : tab, n, half ? 1 : 0,
                       out + off * 24, wire_of(t), wire_of(value));
    HIP_TRY(hipGetLastError());
    return 0;
  }
  const Fr c = (tn - one) * Fr::from_uint((uint64_t)n).inverse() * coeff;
  const size_t runs = (n + LAG_INV_BATCH - 1) / LAG_INV_BATCH;
  const unsigned g = (unsigned)((runs + 255) / 256);
  uint32_t* pre = d->lag_pre + off * FPS_WORDS;
  if (os) hipLaunchKernelGGL((k_lagrange_run<M, true>), dim3(g), dim3(256), 0, st, tab, n, half ? 1 : 0, pre, out + off * 24, wire_of(t), wire_of(c), wire_of(*os), stride);
  else hipLaunchKernelGGL((k_lagrange_run<M, false>), dim3(g), dim3(256), 0, st, tab, n, half ? 1 : 0, pre, out + off * 24, wire_of(t), wire_of(c), wire_of(one), (size_t)0);
  HIP_TRY(hipGetLastError());
  return 0;
}
template <int M>
int lagrange_t(mnt753_domain* d, const uint64_t* host_t, uint32_t* out, hipStream_t st) {
  typedef HFp<M> Fr;
  const Fr one = Fr::one(), t = Fr::from_words(host_t);
  if (d->kind == MNT753_DOMAIN_BASIC) return lagrange_sub<M>(d, d->tw_fwd, d->m, true, out, 0, t, one, nullptr, 0, st);
  if (d->kind == MNT753_DOMAIN_MIXED) return lagrange_sub<M>(d, d->x_fwd, d->m, false, out, 0, t, one, nullptr, 0, st);
  const size_t big_m = d->big_m, small_m = d->small_m;
  if (d->kind == MNT753_DOMAIN_EXTENDED) {           // extended_radix2_domain.tcc:120-139
    const Fr shift = Fr::from_words(FRD[M].mult_gen).squared();
    const Fr ts = t.pow_u64((uint64_t)small_m), ss = shift.pow_u64((uint64_t)small_m);
    const Fr one_over_denom = (ss - one).inverse();
    const Fr t0_coeff = (ts - ss) * (-one_over_denom), t1_coeff = (ts - one) * one_over_denom;
    if (int rc = lagrange_sub<M>(d, d->sub_big->tw_fwd, small_m, true, out, 0, t, t0_coeff, nullptr, 0, st)) return rc;
    return lagrange_sub<M>(d, d->sub_big->tw_fwd, small_m, true, out, small_m, t * shift.inverse(), t1_coeff, nullptr, 0, st);
  }
  // step_radix2_domain.tcc:189-214
  const Fr omega = step_omega<M>(d), os = omega.pow_u64((uint64_t)small_m);
  const Fr l0 = t.pow_u64((uint64_t)small_m) - os;
  const Fr l1 = (t.pow_u64((uint64_t)big_m) - one) * (omega.pow_u64((uint64_t)big_m) - one).inverse();
  if (int rc = lagrange_sub<M>(d, d->sub_big->tw_fwd, big_m, true, out, 0, t, l0, &os, small_m, st)) return rc;
  return lagrange_sub<M>(d, d->sub_small ? d->sub_small->tw_fwd : nullptr, small_m, true, out, big_m, t * omega.inverse(), l1, nullptr, 0, st);
}

}  // namespace

namespace mnt753 {
int domain_curve(const mnt753_domain* d) { return d ? d->curve : -1; }
}

extern "C" {

int mnt753_domain_create(int curve, size_t m, mnt753_domain** out) {
  if (!out || curve < 0 || curve > 1) return set_error(MNT753_EINVAL, "domain_create: bad argument");
  if (int rc = require_device()) return rc;
  const int frm = curve == MNT753_CURVE_MNT4753 ? MOD_A : MOD_B;
  // basic_radix2_domain constructor (basic_radix2_domain.tcc:25-60): m > 1, a power of two, log2 m <= s
  int logm = 0;
  while (((size_t)1 << logm) < m) ++logm;
  if (m <= 1 || ((size_t)1 << logm) != m || logm > FRD[frm].two_adicity)
    return set_error(MNT753_EDOMAIN, "domain_create: size must be a power of two in (1, 2^s], s = 30 (MNT4753) / 15 (MNT6753)");
  return create_basic(curve, frm, m, false, out);
}

int mnt753_domain_create_mixed(int curve, size_t m, mnt753_domain** out) {
  if (!out || curve < 0 || curve > 1) return set_error(MNT753_EINVAL, "domain_create_mixed: bad argument");
  if (int rc = require_device()) return rc;
  const int frm = curve == MNT753_CURVE_MNT4753 ? MOD_A : MOD_B;
  // basic_radix2_domain over a field with a small subgroup (basic_radix2_domain.tcc:26-60); the powers of two are mnt753_domain_create's
  int a, b; size_t rest;
  split_2q(m ? m : 1, a, b, rest);
  if (!small_subgroup(frm) || rest != 1 || b < 1 || b > Q_POWER || a > FRD[frm].two_adicity)
    return set_error(MNT753_EDOMAIN, "domain_create_mixed: MNT6753 only, size must be 2^a 5^b with a <= 15 and 1 <= b <= 2");
  return create_mixed(curve, frm, m, out);
}

int mnt753_domain_create_for_ex(int curve, size_t min_size, unsigned flags, mnt753_domain** out) {
  if (!out || curve < 0 || curve > 1 || (flags & ~MNT753_DOMAIN_ALLOW_MIXED)) return set_error(MNT753_EINVAL, "domain_create_for: bad argument");
  if (int rc = require_device()) return rc;
  const int frm = curve == MNT753_CURVE_MNT4753 ? MOD_A : MOD_B;
  const Pick p = select_domain(frm, min_size, flags);
  if (p.kind < 0) return MNT753_EDOMAIN;
  if (p.kind == MNT753_DOMAIN_BASIC) return create_basic(curve, frm, p.m, false, out);
  if (p.kind == MNT753_DOMAIN_MIXED) return create_mixed(curve, frm, p.m, out);
  return create_outer(curve, frm, p.kind, p.m, out);
}

int mnt753_domain_create_for(int curve, size_t min_size, mnt753_domain** out) {
  return mnt753_domain_create_for_ex(curve, min_size, 0, out);
}

int mnt753_domain_kind(const mnt753_domain* d) { return d ? d->kind : -1; }

int mnt753_domain_free(mnt753_domain* d) {
  if (!d) return 0;
  if (d->sub_small && d->sub_small != d->sub_big) mnt753_domain_free(d->sub_small);
  if (d->sub_big) mnt753_domain_free(d->sub_big);
  OnDevice on(d->device);
  void* ptrs[] = {d->tw_fwd, d->tw_inv, d->cos_fwd, d->cos_fwd_s, d->cos_inv_s, d->consts, d->work, d->stage,
                  d->x_fwd, d->x_inv, d->x_inv2, d->xcos_fwd, d->xcos_inv, d->xconsts, d->zt, d->zt12, d->lag_pre};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  if (d->work_free) (void)hipEventDestroy(d->work_free);
  delete d;
  return 0;
}

size_t mnt753_domain_size(const mnt753_domain* d) { return d ? d->m : 0; }
int mnt753_domain_device(const mnt753_domain* d) { return d ? d->logical_device : -1; }

// Every transform of a domain ping-pongs through the domain's one work buffer.  Callers on different streams are serialised on
// the device: a transform first waits for the event the previous one recorded (host threads must still not call into the
// same domain concurrently -- the threading contract of the reference wrapper).
static int work_acquire(mnt753_domain* d, hipStream_t st) {
  if (!d->work_free) HIP_TRY(hipEventCreateWithFlags(&d->work_free, hipEventDisableTiming));
  else HIP_TRY(hipStreamWaitEvent(st, d->work_free, 0));
  return 0;
}
static int work_release(mnt753_domain* d, hipStream_t st, int rc) {
  if (rc) return rc;
  HIP_TRY(hipEventRecord(d->work_free, st));
  return 0;
}

int mnt753_fft(mnt753_domain* d, int kind, uint64_t* dev_vec, void* stream) {
  if (!d || !dev_vec) return set_error(MNT753_EINVAL, "fft: null argument");
  if (int rc = require_device()) return rc;
  uint32_t* v = reinterpret_cast<uint32_t*>(dev_vec);
  OnDevice on(d->device);
  if (int rc = work_acquire(d, (hipStream_t)stream)) return rc;
  const int rc = d->frm == MOD_A ? fft_t<MOD_A>(d, kind, v, (hipStream_t)stream) : fft_t<MOD_B>(d, kind, v, (hipStream_t)stream);
  return work_release(d, (hipStream_t)stream, rc);
}

int mnt753_divide_by_z_on_coset(mnt753_domain* d, uint64_t* dev_vec, void* stream) {
  if (!d || !dev_vec) return set_error(MNT753_EINVAL, "divide_by_z_on_coset: null argument");
  if (int rc = require_device()) return rc;
  const unsigned gb = (unsigned)((d->m + 255) / 256);
  uint32_t* v = reinterpret_cast<uint32_t*>(dev_vec);
  OnDevice on(d->device);
  if (d->kind == MNT753_DOMAIN_STEP || d->kind == MNT753_DOMAIN_EXTENDED) {
    if (d->frm == MOD_A) hipLaunchKernelGGL((k_vec_mul_ztab<MOD_A>), dim3(gb), dim3(256), 0, (hipStream_t)stream, v, d->zt, d->z_split, d->z_mask, d->m);
    else hipLaunchKernelGGL((k_vec_mul_ztab<MOD_B>), dim3(gb), dim3(256), 0, (hipStream_t)stream, v, d->zt, d->z_split, d->z_mask, d->m);
  } else if (d->frm == MOD_A) hipLaunchKernelGGL((k_vec_mul_const<MOD_A>), dim3(gb), dim3(256), 0, (hipStream_t)stream, v, d->consts + 3 * FPS_WORDS, d->m);
  else hipLaunchKernelGGL((k_vec_mul_const<MOD_B>), dim3(gb), dim3(256), 0, (hipStream_t)stream, v, d->consts + 3 * FPS_WORDS, d->m);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mnt753_vec_muleq(int curve, uint64_t* dev_a, const uint64_t* dev_b, size_t n, void* stream) {
  if (curve < 0 || curve > 1 || (n && (!dev_a || !dev_b))) return set_error(MNT753_EINVAL, "vec_muleq: bad argument");
  if (int rc = require_device()) return rc;
  if (n == 0) return 0;
  const unsigned gb = (unsigned)((n + 255) / 256);
  uint32_t* a = reinterpret_cast<uint32_t*>(dev_a);
  const uint32_t* b = reinterpret_cast<const uint32_t*>(dev_b);
  if (curve == MNT753_CURVE_MNT4753) hipLaunchKernelGGL((k_vec_muleq<MOD_A>), dim3(gb), dim3(256), 0, (hipStream_t)stream, a, b, n);
  else hipLaunchKernelGGL((k_vec_muleq<MOD_B>), dim3(gb), dim3(256), 0, (hipStream_t)stream, a, b, n);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mnt753_vec_scale(int curve, uint64_t* dev_dst, const uint64_t* dev_src, const uint64_t* host_scalar, size_t n, void* stream) {
  if (curve < 0 || curve > 1 || !host_scalar || (n && (!dev_dst || !dev_src))) return set_error(MNT753_EINVAL, "vec_scale: bad argument");
  if (int rc = require_device()) return rc;
  if (n == 0) return 0;
  const unsigned gb = (unsigned)((n + 255) / 256);
  WireElem k;
  memcpy(k.w, host_scalar, 96);
  uint32_t* d = reinterpret_cast<uint32_t*>(dev_dst);
  const uint32_t* s = reinterpret_cast<const uint32_t*>(dev_src);
  if (curve == MNT753_CURVE_MNT4753) hipLaunchKernelGGL((k_vec_scale<MOD_A>), dim3(gb), dim3(256), 0, (hipStream_t)stream, d, s, k, n);
  else hipLaunchKernelGGL((k_vec_scale<MOD_B>), dim3(gb), dim3(256), 0, (hipStream_t)stream, d, s, k, n);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mnt753_vec_subeq(int curve, uint64_t* dev_a, const uint64_t* dev_b, size_t n, void* stream) {
  if (curve < 0 || curve > 1 || (n && (!dev_a || !dev_b))) return set_error(MNT753_EINVAL, "vec_subeq: bad argument");
  if (int rc = require_device()) return rc;
  if (n == 0) return 0;
  const unsigned gb = (unsigned)((n + 255) / 256);
  uint32_t* a = reinterpret_cast<uint32_t*>(dev_a);
  const uint32_t* b = reinterpret_cast<const uint32_t*>(dev_b);
  if (curve == MNT753_CURVE_MNT4753) hipLaunchKernelGGL((k_vec_subeq<MOD_A>), dim3(gb), dim3(256), 0, (hipStream_t)stream, a, b, n);
  else hipLaunchKernelGGL((k_vec_subeq<MOD_B>), dim3(gb), dim3(256), 0, (hipStream_t)stream, a, b, n);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mnt753_compute_h(mnt753_domain* d, uint64_t* dev_ca, uint64_t* dev_cb, uint64_t* dev_cc, uint64_t* dev_h, void* stream) {
  if (!d || !dev_ca || !dev_cb || !dev_cc || !dev_h) return set_error(MNT753_EINVAL, "compute_h: null argument");
  if (int rc = require_device()) return rc;
  uint32_t *a = reinterpret_cast<uint32_t*>(dev_ca), *b = reinterpret_cast<uint32_t*>(dev_cb), *c = reinterpret_cast<uint32_t*>(dev_cc),
           *h = reinterpret_cast<uint32_t*>(dev_h);
  OnDevice on(d->device);
  if (int rc = work_acquire(d, (hipStream_t)stream)) return rc;
  const int rc = d->frm == MOD_A ? compute_h_t<MOD_A>(d, a, b, c, h, (hipStream_t)stream) : compute_h_t<MOD_B>(d, a, b, c, h, (hipStream_t)stream);
  return work_release(d, (hipStream_t)stream, rc);
}

int mnt753_compute_h_chain(mnt753_domain* d, uint64_t* dev_vec, void* stream) {
  if (!d || !dev_vec) return set_error(MNT753_EINVAL, "compute_h_chain: null argument");
  if (int rc = require_device()) return rc;
  OnDevice on(d->device);
  if (int rc = work_acquire(d, (hipStream_t)stream)) return rc;
  uint32_t* v = reinterpret_cast<uint32_t*>(dev_vec);
  const int rc = d->frm == MOD_A ? h_chain_t<MOD_A>(d, v, (hipStream_t)stream) : h_chain_t<MOD_B>(d, v, (hipStream_t)stream);
  return work_release(d, (hipStream_t)stream, rc);
}

int mnt753_compute_h_finish(mnt753_domain* d, uint64_t* dev_a, const uint64_t* dev_b, const uint64_t* dev_c, uint64_t* dev_h, void* stream) {
  if (!d || !dev_a || !dev_b || !dev_c || !dev_h) return set_error(MNT753_EINVAL, "compute_h_finish: null argument");
  if (int rc = require_device()) return rc;
  OnDevice on(d->device);
  if (int rc = work_acquire(d, (hipStream_t)stream)) return rc;
  uint32_t* a = reinterpret_cast<uint32_t*>(dev_a);
  const uint32_t *b = reinterpret_cast<const uint32_t*>(dev_b), *c = reinterpret_cast<const uint32_t*>(dev_c);
  uint32_t* h = reinterpret_cast<uint32_t*>(dev_h);
  const int rc = d->frm == MOD_A ? h_finish_t<MOD_A>(d, a, b, c, h, (hipStream_t)stream) : h_finish_t<MOD_B>(d, a, b, c, h, (hipStream_t)stream);
  return work_release(d, (hipStream_t)stream, rc);
}

static bool fr_canonical(int frm, const uint64_t* w) { return frm == MOD_A ? !HFp<MOD_A>::geq_p(w) : !HFp<MOD_B>::geq_p(w); }

int mnt753_domain_vanishing_at(mnt753_domain* d, const uint64_t* host_t, uint64_t* host_zt) {
  if (!d || !host_t || !host_zt) return set_error(MNT753_EINVAL, "domain_vanishing_at: null argument");
  if (!fr_canonical(d->frm, host_t)) return set_error(MNT753_EINVAL, "domain_vanishing_at: t is not a canonical element of Fr");
  if (d->frm == MOD_A) memcpy(host_zt, vanishing_t<MOD_A>(d, HFp<MOD_A>::from_words(host_t)).l, 96);
  else memcpy(host_zt, vanishing_t<MOD_B>(d, HFp<MOD_B>::from_words(host_t)).l, 96);
  return 0;
}

int mnt753_domain_lagrange_at(mnt753_domain* d, const uint64_t* host_t, uint64_t* dev_u, void* stream) {
  if (!d || !host_t || !dev_u) return set_error(MNT753_EINVAL, "domain_lagrange_at: null argument");
  if (!fr_canonical(d->frm, host_t)) return set_error(MNT753_EINVAL, "domain_lagrange_at: t is not a canonical element of Fr");
  if (int rc = require_device()) return rc;
  OnDevice on(d->device);
  if (!d->lag_pre) {
    if (hipMalloc(&d->lag_pre, d->m * FPS_WORDS * 4) != hipSuccess) {
      (void)hipGetLastError();
      d->lag_pre = nullptr;
      return set_error(MNT753_ENOMEM, "domain_lagrange_at: device allocation failed");
    }
  }
  if (int rc = work_acquire(d, (hipStream_t)stream)) return rc;      // lag_pre is shared like `work`: calls on different streams are ordered
  uint32_t* u = reinterpret_cast<uint32_t*>(dev_u);
  const int rc = d->frm == MOD_A ? lagrange_t<MOD_A>(d, host_t, u, (hipStream_t)stream) : lagrange_t<MOD_B>(d, host_t, u, (hipStream_t)stream);
  return work_release(d, (hipStream_t)stream, rc);
}

int mnt753_vec_powers(int curve, const uint64_t* host_t, uint64_t* dev_out, size_t n, void* stream) {
  if (curve < 0 || curve > 1 || !host_t || (n && !dev_out)) return set_error(MNT753_EINVAL, "vec_powers: bad argument");
  if (!fr_canonical(curve == MNT753_CURVE_MNT4753 ? MOD_A : MOD_B, host_t)) return set_error(MNT753_EINVAL, "vec_powers: t is not a canonical element of Fr");
  if (int rc = require_device()) return rc;
  if (n == 0) return 0;
  WireElem t;
  memcpy(t.w, host_t, 96);
  const size_t runs = (n + POW_RUN - 1) / POW_RUN;
  const unsigned g = (unsigned)((runs + 255) / 256);
  uint32_t* out = reinterpret_cast<uint32_t*>(dev_out);
  if (curve == MNT753_CURVE_MNT4753) hipLaunchKernelGGL((k_vec_powers<MOD_A>), dim3(g), dim3(256), 0, (hipStream_t)stream, out, t, n);
  else hipLaunchKernelGGL((k_vec_powers<MOD_B>), dim3(g), dim3(256), 0, (hipStream_t)stream, out, t, n);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"

// ---- reductions over Fr and the spot check of compute_H (reduce_kernels.hip.h) -------------------------------
namespace {

// The partial sums of a launch and its results, one buffer per device for the life of the process (340 KB).  A reduction holds
// the device's mutex from its first launch until its result is on the host: every one of these calls waits for its stream anyway.
struct RedScratch {
  std::mutex mu;
  uint32_t* p = nullptr;      // RED_MAX_BLOCKS * 3 partials, then 3 results in wire form
  unsigned cap = 0;           // blocks per launch on this device
};
constexpr int RED_MAX_DEVICES = 64;
int current_device_ordinal() {      // HIP's current device: the one the launches below go to (OnDevice, or the caller's own)
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = -1; }
  return dev;
}
RedScratch g_red[RED_MAX_DEVICES];
constexpr size_t RED_PARTIAL_WORDS = (size_t)RED_MAX_BLOCKS * 3 * FPS_WORDS;

int red_scratch(int dev, RedScratch** out) {      // the caller is on device `dev`
  if (dev < 0 || dev >= RED_MAX_DEVICES) return set_error(MNT753_EINVAL, "reduction: device ordinal out of range");
  RedScratch* s = &g_red[dev];
  std::lock_guard<std::mutex> lock(s->mu);
  if (!s->p) {
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const unsigned cap = (unsigned)(cus > 0 ? cus : 1) * RED_BLOCKS_PER_CU;
    uint32_t* p = nullptr;
    if (hipMalloc(&p, (RED_PARTIAL_WORDS + 3 * 24) * 4) != hipSuccess) {
      (void)hipGetLastError();
      return set_error(MNT753_ENOMEM, "reduction: device allocation failed");
    }
    s->cap = cap < RED_MAX_BLOCKS ? cap : RED_MAX_BLOCKS;
    s->p = p;
  }
  *out = s;
  return 0;
}

// k (1 or 3) inner products over n > 0 elements against u, results to the host; on the current device, which owns the vectors.
// max_blocks: 0 for the device's own cap, else a smaller one (the test hook)
template <int M>
int dot_t(const uint32_t* const* vecs, int k, const uint32_t* u, size_t n, uint64_t* host_out, unsigned max_blocks, hipStream_t st) {
  RedScratch* s = nullptr;
  if (int rc = red_scratch(current_device_ordinal(), &s)) return rc;
  std::lock_guard<std::mutex> lock(s->mu);
  unsigned cap = s->cap;
  if (max_blocks && max_blocks < cap) cap = max_blocks;
  const size_t want = (n + RED_BLOCK - 1) / RED_BLOCK;
  const unsigned nb = (unsigned)(want < cap ? want : cap);
  uint32_t* res = s->p + RED_PARTIAL_WORDS;
  DotVecs v{{vecs[0], k == 3 ? vecs[1] : vecs[0], k == 3 ? vecs[2] : vecs[0]}};
  if (k == 3) hipLaunchKernelGGL((k_vec_dot<M, 3>), dim3(nb), dim3(RED_BLOCK), 0, st, v, u, n, s->p);
  else hipLaunchKernelGGL((k_vec_dot<M, 1>), dim3(nb), dim3(RED_BLOCK), 0, st, v, u, n, s->p);
  hipLaunchKernelGGL((k_red_fold<M>), dim3(1), dim3(RED_BLOCK), 0, st, s->p, nb, k, 1, res);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(host_out, res, (size_t)k * 96, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

template <int M>
int poly_t(const uint32_t* c, size_t n, const uint64_t* host_t, uint64_t* host_out, unsigned max_blocks, hipStream_t st) {
  RedScratch* s = nullptr;
  if (int rc = red_scratch(current_device_ordinal(), &s)) return rc;
  std::lock_guard<std::mutex> lock(s->mu);
  unsigned cap = s->cap;
  if (max_blocks && max_blocks < cap) cap = max_blocks;
  const size_t runs = (n + POLY_RUN - 1) / POLY_RUN;
  const size_t want = (runs + RED_BLOCK - 1) / RED_BLOCK;
  const unsigned nb = (unsigned)(want < cap ? want : cap);
  uint32_t* res = s->p + RED_PARTIAL_WORDS;
  WireElem t;
  memcpy(t.w, host_t, 96);
  hipLaunchKernelGGL((k_poly_eval<M>), dim3(nb), dim3(RED_BLOCK), 0, st, c, n, t, s->p);
  hipLaunchKernelGGL((k_red_fold<M>), dim3(1), dim3(RED_BLOCK), 0, st, s->p, nb, 1, 0, res);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(host_out, res, 96, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

int vec_dot_impl(int curve, const uint64_t* dev_a, const uint64_t* dev_b, size_t n, uint64_t* host_out, unsigned max_blocks, void* stream) {
  if (curve < 0 || curve > 1 || !host_out || (n && (!dev_a || !dev_b))) return set_error(MNT753_EINVAL, "vec_dot: bad argument");
  if (int rc = require_device()) return rc;
  if (n == 0) {
    memset(host_out, 0, 96);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
  }
  const uint32_t* a = reinterpret_cast<const uint32_t*>(dev_a);
  const uint32_t* b = reinterpret_cast<const uint32_t*>(dev_b);
  return curve == MNT753_CURVE_MNT4753 ? dot_t<MOD_A>(&a, 1, b, n, host_out, max_blocks, (hipStream_t)stream)
                                       : dot_t<MOD_B>(&a, 1, b, n, host_out, max_blocks, (hipStream_t)stream);
}

int poly_eval_impl(int curve, const uint64_t* dev_coeffs, size_t n, const uint64_t* host_t, uint64_t* host_out, unsigned max_blocks, void* stream) {
  if (curve < 0 || curve > 1 || !host_t || !host_out || (n && !dev_coeffs)) return set_error(MNT753_EINVAL, "poly_eval: bad argument");
  if (!fr_canonical(curve == MNT753_CURVE_MNT4753 ? MOD_A : MOD_B, host_t)) return set_error(MNT753_EINVAL, "poly_eval: t is not a canonical element of Fr");
  if (int rc = require_device()) return rc;
  if (n == 0) {
    memset(host_out, 0, 96);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
  }
  const uint32_t* c = reinterpret_cast<const uint32_t*>(dev_coeffs);
  return curve == MNT753_CURVE_MNT4753 ? poly_t<MOD_A>(c, n, host_t, host_out, max_blocks, (hipStream_t)stream)
                                       : poly_t<MOD_B>(c, n, host_t, host_out, max_blocks, (hipStream_t)stream);
}

template <int M>
bool vanishes_t(const mnt753_domain* d, const uint64_t* host_t) { return vanishing_t<M>(d, HFp<M>::from_words(host_t)).is_zero(); }
bool vanishes(const mnt753_domain* d, const uint64_t* host_t) { return d->frm == MOD_A ? vanishes_t<MOD_A>(d, host_t) : vanishes_t<MOD_B>(d, host_t); }

// lhs = A B - C, rhs = Z H on the host
template <int M>
void h_verdict_t(const mnt753_domain* d, const uint64_t* host_t, const uint64_t* abc, const uint64_t* ht, mnt753_h_check_result* out) {
  typedef HFp<M> Fr;
  const Fr lhs = Fr::from_words(abc) * Fr::from_words(abc + 12) - Fr::from_words(abc + 24);
  const Fr rhs = vanishing_t<M>(d, Fr::from_words(host_t)) * Fr::from_words(ht);
  memcpy(out->lhs, lhs.l, 96);
  memcpy(out->rhs, rhs.l, 96);
  out->ok = lhs == rhs ? 1 : 0;
  out->reserved = 0;
}

}  // namespace

namespace mnt753 {
int vec_dot_capped(int curve, const uint64_t* dev_a, const uint64_t* dev_b, size_t n, uint64_t* host_out, unsigned max_blocks, void* stream) {
  return vec_dot_impl(curve, dev_a, dev_b, n, host_out, max_blocks, stream);
}
int poly_eval_capped(int curve, const uint64_t* dev_coeffs, size_t n, const uint64_t* host_t, uint64_t* host_out, unsigned max_blocks, void* stream) {
  return poly_eval_impl(curve, dev_coeffs, n, host_t, host_out, max_blocks, stream);
}
}  // namespace mnt753

extern "C" {

int mnt753_vec_dot(int curve, const uint64_t* dev_a, const uint64_t* dev_b, size_t n, uint64_t* host_out, void* stream) {
  return vec_dot_impl(curve, dev_a, dev_b, n, host_out, 0, stream);
}

int mnt753_poly_eval(int curve, const uint64_t* dev_coeffs, size_t n, const uint64_t* host_t, uint64_t* host_out, void* stream) {
  return poly_eval_impl(curve, dev_coeffs, n, host_t, host_out, 0, stream);
}

int mnt753_domain_interp_at(mnt753_domain* d, const uint64_t* host_t, const uint64_t* const* dev_vecs, int k, uint64_t* dev_u, uint64_t* host_out, void* stream) {
  if (!d || !host_t || !dev_vecs || k < 1 || k > 3 || !dev_u || !host_out) return set_error(MNT753_EINVAL, "domain_interp_at: bad argument");
  for (int j = 0; j < k; ++j)
    if (!dev_vecs[j]) return set_error(MNT753_EINVAL, "domain_interp_at: null vector");
  if (!fr_canonical(d->frm, host_t)) return set_error(MNT753_EINVAL, "domain_interp_at: t is not a canonical element of Fr");
  if (int rc = mnt753_domain_lagrange_at(d, host_t, dev_u, stream)) return rc;      // takes and releases the domain's work buffer
  OnDevice on(d->device);
  const uint32_t* u = reinterpret_cast<const uint32_t*>(dev_u);
  const uint32_t* v[3];
  for (int j = 0; j < k; ++j) v[j] = reinterpret_cast<const uint32_t*>(dev_vecs[j]);
  const hipStream_t st = (hipStream_t)stream;
  if (k == 3) return d->frm == MOD_A ? dot_t<MOD_A>(v, 3, u, d->m, host_out, 0, st) : dot_t<MOD_B>(v, 3, u, d->m, host_out, 0, st);
  for (int j = 0; j < k; ++j)
    if (int rc = d->frm == MOD_A ? dot_t<MOD_A>(v + j, 1, u, d->m, host_out + 12 * j, 0, st) : dot_t<MOD_B>(v + j, 1, u, d->m, host_out + 12 * j, 0, st)) return rc;
  return 0;
}

int mnt753_h_check(mnt753_domain* d, const uint64_t* host_t, const uint64_t* host_abc, const uint64_t* dev_h, mnt753_h_check_result* out, void* stream) {
  if (!d || !host_t || !host_abc || !dev_h || !out) return set_error(MNT753_EINVAL, "h_check: null argument");
  if (!fr_canonical(d->frm, host_t)) return set_error(MNT753_EINVAL, "h_check: t is not a canonical element of Fr");
  for (int j = 0; j < 3; ++j)
    if (!fr_canonical(d->frm, host_abc + 12 * j)) return set_error(MNT753_EINVAL, "h_check: A(t), B(t), C(t) must be canonical elements of Fr");
  if (vanishes(d, host_t)) return set_error(MNT753_EINVAL, "h_check: t is an element of the domain (Z(t) = 0: the identity would say nothing about H)");
  if (int rc = require_device()) return rc;
  OnDevice on(d->device);
  uint64_t ht[12];
  const uint32_t* h = reinterpret_cast<const uint32_t*>(dev_h);
  if (int rc = d->frm == MOD_A ? poly_t<MOD_A>(h, d->m + 1, host_t, ht, 0, (hipStream_t)stream) : poly_t<MOD_B>(h, d->m + 1, host_t, ht, 0, (hipStream_t)stream)) return rc;
  if (d->frm == MOD_A) h_verdict_t<MOD_A>(d, host_t, host_abc, ht, out);
  else h_verdict_t<MOD_B>(d, host_t, host_abc, ht, out);
  return 0;
}

int mnt753_compute_h_checked(mnt753_domain* d, uint64_t* dev_ca, uint64_t* dev_cb, uint64_t* dev_cc, uint64_t* dev_h, const uint64_t* host_t,
                             mnt753_h_check_result* out, void* stream) {
  if (!d || !dev_ca || !dev_cb || !dev_cc || !dev_h || !out) return set_error(MNT753_EINVAL, "compute_h_checked: null argument");
  uint64_t t[12];
  if (host_t) {
    if (!fr_canonical(d->frm, host_t)) return set_error(MNT753_EINVAL, "compute_h_checked: t is not a canonical element of Fr");
    if (vanishes(d, host_t)) return set_error(MNT753_EINVAL, "compute_h_checked: t is an element of the domain (Z(t) = 0: the identity would say nothing about H)");
    memcpy(t, host_t, 96);
  }
  if (int rc = require_device()) return rc;
  if (!host_t) {
    // 753 random bits, redrawn until they are below r (more than half of the draws are) and outside the domain
    for (int tries = 0;; ++tries) {
      if (tries == 256 || getrandom(t, sizeof t, 0) != (ssize_t)sizeof t) return set_error(MNT753_EINVAL, "compute_h_checked: no random t from getrandom");
      t[11] &= ((uint64_t)1 << (753 - 64 * 11)) - 1;
      if (fr_canonical(d->frm, t) && !vanishes(d, t)) break;
    }
  }
  // L(t) goes into dev_h, which compute_h writes only afterwards
  const uint64_t* vecs[3] = {dev_ca, dev_cb, dev_cc};
  uint64_t abc[36];
  if (int rc = mnt753_domain_interp_at(d, t, vecs, 3, dev_h, abc, stream)) return rc;
  if (int rc = mnt753_compute_h(d, dev_ca, dev_cb, dev_cc, dev_h, stream)) return rc;
  return mnt753_h_check(d, t, abc, dev_h, out, stream);
}

}  // extern "C"
