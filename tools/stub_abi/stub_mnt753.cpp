// TEST STUB of the C ABI (include/mnt753_hip.h) for the host-only sanitizer builds (`make asan`, `make tsan`): "device" memory is
// host memory, copies are memcpy, the file loader is fread -- and every compute entry point (MSM, FFT, compute_H, constraint
// evaluation) does NO arithmetic: an MSM returns the identity, a transform leaves its vector alone.  It exists so that the host
// side of the product (host/main.cpp, host/prover_hip_functions.cpp: loader threads, readiness latches, per-device slices,
// sharded folds, error paths) can run under AddressSanitizer / UBSan / ThreadSanitizer on a machine without a GPU (GPU sanitizers
// are not available on the pool).  It is never linked into the product, the tests of results, or the bench; a binary built on it
// writes the proof of the all-identity MSMs, which nothing compares with anything.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/mnt753_hip.h"
#include "../../snark-challenge-prover-reference_amd/csrc/host_field.hpp"
#include "../../snark-challenge-prover-reference_amd/csrc/point_stream.hpp"

using namespace mnt753;
using namespace mnt753::host;

namespace {
thread_local std::string t_err;
thread_local int t_dev = 0;
int g_ndev = 0;
std::mutex g_io[16];
int fail(int code, const char* msg) { t_err = msg; return code; }
bool bad_cg(int curve, int group) { return curve < 0 || curve > 1 || (group != MNT753_G1 && group != MNT753_G2); }
int deg_of(int curve, int group) { return group == MNT753_G1 ? 1 : (curve == 0 ? 2 : 3); }
template <class HC> int add_t(const uint64_t* a, const uint64_t* b, uint64_t* o) { HPoint<HC>::from_wire(a).add(HPoint<HC>::from_wire(b)).to_wire(o); return 0; }
template <class HC> int scale_t(const uint64_t* s, const uint64_t* p, uint64_t* o) {
  uint64_t e[12]; HFp<HC::FR>::from_words(s).to_integer(e); HPoint<HC>::from_wire(p).mul_words(e, 12).to_wire(o); return 0;
}
template <class HC> int aff_t(const uint64_t* p, uint64_t* o) {
  typename HC::F x, y; HPoint<HC>::from_wire(p).to_affine(x, y);
  for (int k = 0; k < HC::F::DEG; ++k) { memcpy(o + 12 * k, x.comp(k).l, 96); memcpy(o + 12 * (HC::F::DEG + k), y.comp(k).l, 96); }
  return 0;
}
template <class HC> int from_aff_t(const uint64_t* a, uint64_t* o) {
  typedef typename HC::F F; HPoint<HC> p;
  for (int k = 0; k < F::DEG; ++k) { p.X.comp(k) = F::B::from_words(a + 12 * k); p.Y.comp(k) = F::B::from_words(a + 12 * (F::DEG + k)); }
  if (p.Y.is_zero()) p = HPoint<HC>::zero(); else p.Z = F::one();
  p.to_wire(o); return 0;
}
template <class HC> int zero_t(uint64_t* o) { HPoint<HC>::zero().to_wire(o); return 0; }
}  // namespace
#define CG(fn, ...) (curve == 0 ? (group == MNT753_G1 ? fn<HMnt4G1>(__VA_ARGS__) : fn<HMnt4G2>(__VA_ARGS__)) : (group == MNT753_G1 ? fn<HMnt6G1>(__VA_ARGS__) : fn<HMnt6G2>(__VA_ARGS__)))

struct mnt753_bases { int curve, group, device; size_t n; void* copy; int pending; size_t pending_n; };
struct mnt753_domain { int curve; size_t m; int device; };
struct mnt753_r1cs { uint64_t num_inputs, m, nc; };

extern "C" {
int mnt753_init(int device) { if (device != 0) return fail(MNT753_EINVAL, "stub: one device"); if (g_ndev < 1) g_ndev = 1; t_dev = 0; return 0; }
int mnt753_init_devices(int n) { if (n < 1 || n > 16) return fail(MNT753_EINVAL, "mnt753_init_devices: more devices requested than visible"); g_ndev = n; t_dev = 0; return 0; }
int mnt753_device_count(void) { return g_ndev; }
int mnt753_set_device(int d) { if (d < 0 || d >= g_ndev) return fail(MNT753_EINVAL, "mnt753_set_device: not an initialised device"); t_dev = d; return 0; }
int mnt753_get_device(void) { return t_dev; }
// peer access: the stub's devices are host memory; every request is recorded on stderr under MNT753_TRACE=1 so that the sanitizer
// suite can assert that the wrapper asks for every ordered pair
int mnt753_enable_peer_access(int a, int b, int* how) {
  if (a < 0 || a >= g_ndev || b < 0 || b >= g_ndev) return fail(MNT753_EINVAL, "enable_peer_access: not an initialised device");
  if (const char* e = getenv("MNT753_TRACE")) { if (atoi(e)) fprintf(stderr, "stub: peer access requested %d -> %d\n", a, b); }
  if (how) *how = MNT753_PEER_SAME;
  return 0;
}
int mnt753_copy_peer(int, void* d, int, const void* s, size_t n) { if (n) memcpy(d, s, n); return 0; }
int mnt753_copy_peer_async(int dd, void* d, int sd, const void* s, size_t n) { if (dd < 0 || dd >= g_ndev || sd < 0 || sd >= g_ndev) return fail(MNT753_EINVAL, "copy_peer_async: bad device"); if (n) memcpy(d, s, n); return 0; }
const char* mnt753_last_error(void) { return t_err.c_str(); }
// the exchange: a plain copy (the stub's "devices" are host memory); MNT753_STUB_NO_RCCL=1 plays a box without librccl
int mnt753_exchange_points(const uint64_t* const* in, size_t words, uint64_t* out) {
  if (!in || !out || !words) return fail(MNT753_EINVAL, "exchange_points: bad argument");
  if (getenv("MNT753_STUB_NO_RCCL")) return fail(MNT753_ENODEV, "exchange_points: cannot load librccl (stub)");
  for (int g = 0; g < g_ndev; ++g) { if (!in[g]) return fail(MNT753_EINVAL, "exchange_points: null block"); memcpy(out + words * (size_t)g, in[g], 8 * words); }
  return 0;
}
double mnt753_exchange_last_us(void) { return 1.0; }
size_t mnt753_affine_words(int curve, int group) { return bad_cg(curve, group) ? 0 : (size_t)24 * deg_of(curve, group); }
size_t mnt753_projective_words(int curve, int group) { return bad_cg(curve, group) ? 0 : (size_t)36 * deg_of(curve, group); }
int mnt753_dev_alloc(void** p, size_t n) { if (!g_ndev) return fail(MNT753_ENODEV, "no device"); *p = malloc(n ? n : 16); return *p ? 0 : fail(MNT753_ENOMEM, "alloc"); }
int mnt753_dev_free(void* p) { free(p); return 0; }
int mnt753_copy_h2d(void* d, const void* s, size_t n) { if (n) memcpy(d, s, n); return 0; }
int mnt753_copy_d2h(void* d, const void* s, size_t n) { if (n) memcpy(d, s, n); return 0; }
int mnt753_copy_d2d(void* d, const void* s, size_t n) { if (n) memmove(d, s, n); return 0; }
int mnt753_dev_memset(void* d, int v, size_t n) { if (n) memset(d, v, n); return 0; }
int mnt753_sync(void*) { return 0; }
int mnt753_load_file_to_device(const char* path, size_t off, size_t bytes, void* dst) {
  if (!g_ndev) return fail(MNT753_ENODEV, "no device");
  std::lock_guard<std::mutex> l(g_io[t_dev & 15]);   // the product serialises a device's staging buffers the same way
  FILE* f = fopen(path, "rb");
  if (!f) return fail(MNT753_EINVAL, "load_file_to_device: cannot open file");
  int rc = 0;
  if (fseeko(f, (off_t)off, SEEK_SET) != 0 || (bytes && fread(dst, 1, bytes, f) != bytes)) rc = fail(MNT753_EINVAL, "load_file_to_device: short read");
  fclose(f);
  return rc;
}
int mnt753_bases_create(int curve, int group, const uint64_t* aff, int, size_t n, mnt753_bases** out) {
  if (!out || (n && !aff) || bad_cg(curve, group)) return fail(MNT753_EINVAL, "bases_create: bad argument");
  if (!g_ndev) return fail(MNT753_ENODEV, "no device");
  mnt753_bases* b = new mnt753_bases{curve, group, t_dev, n, nullptr, 0, 0};
  const size_t bytes = n * mnt753_affine_words(curve, group) * 8;
  b->copy = malloc(bytes ? bytes : 16);
  if (bytes) memcpy(b->copy, aff, bytes);       // reads every byte the caller promised: ASan checks the caller's buffer
  *out = b; return 0;
}
int mnt753_bases_free(mnt753_bases* b) { if (b) { free(b->copy); delete b; } return 0; }
size_t mnt753_bases_size(const mnt753_bases* b) { return b ? b->n : 0; }
int mnt753_msm_start(mnt753_bases* b, size_t off, const uint64_t* sc, int, size_t n, void*) {
  if (!b || (n && !sc)) return fail(MNT753_EINVAL, "msm_start: null argument");
  if (off + n > b->n) return fail(MNT753_EINVAL, "msm_start: base_offset + n exceeds the base set");
  if (b->pending) return fail(MNT753_EINVAL, "msm_start: this base set already has an MSM in flight (finish it first)");
  volatile uint64_t sink = 0;
  for (size_t i = 0; i < 12 * n; i += 12) sink += sc[i];   // touch the scalar range: ASan / TSan see the access the kernels would make
  (void)sink;
  b->pending = 1; b->pending_n = n; return 0;
}
int mnt753_msm_finish(mnt753_bases* b, uint64_t* out) {
  if (!b || !out) return fail(MNT753_EINVAL, "msm_finish: null argument");
  if (!b->pending) return fail(MNT753_EINVAL, "msm_finish: no MSM in flight on this base set");
  b->pending = 0;
  const int curve = b->curve, group = b->group;
  return CG(zero_t, out);
}
int mnt753_msm(mnt753_bases* b, size_t off, const uint64_t* sc, int od, size_t n, uint64_t* out, void* st) {
  if (int rc = mnt753_msm_start(b, off, sc, od, n, st)) return rc;
  return mnt753_msm_finish(b, out);
}
int mnt753_msm_set_window_bits(int) { return 0; }
int mnt753_dev_mem_info(size_t* f, size_t* t) { if (f) *f = (size_t)200 << 30; if (t) *t = (size_t)288 << 30; return 0; }
int mnt753_self_test_curve(int curve, int level) { if (getenv("MNT753_STUB_LOG")) fprintf(stderr, "stub: self-test level %d curve %d\n", level, curve); const char* e = getenv("MNT753_STUB_SELFTEST_FAILS"); return e && atoi(e) ? fail(MNT753_ESELFTEST, "stub: self-test check 3 failed (as asked)") : 0; }
int mnt753_self_test(int level) { if (getenv("MNT753_STUB_LOG")) fprintf(stderr, "stub: self-test level %d\n", level); const char* e = getenv("MNT753_STUB_SELFTEST_FAILS"); return e && atoi(e) ? fail(MNT753_ESELFTEST, "stub: self-test check 3 failed (as asked)") : 0; }
int mnt753_msm_set_window_table(int mode) { static int m = 1; const int old = m; m = mode != 0; if (getenv("MNT753_STUB_LOG")) fprintf(stderr, "stub: window table mode %d\n", m); return old; }
int mnt753_msm_order_after(mnt753_bases* b, const mnt753_bases* first) { return (b && first && b != first) ? 0 : 22; }
int mnt753_msm_last_timing(float o[5]) { for (int i = 0; i < 5; ++i) o[i] = 0; return 0; }
int mnt753_msm_last_plan(int o[4]) { for (int i = 0; i < 4; ++i) o[i] = 0; return 0; }
int mnt753_msm_last_pair_levels(void) { return 0; }
int mnt753_msm_last_irr_levels(void) { return 0; }
int mnt753_point_add(int curve, int group, const uint64_t* a, const uint64_t* b, uint64_t* o) { if (bad_cg(curve, group)) return fail(MNT753_EINVAL, "point_add"); return CG(add_t, a, b, o); }
int mnt753_point_scale(int curve, int group, const uint64_t* s, const uint64_t* p, uint64_t* o) { if (bad_cg(curve, group)) return fail(MNT753_EINVAL, "point_scale"); return CG(scale_t, s, p, o); }
int mnt753_point_to_affine(int curve, int group, const uint64_t* p, uint64_t* o) { if (bad_cg(curve, group)) return fail(MNT753_EINVAL, "point_to_affine"); return CG(aff_t, p, o); }
int mnt753_point_from_affine(int curve, int group, const uint64_t* a, uint64_t* o) { if (bad_cg(curve, group)) return fail(MNT753_EINVAL, "point_from_affine"); return CG(from_aff_t, a, o); }
int mnt753_domain_create(int curve, size_t m, mnt753_domain** out) {
  if (!out || curve < 0 || curve > 1 || m == 0 || (m & (m - 1))) return fail(MNT753_EDOMAIN, "domain_create: not a power of two");
  *out = new mnt753_domain{curve, m, t_dev}; return 0;
}
// (the stub has no arithmetic: any size above 1 is taken as it is, which is all the wrapper's plumbing needs)
int mnt753_domain_create_for(int curve, size_t min_size, mnt753_domain** out) {
  if (!out || curve < 0 || curve > 1) return fail(MNT753_EINVAL, "domain_create_for: bad argument");
  if (min_size <= 1) return fail(MNT753_EDOMAIN, "domain_create_for: min_size must be above 1");
  *out = new mnt753_domain{curve, min_size, t_dev}; return 0;
}
int mnt753_domain_create_for_ex(int curve, size_t min_size, unsigned flags, mnt753_domain** out) {
  if (flags & ~MNT753_DOMAIN_ALLOW_MIXED) return fail(MNT753_EINVAL, "domain_create_for: bad argument");
  return mnt753_domain_create_for(curve, min_size, out);
}
int mnt753_domain_create_mixed(int curve, size_t m, mnt753_domain** out) {
  if (!out || curve != MNT753_CURVE_MNT6753 || m <= 1 || m % 5) return fail(MNT753_EDOMAIN, "domain_create_mixed: not 2^a 5^b on MNT6753");
  *out = new mnt753_domain{curve, m, t_dev}; return 0;
}
int mnt753_domain_kind(const mnt753_domain* d) { return !d ? -1 : (d->m & (d->m - 1)) ? MNT753_DOMAIN_STEP : MNT753_DOMAIN_BASIC; }
int mnt753_domain_free(mnt753_domain* d) { delete d; return 0; }
size_t mnt753_domain_size(const mnt753_domain* d) { return d ? d->m : 0; }
static void touch(uint64_t* v, size_t n) { volatile uint64_t s = 0; for (size_t i = 0; i < 12 * n; i += 12) { s += v[i]; v[i] = v[i]; } (void)s; }
int mnt753_fft(mnt753_domain* d, int, uint64_t* v, void*) { if (!d || !v) return fail(MNT753_EINVAL, "fft: null"); touch(v, d->m); return 0; }
int mnt753_divide_by_z_on_coset(mnt753_domain* d, uint64_t* v, void*) { if (!d || !v) return fail(MNT753_EINVAL, "divide_by_z: null"); touch(v, d->m); return 0; }
int mnt753_vec_muleq(int, uint64_t* a, const uint64_t* b, size_t n, void*) { touch(a, n); touch(const_cast<uint64_t*>(b), n); return 0; }
int mnt753_vec_scale(int, uint64_t* d, const uint64_t* s, const uint64_t* k, size_t n, void*) { touch(const_cast<uint64_t*>(s), n); touch(d, n); return k ? 0 : -2; }
int mnt753_vec_subeq(int, uint64_t* a, const uint64_t* b, size_t n, void*) { touch(a, n); touch(const_cast<uint64_t*>(b), n); return 0; }
int mnt753_compute_h(mnt753_domain* d, uint64_t* a, uint64_t* b, uint64_t* c, uint64_t* h, void*) {
  if (!d || !a || !b || !c || !h) return fail(MNT753_EINVAL, "compute_h: null");
  touch(a, d->m); touch(b, d->m); touch(c, d->m); memset(h, 0, 96 * (d->m + 1)); return 0;
}
int mnt753_compute_h_chain(mnt753_domain* d, uint64_t* v, void*) { if (!d || !v) return fail(MNT753_EINVAL, "compute_h_chain: null"); touch(v, d->m); return 0; }
int mnt753_compute_h_finish(mnt753_domain* d, uint64_t* a, const uint64_t* b, const uint64_t* c, uint64_t* h, void*) {
  if (!d || !a || !b || !c || !h) return fail(MNT753_EINVAL, "compute_h_finish: null");
  touch(a, d->m); touch(const_cast<uint64_t*>(b), d->m); touch(const_cast<uint64_t*>(c), d->m); memset(h, 0, 96 * (d->m + 1)); return 0;
}
int mnt753_domain_device(const mnt753_domain* d) { return d ? d->device : -1; }
int mnt753_r1cs_create(int curve, uint64_t ni, uint64_t m, uint64_t nc, const uint64_t* const rp[3], const uint32_t* const col[3], const uint64_t* const cf[3], mnt753_r1cs** out) {
  if (curve < 0 || curve > 1 || !out || !rp || !col || !cf || ni > m) return fail(MNT753_EINVAL, "r1cs_create: bad argument");
  for (int k = 0; k < 3; ++k) for (uint64_t i = 0; i < rp[k][nc]; ++i) if (col[k][i] > m) return fail(MNT753_EINVAL, "r1cs_create: variable index out of range");
  *out = new mnt753_r1cs{ni, m, nc}; return 0;
}
int mnt753_r1cs_free(mnt753_r1cs* r) { delete r; return 0; }
size_t mnt753_r1cs_domain_size(const mnt753_r1cs* r) { return r ? (size_t)(r->nc + r->num_inputs + 1) : 0; }
size_t mnt753_r1cs_num_variables(const mnt753_r1cs* r) { return r ? (size_t)r->m : 0; }
size_t mnt753_r1cs_num_inputs(const mnt753_r1cs* r) { return r ? (size_t)r->num_inputs : 0; }
int mnt753_r1cs_evaluate(mnt753_r1cs* r, const uint64_t* w, uint64_t* a, uint64_t* b, uint64_t* c, size_t n, void*) {
  if (!r || !w || !a || !b || !c) return fail(MNT753_EINVAL, "r1cs_evaluate: null");
  touch(const_cast<uint64_t*>(w), r->m + 1); memset(a, 0, 96 * n); memset(b, 0, 96 * n); memset(c, 0, 96 * n); return 0;
}
// input validation: no arithmetic here either, so every input is "good" -- unless MNT753_STUB_BAD_POINT=<index> asks for one bad
// point (off curve) at that index of every point set long enough to have it, MNT753_STUB_BAD_ROW=<row> for one unsatisfied row.
// The ranges are touched like everywhere else: ASan / TSan see the reads the kernels would make.
static void touch_ro(const uint64_t* v, size_t words) { volatile uint64_t s = 0; for (size_t i = 0; i < words; i += 12) s += v[i]; (void)s; }
static void stub_report(mnt753_check_report* out, const char* env, size_t n, uint32_t reason) {
  *out = mnt753_check_report{0, 0, MNT753_BAD_NONE, 0};
  const char* e = getenv(env);
  if (e && *e && strtoull(e, nullptr, 0) < n) *out = mnt753_check_report{1, strtoull(e, nullptr, 0), reason, 0};
}
int mnt753_check_points(int curve, int group, const uint64_t* aff, int, size_t n, mnt753_check_report* out, void*) {
  if (bad_cg(curve, group) || !out || (n && !aff)) return fail(MNT753_EINVAL, "check_points: bad argument");
  if (!g_ndev) return fail(MNT753_ENODEV, "no device");
  touch_ro(aff, n * mnt753_affine_words(curve, group));
  stub_report(out, "MNT753_STUB_BAD_POINT", n, MNT753_BAD_OFF_CURVE);
  return 0;
}
// the subgroup test: G1 is check_points' own result; on G2 MNT753_STUB_BAD_SUBGROUP=<index> asks for one point outside the subgroup at
// that index of every G2 set long enough to have it (MNT753_STUB_BAD_POINT, an earlier reason, wins where both name a point)
int mnt753_check_subgroup(int curve, int group, const uint64_t* aff, int od, size_t n, mnt753_check_report* out, void* st) {
  if (bad_cg(curve, group) || !out || (n && !aff)) return fail(MNT753_EINVAL, "check_subgroup: bad argument");
  if (int rc = mnt753_check_points(curve, group, aff, od, n, out, st)) return rc;
  if (group == MNT753_G1 || out->n_bad) return 0;
  stub_report(out, "MNT753_STUB_BAD_SUBGROUP", n, MNT753_BAD_NOT_IN_SUBGROUP);
  return 0;
}
int mnt753_check_scalars(int curve, const uint64_t* fr, int, size_t n, mnt753_check_report* out, void*) {
  if (curve < 0 || curve > 1 || !out || (n && !fr)) return fail(MNT753_EINVAL, "check_scalars: bad argument");
  if (!g_ndev) return fail(MNT753_ENODEV, "no device");
  touch_ro(fr, 12 * n);
  *out = mnt753_check_report{0, 0, MNT753_BAD_NONE, 0};
  return 0;
}
int mnt753_check_products(int curve, const uint64_t* a, const uint64_t* b, const uint64_t* c, size_t n, mnt753_check_report* out, void*) {
  if (curve < 0 || curve > 1 || !out || (n && (!a || !b || !c))) return fail(MNT753_EINVAL, "check_products: bad argument");
  if (!g_ndev) return fail(MNT753_ENODEV, "no device");
  touch_ro(a, 12 * n); touch_ro(b, 12 * n); touch_ro(c, 12 * n);
  stub_report(out, "MNT753_STUB_BAD_ROW", n, MNT753_BAD_UNSATISFIED);
  return 0;
}
// the QAP at a point: the stub writes zeros (no arithmetic), with the refusals of the product
int mnt753_domain_vanishing_at(mnt753_domain* d, const uint64_t* t, uint64_t* zt) { if (!d || !t || !zt) return fail(MNT753_EINVAL, "domain_vanishing_at: null argument"); memset(zt, 0, 96); return 0; }
int mnt753_domain_lagrange_at(mnt753_domain* d, const uint64_t* t, uint64_t* u, void*) { if (!d || !t || !u) return fail(MNT753_EINVAL, "domain_lagrange_at: null argument"); memset(u, 0, 96 * d->m); return 0; }
int mnt753_vec_powers(int curve, const uint64_t* t, uint64_t* out, size_t n, void*) { if (curve < 0 || curve > 1 || !t || (n && !out)) return fail(MNT753_EINVAL, "vec_powers: bad argument"); if (n) memset(out, 0, 96 * n); return 0; }
int mnt753_vec_dot(int curve, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, void*) {
  if (curve < 0 || curve > 1 || !out || (n && (!a || !b))) return fail(MNT753_EINVAL, "vec_dot: bad argument");
  if (!g_ndev) return fail(MNT753_ENODEV, "no device");
  touch_ro(a, 12 * n); touch_ro(b, 12 * n); memset(out, 0, 96); return 0;
}
int mnt753_poly_eval(int curve, const uint64_t* c, size_t n, const uint64_t* t, uint64_t* out, void*) {
  if (curve < 0 || curve > 1 || !t || !out || (n && !c)) return fail(MNT753_EINVAL, "poly_eval: bad argument");
  if (!g_ndev) return fail(MNT753_ENODEV, "no device");
  touch_ro(c, 12 * n); memset(out, 0, 96); return 0;
}
int mnt753_domain_interp_at(mnt753_domain* d, const uint64_t* t, const uint64_t* const* vecs, int k, uint64_t* u, uint64_t* out, void*) {
  if (!d || !t || !vecs || k < 1 || k > 3 || !u || !out) return fail(MNT753_EINVAL, "domain_interp_at: bad argument");
  for (int j = 0; j < k; ++j) { if (!vecs[j]) return fail(MNT753_EINVAL, "domain_interp_at: null vector"); touch_ro(vecs[j], 12 * d->m); }
  memset(u, 0, 96 * d->m); memset(out, 0, 96 * (size_t)k); return 0;
}
int mnt753_h_check(mnt753_domain* d, const uint64_t* t, const uint64_t* abc, const uint64_t* h, mnt753_h_check_result* out, void*) {
  if (!d || !t || !abc || !h || !out) return fail(MNT753_EINVAL, "h_check: null argument");
  touch_ro(h, 12 * (d->m + 1)); touch_ro(abc, 36); memset(out, 0, sizeof *out); out->ok = 1; return 0;
}
int mnt753_compute_h_checked(mnt753_domain* d, uint64_t* a, uint64_t* b, uint64_t* c, uint64_t* h, const uint64_t* t, mnt753_h_check_result* out, void* st) {
  if (!d || !a || !b || !c || !h || !out) return fail(MNT753_EINVAL, "compute_h_checked: null argument");
  if (t) touch_ro(t, 12);
  if (int rc = mnt753_compute_h(d, a, b, c, h, st)) return rc;
  memset(out, 0, sizeof *out); out->ok = 1; return 0;
}
int mnt753_r1cs_qap_plan(const mnt753_r1cs* r, mnt753_qap_plan* out) { if (!r || !out) return fail(MNT753_EINVAL, "r1cs_qap_plan: null argument"); memset(out, 0, sizeof *out); out->chunk_terms = 256; return 0; }
int mnt753_r1cs_qap_at(mnt753_r1cs* r, mnt753_domain* d, const uint64_t* t, uint64_t* at, uint64_t* bt, uint64_t* ct, uint64_t* ht, uint64_t* zt, void*) {
  if (!r || !d || !t || !at || !bt || !ct || !ht || !zt) return fail(MNT753_EINVAL, "r1cs_qap_at: null argument");
  if (d->m < r->nc + r->num_inputs + 1) return fail(MNT753_EINVAL, "r1cs_qap_at: domain below constraints + inputs + 1");
  memset(at, 0, 96 * (r->m + 1)); memset(bt, 0, 96 * (r->m + 1)); memset(ct, 0, 96 * (r->m + 1)); memset(ht, 0, 96 * (d->m + 1)); memset(zt, 0, 96);
  return 0;
}
int mnt753_r1cs_check(mnt753_r1cs* r, const uint64_t* w, mnt753_check_report* out, void*) {
  if (!r || !w || !out) return fail(MNT753_EINVAL, "r1cs_check: null argument");
  touch_ro(w, 12 * (r->m + 1));
  stub_report(out, "MNT753_STUB_BAD_ROW", r->nc, MNT753_BAD_UNSATISFIED);
  return 0;
}
int mnt753_synth_scalars(int, uint64_t seed, size_t n, uint64_t* out) { for (size_t i = 0; i < 12 * n; ++i) out[i] = seed + i; return 0; }
// the pairing and verification: sizes and argument checks only (no arithmetic: every proof is "accepted" unless MNT753_STUB_REJECT is set)
struct mnt753_vk { int curve; size_t num_inputs; };
size_t mnt753_gt_words(int curve) { return curve == 0 ? 48 : (curve == 1 ? 72 : 0); }
int mnt753_pairing(int curve, const uint64_t* g1, const uint64_t* g2, size_t n, int, uint64_t* out, void*) {
  if (curve < 0 || curve > 1 || (n && (!g1 || !g2 || !out))) return fail(MNT753_EINVAL, "pairing: bad argument");
  if (!g_ndev) return fail(MNT753_ENODEV, "no device");
  touch_ro(g1, 24 * n); touch_ro(g2, n * mnt753_affine_words(curve, MNT753_G2));
  for (size_t i = 0; i < n * mnt753_gt_words(curve); ++i) out[i] = i;
  return 0;
}
int mnt753_vk_create(int curve, const uint64_t* a, const uint64_t* b, const uint64_t* d, const uint64_t* abc, size_t num_inputs, mnt753_vk** out) {
  if (curve < 0 || curve > 1 || !a || !b || !d || !abc || !out) return fail(MNT753_EINVAL, "vk_create: bad argument");
  if (!g_ndev) return fail(MNT753_ENODEV, "no device");
  touch_ro(a, 24); touch_ro(b, mnt753_affine_words(curve, MNT753_G2)); touch_ro(d, mnt753_affine_words(curve, MNT753_G2)); touch_ro(abc, 24 * (num_inputs + 1));
  *out = new mnt753_vk{curve, num_inputs};
  return 0;
}
int mnt753_vk_destroy(mnt753_vk* vk) { delete vk; return 0; }
size_t mnt753_vk_num_inputs(const mnt753_vk* vk) { return vk ? vk->num_inputs : 0; }
size_t mnt753_vk_coefficient_bytes(const mnt753_vk* vk) { return vk ? 1024 : 0; }
int mnt753_vk_set_workspace_cap(mnt753_vk* vk, size_t) { return vk ? 0 : fail(MNT753_EINVAL, "vk_set_workspace_cap: bad argument"); }
int mnt753_vk_gt(const mnt753_vk* vk, uint64_t* out) {
  if (!vk || !out) return fail(MNT753_EINVAL, "vk_gt: bad argument");
  for (size_t i = 0; i < mnt753_gt_words(vk->curve); ++i) out[i] = i;
  return 0;
}
int mnt753_vk_serialize(const mnt753_vk* vk, uint8_t* buf, size_t cap, size_t* len) {
  if (!vk || !len) return fail(MNT753_EINVAL, "vk_serialize: bad argument");
  *len = 8 * mnt753_gt_words(vk->curve) + 16;
  if (!buf) return 0;
  if (cap < *len) return fail(MNT753_EINVAL, "vk_serialize: buffer too small");
  for (size_t i = 0; i < *len; ++i) buf[i] = (uint8_t)i;
  return 0;
}
int mnt753_vk_accumulate(const mnt753_vk* vk, const uint64_t* inputs, size_t n, uint64_t* out) {
  if (!vk || (n && !out)) return fail(MNT753_EINVAL, "vk_accumulate: bad argument");
  touch_ro(inputs, 12 * vk->num_inputs * n);
  for (size_t i = 0; i < 24 * n; ++i) out[i] = i;
  return 0;
}
// input tables: no table, the plan of the widths asked for (default: 4); the refusals of the product
int mnt753_vk_prepare_inputs(mnt753_vk* vk, int window_bits, size_t) {
  if (!vk || !vk->num_inputs || (window_bits && (window_bits < 2 || window_bits > 16))) return fail(MNT753_EINVAL, "vk_prepare_inputs: bad argument");
  return 0;
}
int mnt753_vk_input_plan(const mnt753_vk* vk, size_t, mnt753_vk_input_plan_t* out) {
  if (!vk || !out) return fail(MNT753_EINVAL, "vk_input_plan: bad argument");
  *out = mnt753_vk_input_plan_t{4, 189, 1u, 0u, (uint64_t)(vk->num_inputs + 1) * 189 * 8 * 256, 1, 0};
  return 0;
}
int mnt753_vk_release_inputs(mnt753_vk* vk) { return vk ? 0 : fail(MNT753_EINVAL, "vk_release_inputs: bad argument"); }
// with MNT753_VERIFY_CHECK_SUBGROUP, MNT753_STUB_BAD_B=<index> gives that proof verdict 3
int mnt753_groth16_verify_ex(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int, unsigned flags, uint8_t* verdicts, void*) {
  if (!vk || (n && (!proofs || !verdicts)) || (flags & ~MNT753_VERIFY_CHECK_SUBGROUP)) return fail(MNT753_EINVAL, "groth16_verify: bad argument");
  touch_ro(proofs, n * (48 + mnt753_affine_words(vk->curve, MNT753_G2))); touch_ro(inputs, 12 * vk->num_inputs * n);
  const int reject = getenv("MNT753_STUB_REJECT") != nullptr;
  const char* e = (flags & MNT753_VERIFY_CHECK_SUBGROUP) ? getenv("MNT753_STUB_BAD_B") : nullptr;
  const size_t bad_b = e && *e ? strtoull(e, nullptr, 0) : n;
  int rejected = 0;
  for (size_t i = 0; i < n; ++i) { verdicts[i] = i == bad_b ? 3 : (reject ? 2 : 0); rejected += verdicts[i] != 0; }
  return rejected;
}
int mnt753_groth16_verify(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int od, uint8_t* verdicts, void* st) {
  return mnt753_groth16_verify_ex(vk, proofs, inputs, n, od, 0u, verdicts, st);
}
// compressed points: no arithmetic -- compress copies x and gives flag 0 (2 for y = 0), decompress copies x back and writes y = x
// (a point whose words are not zero); MNT753_STUB_BAD_POINT=<index> makes that element of a long enough set BAD_OFF_CURVE, as in
// mnt753_check_points.  The stream records are the product's own codec (csrc/point_stream.hpp: bytes only).
size_t mnt753_compressed_words(int curve, int group) { return bad_cg(curve, group) ? 0 : mnt753_affine_words(curve, group) / 2; }
int mnt753_compress_points(int curve, int group, const uint64_t* aff, int, size_t n, uint64_t* x, uint8_t* flags, void*) {
  if (bad_cg(curve, group) || (n && (!aff || !x || !flags))) return fail(MNT753_EINVAL, "compress_points: bad argument");
  if (!g_ndev) return fail(MNT753_ENODEV, "no device");
  const size_t wx = mnt753_compressed_words(curve, group);
  for (size_t i = 0; i < n; ++i) {
    uint64_t yor = 0;
    for (size_t k = 0; k < wx; ++k) yor |= aff[(2 * i + 1) * wx + k];
    for (size_t k = 0; k < wx; ++k) x[i * wx + k] = yor ? aff[2 * i * wx + k] : 0;
    flags[i] = yor ? 0 : 2;
  }
  return 0;
}
int mnt753_decompress_points(int curve, int group, const uint64_t* x, const uint8_t* flags, int, size_t n, uint64_t* aff, mnt753_check_report* out, void*) {
  if (bad_cg(curve, group) || !out || (n && (!x || !flags || !aff))) return fail(MNT753_EINVAL, "decompress_points: bad argument");
  if (!g_ndev) return fail(MNT753_ENODEV, "no device");
  const size_t wx = mnt753_compressed_words(curve, group);
  *out = mnt753_check_report{0, 0, MNT753_BAD_NONE, 0};
  stub_report(out, "MNT753_STUB_BAD_POINT", n, MNT753_BAD_OFF_CURVE);
  for (size_t i = 0; i < n; ++i) {
    const bool zero = (flags[i] & 2u) || (out->n_bad && out->first_bad == i);
    for (size_t k = 0; k < wx; ++k) aff[2 * i * wx + k] = aff[(2 * i + 1) * wx + k] = zero ? 0 : (x[i * wx + k] | 1u);
  }
  return 0;
}
int mnt753_groth16_verify_compressed(const mnt753_vk* vk, const uint64_t* x, const uint8_t* flags, const uint64_t* inputs, size_t n, int od, unsigned vflags,
                                     uint8_t* verdicts, void* st) {
  if (!vk || (n && (!x || !flags || !verdicts)) || (vflags & ~MNT753_VERIFY_CHECK_SUBGROUP)) return fail(MNT753_EINVAL, "groth16_verify_compressed: bad argument");
  const size_t xw = 24 + mnt753_compressed_words(vk->curve, MNT753_G2);
  touch_ro(x, n * xw);
  std::string proofs(8 * n * (48 + mnt753_affine_words(vk->curve, MNT753_G2)) + 8, '\1');   // what a decompressed batch would be
  int rc = mnt753_groth16_verify_ex(vk, reinterpret_cast<const uint64_t*>(proofs.data()), inputs, n, od, vflags, verdicts, st);
  if (rc < 0) return rc;
  rc = 0;
  for (size_t i = 0; i < n; ++i) {               // an identity flag or an unknown flag bit on A, B or C: malformed
    if ((flags[3 * i] | flags[3 * i + 1] | flags[3 * i + 2]) & 0xfeu) verdicts[i] = 1;
    rc += verdicts[i] != 0;
  }
  return rc;
}
int mnt753_points_to_stream(int curve, int group, const uint64_t* x, const uint8_t* flags, size_t n, uint8_t* buf, size_t cap, size_t* len) {
  if (bad_cg(curve, group) || !len || (n && (!x || !flags))) return fail(MNT753_EINVAL, "points_to_stream: bad argument");
  const size_t xb = 8 * mnt753_compressed_words(curve, group);
  *len = n * (xb + 2);
  if (!buf) return 0;
  if (cap < *len) return fail(MNT753_EINVAL, "points_to_stream: buffer too small");
  return stream_write(xb, x, flags, n, buf) == STREAM_OK ? 0 : fail(MNT753_EINVAL, "points_to_stream: a flag byte has a bit above the identity flag set");
}
int mnt753_points_from_stream(int curve, int group, const uint8_t* buf, size_t len, size_t n, uint64_t* x, uint8_t* flags) {
  if (bad_cg(curve, group) || (n && (!buf || !x || !flags))) return fail(MNT753_EINVAL, "points_from_stream: bad argument");
  return stream_read(8 * mnt753_compressed_words(curve, group), buf, len, n, x, flags) == STREAM_OK
             ? 0 : fail(MNT753_EINVAL, "points_from_stream: not n well-formed records");
}
// MNT753_STUB_REJECT rejects the fold as it rejects every proof
int mnt753_groth16_verify_folded(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int, const uint64_t* coefficients, uint8_t* status,
                                 int* accepted, void*) {
  if (!vk || !accepted || (n && (!proofs || !coefficients))) return fail(MNT753_EINVAL, "groth16_verify_folded: bad argument");
  touch_ro(proofs, n * (48 + mnt753_affine_words(vk->curve, MNT753_G2))); touch_ro(inputs, 12 * vk->num_inputs * n); touch_ro(coefficients, 2 * n);
  for (size_t i = 0; i < n; ++i)
    if (!(coefficients[2 * i] | coefficients[2 * i + 1])) return fail(MNT753_EINVAL, "groth16_verify_folded: a coefficient is zero");
  for (size_t i = 0; status && i < n; ++i) status[i] = 0;
  *accepted = getenv("MNT753_STUB_REJECT") == nullptr;
  return 0;
}
// every segment that holds a rejected proof is "rechecked": the verdicts are mnt753_groth16_verify_ex's (MNT753_STUB_REJECT)
size_t mnt753_fold_segment_proofs(int curve) { return curve == MNT753_CURVE_MNT4753 ? 128 : (curve == MNT753_CURVE_MNT6753 ? 84 : 0); }
int mnt753_groth16_verify_folded_locate(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int od, const uint64_t* coefficients,
                                        uint8_t* verdicts, mnt753_fold_locate_report* report, void* st) {
  if (!vk || (n && (!proofs || !coefficients || !verdicts))) return fail(MNT753_EINVAL, "groth16_verify_folded_locate: bad argument");
  touch_ro(coefficients, 2 * n);
  for (size_t i = 0; i < n; ++i)
    if (!(coefficients[2 * i] | coefficients[2 * i + 1])) return fail(MNT753_EINVAL, "groth16_verify_folded_locate: a coefficient is zero");
  const int rc = mnt753_groth16_verify_ex(vk, proofs, inputs, n, od, MNT753_VERIFY_CHECK_SUBGROUP, verdicts, st);
  if (rc < 0 || !report) return rc;
  const size_t g = mnt753_fold_segment_proofs(vk->curve);
  *report = mnt753_fold_locate_report{(n + g - 1) / g, 0, 0, 0.f, 0.f, 0.f, 0.f};
  for (size_t s = 0; s * g < n; ++s) {
    const size_t end = (s + 1) * g < n ? (s + 1) * g : n;
    bool bad = false;
    for (size_t i = s * g; i < end; ++i) bad |= verdicts[i] != 0;
    if (bad) { ++report->segments_rejected; report->proofs_rechecked += end - s * g; }
  }
  return rc;
}
int mnt753_group_generator(int curve, int group, uint64_t* out) {
  if (curve < 0 || curve > 1 || (group != MNT753_G1 && group != MNT753_G2) || !out) return fail(MNT753_EINVAL, "group_generator: bad argument");
  for (size_t i = 0; i < mnt753_affine_words(curve, group); ++i) out[i] = 1 + i;
  return 0;
}
int mnt753_groth16_sizes(const mnt753_r1cs* r, const mnt753_domain* d, mnt753_keygen_sizes* out) {
  if (!r || !d || !out || d->m < r->nc + r->num_inputs + 1) return fail(MNT753_EINVAL, "groth16_sizes: bad argument");
  out->a_query = out->b_g1_query = out->b_g2_query = r->m + 1; out->l_query = r->m - r->num_inputs; out->h_query = d->m - 1; out->abc_g1 = r->num_inputs + 1;
  return 0;
}
int mnt753_groth16_generate(mnt753_r1cs* r, mnt753_domain* d, const uint64_t* t, const uint64_t* alpha, const uint64_t* beta, const uint64_t* delta, const uint64_t* g1,
                            const mnt753_keygen_opts*, const mnt753_keygen_out* out, mnt753_keygen_report* rep, void*) {
  mnt753_keygen_sizes sz;
  if (!t || !alpha || !beta || !delta || !g1 || !out) return fail(MNT753_EINVAL, "groth16_generate: null argument");
  if (int rc = mnt753_groth16_sizes(r, d, &sz)) return rc;
  touch_ro(t, 12); touch_ro(alpha, 12); touch_ro(beta, 12); touch_ro(delta, 12); touch_ro(g1, 24);
  const size_t w1 = mnt753_affine_words(d->curve, MNT753_G1), w2 = mnt753_affine_words(d->curve, MNT753_G2);
  memset(out->dev_a_query, 0, 8 * w1 * sz.a_query); memset(out->dev_b_g1_query, 0, 8 * w1 * sz.b_g1_query); memset(out->dev_b_g2_query, 0, 8 * w2 * sz.b_g2_query);
  if (sz.l_query) memset(out->dev_l_query, 0, 8 * w1 * sz.l_query);
  memset(out->dev_h_query, 0, 8 * w1 * sz.h_query); memset(out->dev_abc_g1, 0, 8 * w1 * sz.abc_g1);
  memset(out->host_alpha_g1, 0, 8 * w1); memset(out->host_beta_g1, 0, 8 * w1); memset(out->host_beta_g2, 0, 8 * w2); memset(out->host_delta_g1, 0, 8 * w1);
  memset(out->host_delta_g2, 0, 8 * w2);
  if (rep) { rep->non_zero_at = rep->non_zero_bt = 0; rep->swapped = 0; rep->reserved = 0; }
  return 0;
}
}
