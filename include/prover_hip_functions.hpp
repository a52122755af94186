// prover_hip_functions.hpp -- the MI355X drop-in for the reference's prover wrapper.
//
// Mirrors libsnark/prover_reference_include/prover_reference_functions.hpp:5-162 of
// MinaProtocol/snark-challenge-prover-reference member for member: the same nested opaque types and the
// same static methods with the same argument meaning, so that the reference's own drivers
//     template <typename B> compute_H(...)   (cuda_prover_piecewise.cu:18-53)
//     template <typename B> run_prover(...)  (cuda_prover_piecewise.cu:55-98)
// compile unchanged with B = mnt4753_hip / mnt6753_hip.  Everything lands in libmnt753_hip.so through the
// C ABI of include/mnt753_hip.h; vectors live in HBM, points that the driver handles one at a time
// (G1 / G2 / field) live on the host in the reference's in-memory (wire) format.
//
// Differences a maintainer should know:
//   * errors: the reference has none on this path (unchecked fopen/fread).  Here a failed HIP call, a missing
//     device or a short file throws std::runtime_error with the C ABI's message.
//   * ownership is the reference's: every accessor returns a new wrapper that shares the underlying storage;
//     delete_* frees the wrapper (delete_G2 takes a G2*, fixing the reference's `delete_G2(G1*)` typo, hpp:73).
//   * vector_Fr_copy_into of the MNT4753 class ignores the source offset exactly like the reference
//     (prover_reference_functions.cpp:209-212); the MNT6753 class honours it (:515-520).
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace mnt753_hip_detail {
struct DeviceBuffer;   // RAII hipMalloc'd block
struct BaseSetHolder;  // RAII mnt753_bases*
struct DomainHolder;   // RAII mnt753_domain*
}  // namespace mnt753_hip_detail

template <int CURVE>
class mnt753_hip_impl {
public:
  class groth16_input;
  class groth16_params;
  struct evaluation_domain;
  struct field;
  struct G1;
  struct G2;
  struct vector_Fr;
  struct vector_G1;
  struct vector_G2;
  class r1cs;   // extension: a constraint system resident on the device (witness-map front end)

  static void init_public_params();

  static void print_G1(G1 *a);
  static void print_G2(G2 *a);

  static evaluation_domain *get_evaluation_domain(size_t d);

  static G1 *G1_add(G1 *a, G1 *b);
  static G1 *G1_scale(field *a, G1 *b);

  static void vector_Fr_muleq(vector_Fr *a, vector_Fr *b, size_t size);
  static void vector_Fr_subeq(vector_Fr *a, vector_Fr *b, size_t size);
  static vector_Fr *vector_Fr_offset(vector_Fr *a, size_t offset);
  static void vector_Fr_copy_into(vector_Fr *src, vector_Fr *dst, size_t length);
  static vector_Fr *vector_Fr_zeros(size_t length);

  static void domain_iFFT(evaluation_domain *domain, vector_Fr *a);
  static void domain_cosetFFT(evaluation_domain *domain, vector_Fr *a);
  static void domain_icosetFFT(evaluation_domain *domain, vector_Fr *a);
  static void domain_divide_by_Z_on_coset(evaluation_domain *domain, vector_Fr *a);
  static size_t domain_get_m(evaluation_domain *domain);

  static G1 *multiexp_G1(vector_Fr *scalar_start, vector_G1 *g_start, size_t length);
  static G2 *multiexp_G2(vector_Fr *scalar_start, vector_G2 *g_start, size_t length);

  static groth16_input *read_input(const char *path, groth16_params *params);

  static vector_Fr *input_w(groth16_input *input);
  static vector_Fr *input_ca(groth16_input *input);
  static vector_Fr *input_cb(groth16_input *input);
  static vector_Fr *input_cc(groth16_input *input);
  static field *input_r(groth16_input *input);

  static groth16_params *read_params(const char *path);

  static size_t params_d(groth16_params *params);
  static size_t params_m(groth16_params *params);
  static vector_G1 *params_A(groth16_params *params);
  static vector_G1 *params_B1(groth16_params *params);
  static vector_G1 *params_L(groth16_params *params);
  static vector_G1 *params_H(groth16_params *params);
  static vector_G2 *params_B2(groth16_params *params);

  static void delete_G1(G1 *a);
  static void delete_G2(G2 *a);
  static void delete_field(field *a);   // extension: the reference never frees the B::field of input_r (no such member there)
  static void delete_vector_Fr(vector_Fr *a);
  static void delete_vector_G1(vector_G1 *a);
  static void delete_vector_G2(vector_G2 *a);
  static void delete_groth16_input(groth16_input *a);
  static void delete_groth16_params(groth16_params *a);
  static void delete_evaluation_domain(evaluation_domain *a);

  static void groth16_output_write(G1 *A, G2 *B, G1 *C, const char *output_path);

  // ---- extensions (not in the reference wrapper) -------------------------------------------------
  // the whole of compute_H<B> in one device-resident call (overwrites ca, cb, cc like the reference)
  static vector_Fr *compute_H_fused(evaluation_domain *domain, vector_Fr *ca, vector_Fr *cb, vector_Fr *cc);
  // ---- the spot check of compute_H: H(t) Z(t) = A(t) B(t) - C(t) at one point t (mnt753_h_check) ----------
  // A(t), B(t), C(t) are the values at t of the polynomials that take ca, cb, cc on the domain: they must be taken BEFORE compute_H
  // overwrites the vectors (h_check_begin: one inner product per vector against L(t), each on the device its vector lives on), and
  // are compared with Z(t) H(t) once the coefficients exist (h_check_finish, on h's device; it frees the state).  t: 12 words in wire
  // form, or null for a random point from the operating system; a t inside the domain or >= r throws.  With probability >= 1 - 2m/r
  // over t the identity fails whenever a row has ca cb != cc or a coefficient of H is wrong.
  struct h_check_state;
  struct h_check_result {
    bool ok;
    uint64_t t[12], lhs[12], rhs[12];      // the point, A(t) B(t) - C(t) and Z(t) H(t), wire form
    std::string message() const;           // "H: H·Z = A·B − C fails at t = 0x…" (t as an integer in the Montgomery wire form's words)
  };
  struct h_check_failed : std::runtime_error { using std::runtime_error::runtime_error; };
  static h_check_state *h_check_begin(evaluation_domain *domain, vector_Fr *ca, vector_Fr *cb, vector_Fr *cc, const uint64_t *t_or_null);
  static h_check_result h_check_finish(h_check_state *state, vector_Fr *h);
  // true: compute_H_fused runs both around its transforms, at a random t, and throws h_check_failed where the identity fails
  // (off by default; main_hip --check-h calls begin and finish itself, around either form of compute_H)
  static void check_H(bool on);
  // C = Ht + Lt + r Bt1 (cuda_prover_piecewise.cu:79-90: three multiexps, B::G1_scale, two B::G1_add) as ONE multi-scalar
  // multiplication over the concatenated base set H | L | B1 with the scalars coefficients_for_H | w_L | r w.  The same group
  // element, hence the same proof bytes.  read_params builds the concatenated set (and B1 / L / H as sets of their own only when
  // params_B1 / params_L / params_H are first asked for) unless fuse_C(false) was called before it or MNT753_FUSED_C=0 is set.
  static G1 *groth16_C(groth16_params *params, vector_Fr *coefficients_for_H, vector_Fr *w_L, vector_Fr *w, field *r);
  static void fuse_C(bool on);
  // Number of GPUs of this node the parameters are sharded over (call before init_public_params; default 1, or the value of
  // the environment variable MNT753_GPUS).  Every vector_G1 / vector_G2 is cut into contiguous slices, one per device, exactly
  // as libff cuts an MSM over OpenMP threads (multiexp.tcc:417-431); multiexp_G1 / multiexp_G2 run the slices concurrently
  // and fold the partial results in rank order (multiexp.tcc:433-438).  The FFTs stay on device 0.
  static void use_devices(int n);
  // Where the partial points of a sharded multiexp meet: false (default) -- on the host, where mnt753_msm_finish leaves them anyway;
  // true -- through an RCCL all-gather over the devices (mnt753_exchange_points, xGMI) before the fold.  Also MNT753_FOLD=rccl.
  static void fold_over_rccl(bool on);
  // true: this process proves ONCE -- what the reference's `./main <curve> compute ...` is (libsnark/main.cpp:196-203 loads the
  // parameters per invocation, :274-293).  read_params then builds the base sets without their window tables and runs no warm-up MSM:
  // a table costs 0.33 s per 2^20 G1 points (1.3 s for the G2 set) and saves 20 ms per MSM, which pays from the second proof of a
  // resident prover (--repeat / --serve / several jobs), never in one.  Same proof bytes.  main_hip sets it for a single job on one
  // device; MNT753_ONE_SHOT=0 / 1 and MNT753_MSM_PRECOMP=0 / 1 override.  Call before read_params.
  static void one_shot(bool on);
  // true: get_evaluation_domain also builds the mixed-radix basic domains of MNT6753 (2^a 5^b, up to 819200 elements: libfqfft's
  // basic_radix2_domain over the small subgroup of Fr, candidates 1, 4 and 7 of get_evaluation_domain) where it otherwise throws
  // with the library's message -- mnt753_domain_create_for_ex with MNT753_DOMAIN_ALLOW_MIXED.  Off by default; nothing changes on
  // MNT4753.  main_hip --mixed-radix / MNT753_MIXED_RADIX=1.  Call before read_params and get_evaluation_domain.
  static void allow_mixed_radix(bool on);
  // The step before the hot path: instead of reading ca / cb / cc from the input file (where the
  // reference's generator put them, generate_parameters.cpp:44-57), evaluate the constraint system on the assignment on the
  // device -- the first loop of r1cs_to_qap_witness_map (reductions/r1cs_to_qap/r1cs_to_qap.tcc:223-237).
  // read_r1cs: the file written by oracle/ref_groth16.cpp (u64 num_inputs, m, nc; per matrix a, b, c: u64 row_ptr[nc + 1],
  // u32 col[nnz], Fr coeff[nnz]).  read_witness: a file holding w[m + 1] and r only; the returned groth16_input behaves like
  // one from read_input.
  static r1cs *read_r1cs(const char *path);
  static groth16_input *read_witness(const char *path, groth16_params *params, r1cs *cs);
  static void delete_r1cs(r1cs *a);
  // Input validation on the device (include/mnt753_hip.h, "input validation"; the reference's counterparts are libff's
  // G::is_well_formed() and the cs.is_satisfied() assertion of r1cs_to_qap.tcc:216 -- its prover wrapper has neither).  One entry per
  // set that was looked at: its name (A, B1, B2, L, H; w, ca, cb, cc, r; "constraints" for the rows ca[i] cb[i] = cc[i]), its size,
  // the number of bad elements, the lowest bad index inside the set (file order, also with several devices) and that index's reason
  // (MNT753_BAD_*).  Nothing throws for a malformed input; I/O and device errors throw as everywhere.
  struct check_entry { const char *set; size_t size; uint64_t n_bad, first_bad; int reason; };
  struct check_report {
    check_entry sets[8];
    int n_sets = 0;
    bool ok() const { for (int k = 0; k < n_sets; ++k) if (sets[k].n_bad) return false; return true; }
    const check_entry *first_bad() const { for (int k = 0; k < n_sets; ++k) if (sets[k].n_bad) return &sets[k]; return nullptr; }
  };
  // check_params: the five point sets of the file the parameters were read from -- the base sets keep their points in the device
  // radix, so the wire points are streamed from the file once more (every device its own slices, mnt753_load_file_to_device) into a
  // block that lives for the check only.  check_input: w, ca, cb, cc, r canonical, and ca[i] cb[i] = cc[i] for every row -- call it
  // before compute_H, which overwrites the three vectors; it waits for the input's loaders.
  static check_report check_params(groth16_params *params);
  static check_report check_input(groth16_input *input, groth16_params *params);
  // the same from files alone: no base sets, no window tables, no evaluation domain (what `main_hip <curve> check` runs);
  // input_path may be null.  check_witness_file: w and r canonical, and mnt753_r1cs_check of w against the system.
  static check_report check_params_file(const char *params_path);
  static check_report check_input_file(const char *params_path, const char *input_path);
  static check_report check_witness_file(const char *params_path, r1cs *cs, const char *witness_path);
  static const char *check_reason_text(int reason);
  // Subgroup membership (mnt753_check_subgroup), opt-in: the overloads with subgroup = true send the B2 set
  // through it instead of mnt753_check_points (the same tests first, then MNT753_BAD_NOT_IN_SUBGROUP; the G1 sets have cofactor 1).
  // check_subgroup: n G2 points in host memory (wire words), e.g. beta_g2 | delta_g2 of a key, as one entry named "G2".
  static check_report check_params(groth16_params *params, bool subgroup);
  static check_report check_params_file(const char *params_path, bool subgroup);
  static check_entry check_subgroup(const uint64_t *g2_affine, size_t n);
  // seconds the background loader of read_input needed until the whole input file was on the device (waits for it)
  static double input_load_seconds(groth16_input *input);
  // The pairing and Groth16 verification on the device (mnt753_pairing, mnt753_vk_create + mnt753_groth16_verify): extensions, the
  // reference's B has neither.  Wire words in host memory.  pairing: n reduced pairings, mnt753_gt_words words each.  verify:
  // vk_elements = alpha_g1 | beta_g2 | delta_g2 | ABC_g1 (num_inputs + 1 points, the contents of `generate`'s vk_elements.bin),
  // proofs = n x (A | B | C), inputs = n x num_inputs Fr; one verdict per proof: 0 accepted, 1 malformed, 2 the pairing check failed.
  static std::vector<uint64_t> pairing(const uint64_t *g1_affine, const uint64_t *g2_affine, size_t n);
  static std::vector<uint8_t> verify(const uint64_t *vk_elements, size_t num_inputs, const uint64_t *proofs, const uint64_t *inputs, size_t n);
  // with check_subgroup also verdict 3: B is not in the order-r subgroup of the twist (mnt753_groth16_verify_ex); the key's own G2
  // elements are not tested by this call (check_subgroup above does that)
  static std::vector<uint8_t> verify(const uint64_t *vk_elements, size_t num_inputs, const uint64_t *proofs, const uint64_t *inputs, size_t n,
                                     bool check_subgroup);
  // the batch folded into ONE final exponentiation (mnt753_groth16_verify_folded): coefficients = n x 2 words,
  // 0 < rho_i < 2^128, drawn by the caller AFTER the proofs are fixed; status per proof 0, 1 (malformed) or 3 (B not in the subgroup);
  // accepted: every status is 0 and the folded equation holds.  A rejected batch does not name the wrong proof: verify(.., true) does.
  struct folded_verdict {
    bool accepted;
    std::vector<uint8_t> status;
  };
  static folded_verdict verify_folded(const uint64_t *vk_elements, size_t num_inputs, const uint64_t *proofs, const uint64_t *inputs, size_t n,
                                      const uint64_t *coefficients);
  // the fold with one tail per segment (mnt753_groth16_verify_folded_locate): the verdicts of verify(.., true),
  // with the per-proof pass run on the rejected segments only (segments of mnt753_fold_segment_proofs(curve) proofs); coefficients as
  // for verify_folded
  struct fold_locate_report { uint64_t segments, segments_rejected, proofs_rechecked; float ms_scale, ms_miller, ms_tails, ms_recheck; };
  struct located_verdicts {
    std::vector<uint8_t> verdicts;
    fold_locate_report report;
  };
  static located_verdicts verify_folded_locate(const uint64_t *vk_elements, size_t num_inputs, const uint64_t *proofs, const uint64_t *inputs, size_t n,
                                               const uint64_t *coefficients);
  // Compressed points (mnt753_compress_points / mnt753_decompress_points / mnt753_groth16_verify_compressed):
  // x and one flag byte per point -- bit 0 the parity of y as an integer, bit 1 the identity.  group: MNT753_G1 / MNT753_G2; wire words
  // in host memory.  compress_points validates nothing; decompress_points reports like a check (entry "points"), a bad point's words
  // are zero.  verify_compressed: x = n x (x_A | x_B | x_C), flags = n x 3; the verdicts of verify(), 1 also for a point that does not
  // decompress and for an identity flag.
  struct compressed_points {
    std::vector<uint64_t> x;
    std::vector<uint8_t> flags;
  };
  struct decompressed_points {
    std::vector<uint64_t> affine;
    check_entry report;
  };
  static compressed_points compress_points(int group, const uint64_t *affine, size_t n);
  static decompressed_points decompress_points(int group, const uint64_t *x, const uint8_t *flags, size_t n);
  static std::vector<uint8_t> verify_compressed(const uint64_t *vk_elements, size_t num_inputs, const uint64_t *x, const uint8_t *flags, const uint64_t *inputs,
                                                size_t n, bool check_subgroup);
  // Input tables (mnt753_vk_prepare_inputs), opt-in: with tables.enabled the key these calls make is prepared
  // before it verifies -- one window table per ABC point, W = ceil(754 / w) additions per public input instead of a double-and-add over
  // 753 bits; the same verdicts.  window_bits 0: the widest width whose tables fit max_table_bytes (0: 256 MiB); a width or a cap that
  // cannot be met throws.  plan, where given, receives what was built.
  struct input_table_plan { int window_bits, windows; uint64_t table_bytes; };
  struct input_tables {
    bool enabled = false;
    int window_bits = 0;
    size_t max_table_bytes = 0;
    input_table_plan *plan = nullptr;
  };
  static std::vector<uint8_t> verify(const uint64_t *vk_elements, size_t num_inputs, const uint64_t *proofs, const uint64_t *inputs, size_t n,
                                     bool check_subgroup, const input_tables &tables);
  static folded_verdict verify_folded(const uint64_t *vk_elements, size_t num_inputs, const uint64_t *proofs, const uint64_t *inputs, size_t n,
                                      const uint64_t *coefficients, const input_tables &tables);
  static located_verdicts verify_folded_locate(const uint64_t *vk_elements, size_t num_inputs, const uint64_t *proofs, const uint64_t *inputs, size_t n,
                                               const uint64_t *coefficients, const input_tables &tables);
  static std::vector<uint8_t> verify_compressed(const uint64_t *vk_elements, size_t num_inputs, const uint64_t *x, const uint8_t *flags, const uint64_t *inputs,
                                                size_t n, bool check_subgroup, const input_tables &tables);
  // raw access for tests / tools
  static const uint64_t *G1_words(const G1 *a);
  static const uint64_t *G2_words(const G2 *a);
};

using mnt4753_hip = mnt753_hip_impl<0>;
using mnt6753_hip = mnt753_hip_impl<1>;

extern template class mnt753_hip_impl<0>;
extern template class mnt753_hip_impl<1>;
