// ./main_hip <curve> <command> ...     <curve>: MNT4753 | MNT6753
// The commands are the rows of `commands` near the end of this file, in that order: compute, compute-r1cs, complete, check, check-r1cs,
// qap-at, generate, vk, verify, compress-proof, decompress-proof, self-test.  Each row carries its usage text, which names the command's words and options and is what
// the program prints for a command line it cannot read; the comment above each command's function says what the command does.
// Options come from, in rising precedence: defaults, the environment (read_environment), the command line.
// Exit codes: 0 success, 1 device / I/O / self-test failure, 2 usage, 3 an input failed validation (or its H failed --check-h).
//
// The prover driver, same command line as the reference binaries (libsnark/main.cpp:274-293,
// cuda_prover_piecewise.cu:100-120).  compute_H<B> and run_prover<B> keep the reference's shape -- they are
// written against the wrapper type B only -- and are instantiated with the MI355X classes.
// Timing prints follow libsnark/main.cpp:201-270: the window "Total time from input to output" opens after
// the parameters are loaded and contains input load, compute and output write.
#include <sys/random.h>
#include <sys/stat.h>

#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mnt753_hip.h"
#include "../../include/prover_hip_functions.hpp"
#include "main_io.hpp"   // the file helpers, R1csFile, owners for the C ABI's handles
#include "../csrc/mnt753_constants.h"   // FPC[].one64: the wire form of 1

// Defaults = the fastest schedule on one MI355X: the G2 MSM is enqueued as soon as w is on the device, compute_H (one fused
// call) follows as soon as ca / cb / cc are, then the G1 MSMs.  The point kernels occupy every SIMD with long-lived
// workgroups, so the ~60 short NTT kernels of compute_H must not be enqueued behind the G1 MSMs (measured: 0.24 s with this
// order, 0.44-1.1 s with the reference's source order), and C = Ht + Lt + r Bt1 is one MSM over the concatenated base set
// (B::groth16_C).  --ref-order keeps the call sequence of cuda_prover_piecewise.cu:64-90 (five multiexps, compute_H after the
// first three, G1_scale, two G1_add -- the wrapper still runs the last three multiexps and that tail as one MSM, see LazyPoint in
// prover_hip_functions.cpp), --unfused-c loads the parameters as five base sets and runs the five multiexps, --unfused-h the
// reference's sequence of B:: calls inside compute_H (cuda_prover_piecewise.cu:24-47); every combination writes the same bytes.
struct Options {
  bool fused_h = true;
  bool quiet = false;
  bool h_first = true;
  bool c_first = true;    // fused C: its MSM (3x the points of A's) is enqueued ahead of A's; --c-last the other way round
  bool explicit_c = true;   // call B::groth16_C; off (--ref-order): the reference's calls, which the wrapper fuses by itself when the parameters are fused
  bool touch_all = false;   // --touch-all (with --ref-order): read Bt1, Lt, Ht before they are combined -- with fused parameters that forces the three separate MSMs
  bool fused_c = true;   // C = Ht + Lt + r Bt1 as one MSM over H | L | B1 (B::groth16_C); --unfused-c / --ref-order: the reference's five multiexps
  int gpus = 0;   // --gpus N: parameter vectors sharded over N devices of this node (0: MNT753_GPUS or 1)
  int env_gpus = 0;   // MNT753_GPUS as the wrapper will read it (0: not set); here only the one-shot decision looks at it
  bool serve = false;    // --serve: after the listed jobs, read further "<input> <output>" lines from stdin until EOF
  int one_shot = -1;     // -1: decided from the job list (one job, no --serve, one device: a one-proof process); --one-shot / --tables force it
  bool peer_bench = false;   // --peer-bench (with --gpus N): time the peer copies the sharded prover makes, 100 MB each, before proving
  int fold_rccl = -1;    // --fold rccl | host: where the partial points of a sharded multiexp meet (default: MNT753_FOLD, else host)

  // --validate (or MNT753_VALIDATE=1): the parameters are checked once after they are loaded (points canonical and on their curves),
  // every job's input before its proof starts (scalars canonical, ca[i] cb[i] = cc[i] on every row -- for compute-r1cs that is the
  // witness against the system).  A failing job writes no output file; the process exits 3 if anything failed validation.
  bool validate = false;
  // --mixed-radix (or MNT753_MIXED_RADIX=1): B::get_evaluation_domain also builds libfqfft's mixed-radix basic domains of MNT6753
  // (B::allow_mixed_radix); without it such a d + 1 ends with the library's message, as before
  bool mixed_radix = false;
  // --check-h (or MNT753_CHECK_H=1): every job's quotient polynomial is checked against its ca, cb, cc at one point t before anything is
  // written, H(t) Z(t) = A(t) B(t) - C(t) (B::h_check_begin / B::h_check_finish around compute_H, fused or not, sharded or not).  A
  // random t per job, or the 96-byte wire element of --check-h-t <file> for a reproducible run.  A failing job writes no output file
  // and the process exits 3, as with --validate; unlike --validate the check also covers compute_H itself.
  bool check_h = false;
  bool check_h_t_given = false;
  uint64_t check_h_t[12] = {};

  // compute / compute-r1cs: (input, output) pairs, all proved against the same resident parameters; --repeat N lists them N times
  std::vector<std::pair<std::string, std::string>> jobs;
  int repeat = 1;
};
struct validation_failed : std::runtime_error { using std::runtime_error::runtime_error; };

// What the environment sets, under the command line and over the defaults.  The only getenv of this file: the wrapper reads its own
// variables (MNT753_GPUS among them, init_public_params).
static void read_environment(Options& o) {
  if (const char* e = getenv("MNT753_VALIDATE")) o.validate = atoi(e) != 0;
  if (const char* e = getenv("MNT753_MIXED_RADIX")) o.mixed_radix = atoi(e) != 0;
  if (const char* e = getenv("MNT753_CHECK_H")) o.check_h = atoi(e) != 0;
  if (const char* e = getenv("MNT753_GPUS")) o.env_gpus = atoi(e);
}

// one line per set: "A: 1048577 points ok" / "H: 3 bad, first at 524288: off curve" / "constraint 17 of 30 is not satisfied"
template <typename B>
static std::string check_line(const typename B::check_entry& e) {
  const bool rows = !strcmp(e.set, "constraints");
  const bool points = e.set[0] >= 'A' && e.set[0] <= 'Z';
  if (!e.n_bad) return std::string(e.set) + ": " + std::to_string(e.size) + (rows ? " rows satisfied" : (points ? " points ok" : " scalars ok"));
  if (rows && e.reason == MNT753_BAD_UNSATISFIED)
    return "constraint " + std::to_string(e.first_bad) + " of " + std::to_string(e.size) + " is not satisfied (" + std::to_string(e.n_bad) + " in all)";
  return std::string(e.set) + ": " + std::to_string(e.n_bad) + " bad, first at " + std::to_string(e.first_bad) + ": " + B::check_reason_text(e.reason);
}
template <typename B>
static bool print_report(const typename B::check_report& rep) {
  for (int k = 0; k < rep.n_sets; ++k) printf("%s\n", check_line<B>(rep.sets[k]).c_str());
  return rep.ok();
}

typedef std::chrono::steady_clock clk;
static double secs(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }
static void ck(int rc, const char* what) { if (rc) throw std::runtime_error(std::string(what) + ": " + mnt753_last_error()); }

// cuda_prover_piecewise.cu:18-53.  Overwrites ca (and cb, cc), like the reference.
// h_failure: under --check-h, the message of an H that failed its check; left alone while the H stands
template <typename B>
typename B::vector_Fr* compute_H(const Options& o, size_t d, typename B::vector_Fr* ca, typename B::vector_Fr* cb, typename B::vector_Fr* cc, std::string& h_failure) {
  auto domain = B::get_evaluation_domain(d + 1);
  // A(t), B(t), C(t) before the transforms overwrite the vectors; the verdict once the coefficients exist.  A failed identity is
  // recorded, not thrown: the job runs to its end like any other (every buffer is released on the one path) and writes nothing.
  typename B::h_check_state* checking = o.check_h ? B::h_check_begin(domain, ca, cb, cc, o.check_h_t_given ? o.check_h_t : nullptr) : nullptr;
  auto verdict = [&](typename B::vector_Fr* h) {
    if (!checking) return;
    const auto tv = clk::now();
    const auto res = B::h_check_finish(checking, h);
    if (!res.ok) h_failure = res.message();
    if (!o.quiet) printf("check H: %s (%.4fs behind compute_H)\n", res.ok ? "H Z = A B - C holds" : "FAILED", secs(tv, clk::now()));
  };
  if (o.fused_h) {
    auto H_res = B::compute_H_fused(domain, ca, cb, cc);
    verdict(H_res);
    B::delete_evaluation_domain(domain);
    return H_res;
  }
  B::domain_iFFT(domain, ca);
  B::domain_iFFT(domain, cb);
  B::domain_cosetFFT(domain, ca);
  B::domain_cosetFFT(domain, cb);
  auto H_tmp = ca;  // ca stores H
  size_t m = B::domain_get_m(domain);
  B::vector_Fr_muleq(H_tmp, cb, m);
  B::domain_iFFT(domain, cc);
  B::domain_cosetFFT(domain, cc);
  B::vector_Fr_subeq(H_tmp, cc, m);
  B::domain_divide_by_Z_on_coset(domain, H_tmp);
  B::domain_icosetFFT(domain, H_tmp);
  typename B::vector_Fr* H_res = B::vector_Fr_zeros(m + 1);
  B::vector_Fr_copy_into(H_tmp, H_res, m);
  verdict(H_res);
  B::delete_evaluation_domain(domain);
  return H_res;
}

// cuda_prover_piecewise.cu:55-98, split at the line where the reference opens its timing window (libsnark/main.cpp:201-203):
// the parameters are loaded once and stay resident (window tables, workspaces, evaluation domain); every (input, output)
// pair after that is one proof.  With a single pair this is exactly the reference's run_prover.
template <typename B>
void prove_one(const Options& o, typename B::groth16_params* params, const char* input_path, const char* output_path, clk::time_point t0, bool first,
               typename B::r1cs* cs = nullptr) {
  const size_t primary_input_size = 1;
  auto t_main = clk::now();
  // compute-r1cs: the input file holds w and r only; ca / cb / cc come from the constraint system, evaluated on the device
  auto input = cs ? B::read_witness(input_path, params, cs) : B::read_input(input_path, params);
  std::string h_failure;    // the message of this job, empty while its H stands
  if (o.validate) {
    // before anything is enqueued on these vectors (compute_H overwrites ca, cb, cc); waits for the input's loaders
    const auto tv = clk::now();
    const auto rep = B::check_input(input, params);
    if (!o.quiet) printf("validate input: %.4fs\n", secs(tv, clk::now()));
    if (!rep.ok()) {
      const std::string line = check_line<B>(*rep.first_bad());
      B::delete_groth16_input(input);
      throw validation_failed(line);
    }
  }
  auto t_in = clk::now();
  if (!o.quiet) printf("load inputs (started in the background): %.3fs\n", secs(t_main, t_in));

  auto w = B::input_w(input);
  auto ca = B::input_ca(input), cb = B::input_cb(input), cc = B::input_cc(input);
  auto pA = B::params_A(params); auto pB2 = B::params_B2(params);
  // Same operations as cuda_prover_piecewise.cu:64-81, in an order that follows the data: B::read_input streams the
  // file in the background (w first), B::multiexp_* only enqueue work, so the G2 MSM -- the longest, and it needs nothing
  // but w -- starts as soon as w is on the device, while ca / cb / cc are still loading.
  typename B::G2* evaluation_Bt2 = B::multiexp_G2(w, pB2, B::params_m(params) + 1);
  typename B::G1 *evaluation_At, *C;
  auto w_off = B::vector_Fr_offset(w, primary_input_size + 1);
  typename B::vector_Fr* coefficients_for_H;
  auto r = B::input_r(input);
  auto t_h = clk::now();
  clk::time_point t_msm, t_c;
  if (o.fused_c && o.explicit_c) {
    // Ht + Lt + r Bt1 is one group element: one MSM over the concatenated base set H | L | B1 with the scalars h | w_off | r w
    // (B::groth16_C) instead of three MSMs, a scalar multiplication and two additions -- what an MSM pays per call and per bucket
    // is paid once.  It needs coefficients_for_H, so compute_H goes first, right behind the G2 MSM.
    coefficients_for_H = compute_H<B>(o, B::params_d(params), ca, cb, cc, h_failure);
    t_h = clk::now();
    if (o.c_first) C = B::groth16_C(params, coefficients_for_H, w_off, w, r);
    evaluation_At = B::multiexp_G1(w, pA, B::params_m(params) + 1);
    if (!o.c_first) C = B::groth16_C(params, coefficients_for_H, w_off, w, r);
    // touching a result waits for its MSM and runs the host tail of its bucket reduction (c - 1 doublings and additions: 0.33 ms for
    // an Fq3 point).  In the order the device finishes them -- the G2 MSM was enqueued first, A's point kernels are ordered behind
    // C's on the small sets -- so that every tail but the last runs under the kernels still in flight (profiles/r05/mnt6753_prove_timeline.txt)
    (void)B::G2_words(evaluation_Bt2); (void)B::G1_words(C); (void)B::G1_words(evaluation_At);
    t_msm = t_c = clk::now();
  } else {
    auto pB1 = B::params_B1(params); auto pH = B::params_H(params); auto pL = B::params_L(params);
    typename B::G1 *evaluation_Bt1, *evaluation_Lt, *evaluation_Ht;
    if (o.h_first) {
      // compute_H right behind the G2 MSM: its short kernels are not starved by four G1 accumulation phases, and the H MSM
      // overlaps the others instead of running alone at the end
      coefficients_for_H = compute_H<B>(o, B::params_d(params), ca, cb, cc, h_failure);
      t_h = clk::now();
      evaluation_Ht = B::multiexp_G1(coefficients_for_H, pH, B::params_d(params));
      evaluation_At = B::multiexp_G1(w, pA, B::params_m(params) + 1);
      evaluation_Bt1 = B::multiexp_G1(w, pB1, B::params_m(params) + 1);
      evaluation_Lt = B::multiexp_G1(w_off, pL, B::params_m(params) - 1);
    } else {
      evaluation_At = B::multiexp_G1(w, pA, B::params_m(params) + 1);
      evaluation_Bt1 = B::multiexp_G1(w, pB1, B::params_m(params) + 1);
      evaluation_Lt = B::multiexp_G1(w_off, pL, B::params_m(params) - 1);
      coefficients_for_H = compute_H<B>(o, B::params_d(params), ca, cb, cc, h_failure);
      t_h = clk::now();
      evaluation_Ht = B::multiexp_G1(coefficients_for_H, pH, B::params_d(params));
    }
    // the five MSMs run concurrently on their base sets' streams; touching the results waits for them.  (With fused parameters
    // Bt1, Lt and Ht are not computed at all: the wrapper recognises Ht + (Lt + r Bt1) below and runs it as one MSM -- touching
    // them here would force the three separate ones.)
    (void)B::G1_words(evaluation_At); (void)B::G2_words(evaluation_Bt2);
    if (!o.fused_c || o.touch_all) { (void)B::G1_words(evaluation_Bt1); (void)B::G1_words(evaluation_Ht); (void)B::G1_words(evaluation_Lt); }
    t_msm = clk::now();
    auto scaled_Bt1 = B::G1_scale(r, evaluation_Bt1);
    auto Lt1_plus_scaled_Bt1 = B::G1_add(evaluation_Lt, scaled_Bt1);
    C = B::G1_add(evaluation_Ht, Lt1_plus_scaled_Bt1);
    (void)B::G1_words(C);
    t_c = clk::now();
    B::delete_G1(evaluation_Bt1); B::delete_G1(evaluation_Ht); B::delete_G1(evaluation_Lt);
    B::delete_G1(scaled_Bt1); B::delete_G1(Lt1_plus_scaled_Bt1);
    B::delete_vector_G1(pB1); B::delete_vector_G1(pH); B::delete_vector_G1(pL);
  }
  if (h_failure.empty()) B::groth16_output_write(evaluation_At, evaluation_Bt2, C, output_path);
  auto t_out = clk::now();
  if (!o.quiet && h_failure.empty()) {
    printf("G2 MSM enqueued + compute_H (input streaming in): %.3fs\nremaining MSM time: %.3fs\nC = Ht + Lt + r*Bt1: %.3fs%s\ngpu: %.4fs\nstore: %.3fs\n", secs(t_in, t_h), secs(t_h, t_msm),
           secs(t_msm, t_c), o.fused_c ? " (one MSM over H | L | B1)" : "", secs(t_in, t_c), secs(t_c, t_out));
    printf("input file on the device after: %.3fs (background loader)\n", B::input_load_seconds(input));
    printf("Total time from input to output: %.4fs\n", secs(t_main, t_out));
    if (first) printf("Total wall (incl. load params): %.3fs\n", secs(t0, t_out));
  }

  B::delete_G1(evaluation_At); B::delete_G2(evaluation_Bt2); B::delete_G1(C);
  B::delete_vector_Fr(coefficients_for_H); B::delete_vector_Fr(w); B::delete_vector_Fr(w_off);
  B::delete_vector_Fr(ca); B::delete_vector_Fr(cb); B::delete_vector_Fr(cc);
  B::delete_vector_G1(pA); B::delete_vector_G2(pB2);
  B::delete_field(r);   // (the reference's wrapper has no delete_field and its driver leaks the element)
  B::delete_groth16_input(input);
  if (!h_failure.empty()) throw validation_failed(h_failure);
}

// --peer-bench: what DESIGN.md section 5 ASSUMES (2.0 ms for 100 MB over one xGMI link), measured on the box the prover runs on: the
// copies of the sharded prove -- the transformed cb / cc 1 -> 0 and 2 -> 0 (cuda_prover_piecewise.cu:24-34 keeps them on one device;
// here they cross), a slice of coefficients_for_H 0 -> g -- as one 100 MB mnt753_copy_peer_async each, best of three, with what the
// platform granted for the pair.  One line per copy on stdout; bench.py --gpus N carries them.
static void peer_bench() {
  const int n = mnt753_device_count();
  if (n < 2) { printf("peer copy: one device, nothing to measure\n"); return; }
  const size_t bytes = (size_t)100 << 20;
  std::vector<void*> buf(n, nullptr);
  for (int g = 0; g < n; ++g) { ck(mnt753_set_device(g), "mnt753_set_device"); ck(mnt753_dev_alloc(&buf[g], bytes), "mnt753_dev_alloc"); ck(mnt753_dev_memset(buf[g], g, bytes), "mnt753_dev_memset"); }
  std::vector<std::pair<int, int>> pairs;   // (source, destination)
  pairs.emplace_back(1, 0);
  if (n > 2) pairs.emplace_back(2, 0);
  for (int g = 1; g < n; ++g) pairs.emplace_back(0, g);
  static const char* const names[] = {"same GPU (logical devices share it)", "direct (peer access)", "staged through host memory"};
  for (auto pr : pairs) {
    int how = MNT753_PEER_STAGED;
    ck(mnt753_enable_peer_access(pr.second, pr.first, &how), "mnt753_enable_peer_access");
    double best = 1e30;
    for (int k = 0; k < 4; ++k) {     // the first pass warms the path
      ck(mnt753_set_device(pr.first), "mnt753_set_device"); ck(mnt753_sync(nullptr), "mnt753_sync");
      ck(mnt753_set_device(pr.second), "mnt753_set_device"); ck(mnt753_sync(nullptr), "mnt753_sync");
      const auto t0 = clk::now();
      ck(mnt753_copy_peer_async(pr.second, buf[pr.second], pr.first, buf[pr.first], bytes), "mnt753_copy_peer_async");
      ck(mnt753_set_device(pr.second), "mnt753_set_device"); ck(mnt753_sync(nullptr), "mnt753_sync");
      const double ms = 1e3 * secs(t0, clk::now());
      if (k > 0 && ms < best) best = ms;
    }
    printf("peer copy 100 MB device %d -> %d: %.3f ms (%.1f GB/s), %s\n", pr.first, pr.second, best, bytes / best / 1e6, names[how >= 0 && how <= 2 ? how : 2]);
  }
  for (int g = 0; g < n; ++g) { ck(mnt753_set_device(g), "mnt753_set_device"); ck(mnt753_dev_free(buf[g]), "mnt753_dev_free"); }
  ck(mnt753_set_device(0), "mnt753_set_device");
}

// o.jobs: (input, output) pairs; all proved against the same resident parameters
// returns the exit code: 0, or 3 if a job (or the parameters) failed validation
template <typename B>
int run_prover(const Options& o, const char* params_path, const char* r1cs_path) {
  const auto& jobs = o.jobs;
  if (o.gpus > 0) B::use_devices(o.gpus);
  B::fuse_C(o.fused_c);
  B::allow_mixed_radix(o.mixed_radix);
  if (o.fold_rccl >= 0) B::fold_over_rccl(o.fold_rccl != 0);
  // The reference's CLI is a one-shot process: parameters loaded per invocation, one proof, exit (libsnark/main.cpp:196-203, :274-293).
  // Invoked the same way -- one job, no --repeat / --serve, one device -- this prover builds no window tables and runs no warm-up MSM:
  // 2.7 s of table kernels and 0.7 s of warm-up would buy 0.1 s on the one proof.  A resident prover (several jobs, --repeat, --serve)
  // and a sharded one (--gpus) keep them.  --tables / --one-shot force either; MNT753_MSM_PRECOMP stays the override underneath.
  {
    const bool several_devices = o.gpus > 1 || (o.gpus == 0 && o.env_gpus > 1);
    const bool one = o.one_shot >= 0 ? o.one_shot != 0 : (jobs.size() == 1 && !o.serve && !several_devices);
    B::one_shot(one);
    if (!o.quiet && one) printf("one-shot prover: no window tables (one job, no --repeat / --serve; --tables builds them)\n");
  }
  B::init_public_params();
  if (o.peer_bench) peer_bench();
  auto t0 = clk::now();
  auto params = B::read_params(params_path);
  typename B::r1cs* cs = r1cs_path ? B::read_r1cs(r1cs_path) : nullptr;
  auto t_params = clk::now();
  if (!o.quiet) printf("load params: %.3fs\n", secs(t0, t_params));
  int exit_code = 0;
  if (o.validate) {
    const auto tv = clk::now();
    const auto rep = B::check_params(params);
    if (!o.quiet) printf("validate params: %.3fs\n", secs(tv, clk::now()));
    if (!rep.ok()) {
      // nothing can be proved against these parameters: every job fails, nothing is written
      fprintf(stderr, "main_hip: %s: %s\n", params_path, check_line<B>(*rep.first_bad()).c_str());
      if (cs) B::delete_r1cs(cs);
      B::delete_groth16_params(params);
      return 3;
    }
  }
  bool first = true;
  for (const auto& job : jobs) {
    if (!o.quiet && jobs.size() > 1) printf("-- proof %s -> %s\n", job.first.c_str(), job.second.c_str());
    try {
      prove_one<B>(o, params, job.first.c_str(), job.second.c_str(), t0, first, cs);
    } catch (const validation_failed& e) {
      fprintf(stderr, "main_hip: %s: %s\n", job.first.c_str(), e.what());
      if (jobs.size() > 1 || o.serve) printf("failed %s: %s\n", job.second.c_str(), e.what());
      exit_code = 3;
    }
    first = false;
  }
  if (o.serve) {
    // Resident job feed: the parameters (window tables, workspaces, evaluation domain: ~6 s and ~54 GB of HBM to build for the 2^20
    // set) are paid once per HOST process, every job after that costs its prove time.  One job per line on stdin,
    // "<input path> <output path>"; after each, one line "proved <output path> <seconds>" (or "failed <output path>: <reason>") on
    // stdout, flushed, so a driver can pipeline requests.  EOF ends the service.
    char line[8192];
    while (fgets(line, sizeof(line), stdin)) {
      char in_path[4096], out_path[4096];
      if (sscanf(line, "%4095s %4095s", in_path, out_path) != 2) continue;
      const auto tj = clk::now();
      try {
        prove_one<B>(o, params, in_path, out_path, t0, false, cs);
        printf("proved %s %.3f\n", out_path, secs(tj, clk::now()));
      } catch (const validation_failed& e) {
        fprintf(stderr, "main_hip: %s: %s\n", in_path, e.what());
        printf("failed %s: %s\n", out_path, e.what());
        exit_code = 3;
      } catch (const std::exception& e) {
        printf("failed %s: %s\n", out_path, e.what());
      }
      fflush(stdout);
    }
  }
  if (cs) B::delete_r1cs(cs);
  B::delete_groth16_params(params);
  return exit_code;
}

// ./main_hip <curve> check <params> [<input>]             points of A, B1, B2, L, H; scalars of the input and its rows ca cb = cc
// ./main_hip <curve> check-r1cs <params> <r1cs> <witness>  the same for the parameters, and the witness against the constraint system
// One line per set on stdout; exit code 0 if everything is well formed, 3 if not.  A one-shot by nature: the files are streamed to the
// device and checked there -- no base sets, no window tables, no level buffers, no evaluation domain, no warm-up.
// --subgroup: B2 also goes through the subgroup test of G2 (mnt753_check_subgroup): "B2: 1 bad, first at 3: not in the subgroup"
template <typename B>
int run_check(const Options& o, const char* params_path, const char* input_path, const char* r1cs_path, bool subgroup) {
  if (o.gpus > 0) B::use_devices(o.gpus);
  B::init_public_params();
  bool ok = print_report<B>(subgroup ? B::check_params_file(params_path, true) : B::check_params_file(params_path));
  if (r1cs_path) {
    auto cs = B::read_r1cs(r1cs_path);
    try { ok = print_report<B>(B::check_witness_file(params_path, cs, input_path)) && ok; } catch (...) { B::delete_r1cs(cs); throw; }
    B::delete_r1cs(cs);
  } else if (input_path) {
    ok = print_report<B>(B::check_input_file(params_path, input_path)) && ok;
  }
  return ok ? 0 : 3;
}

// The one place where a curve number becomes a wrapper class: f is called with a value of mnt4753_hip or of mnt6753_hip, and
// reads the class off it (typedef decltype(b) B).
template <typename F>
static auto with_curve(int curve, F f) -> decltype(f(mnt4753_hip{})) { return curve == 0 ? f(mnt4753_hip{}) : f(mnt6753_hip{}); }
static const char* reason_text(int curve, int reason) {
  return with_curve(curve, [&](auto b) { return decltype(b)::check_reason_text(reason); });
}

// ./main_hip <curve> complete <keys> <input|witness> <challenge_proof> <full_proof> [--s-file <Fr> | --s-seed N]
//
// The step AFTER the hot path: the challenge prover stops at (A, B, C) = (sum w_i A_i, sum w_i B_i,
// Ht + Lt + r Bt1); libsnark/main.cpp:312-319 shows how the reference completes that to a Groth16 proof a verifier accepts:
//     A' = alpha + A + r delta,    B' = beta + B + s delta,    C' = C + s A' + r beta          (r from the input file, s fresh)
// keys = alpha_g1 | beta_g1 | beta_g2 | delta_g1 | delta_g2 in the wire format (oracle/ref_groth16.cpp mints them from the
// reference's generator).  O(1) group operations on the host through the C ABI; no GPU needed.
static bool read_start(const char* path, void* dst, size_t bytes) {
  return read_exact(path, dst, bytes, false, std::string("cannot open ") + path, std::string("short read: ") + path);
}
// what complete and its --validate read: the keys, the challenge proof, and r, the last element of the input file
struct CompletionInputs {
  size_t g1 = 24, g2 = 0;
  std::vector<uint64_t> keys, proof;
  uint64_t r[12];
  bool load(int curve, const char* keys_path, const char* input_path, const char* challenge_path) {
    g2 = mnt753_affine_words(curve, MNT753_G2);
    keys.resize(3 * g1 + 2 * g2); proof.resize(2 * g1 + g2);
    return read_start(keys_path, keys.data(), keys.size() * 8) && read_start(challenge_path, proof.data(), proof.size() * 8) &&
           read_tail(input_path, r, 96, std::string("cannot open ") + input_path, std::string("seek failed: ") + input_path, std::string("short read: ") + input_path);
  }
};
static int complete_proof(int curve, const char* keys_path, const char* input_path, const char* challenge_path, const char* out_path,
                          const char* s_file, uint64_t s_seed) {
  CompletionInputs in;
  if (!in.load(curve, keys_path, input_path, challenge_path)) return 1;
  const size_t g1 = in.g1, g2 = in.g2;
  const std::vector<uint64_t>& keys = in.keys, &proof = in.proof;
  const uint64_t* r = in.r;
  uint64_t s[12];
  if (s_file) { if (!read_start(s_file, s, 96)) return 1; } else ck(mnt753_synth_scalars(curve, s_seed, 1, s), "mnt753_synth_scalars");
  const uint64_t *alpha1 = keys.data(), *beta1 = alpha1 + g1, *beta2 = beta1 + g1, *delta1 = beta2 + g2, *delta2 = delta1 + g1;
  auto lift = [&](int group, const uint64_t* aff, uint64_t* proj) { ck(mnt753_point_from_affine(curve, group, aff, proj), "mnt753_point_from_affine"); };
  uint64_t pa[36], pb[108], pc[36], t1[36], t2[108], u1[36], u2[108];
  // A' = alpha + A + r delta
  lift(MNT753_G1, proof.data(), pa); lift(MNT753_G1, alpha1, t1);
  ck(mnt753_point_add(curve, MNT753_G1, t1, pa, pa), "mnt753_point_add");
  lift(MNT753_G1, delta1, t1); ck(mnt753_point_scale(curve, MNT753_G1, r, t1, u1), "mnt753_point_scale");
  ck(mnt753_point_add(curve, MNT753_G1, pa, u1, pa), "mnt753_point_add");
  // B' = beta + B + s delta
  lift(MNT753_G2, proof.data() + g1, pb); lift(MNT753_G2, beta2, t2);
  ck(mnt753_point_add(curve, MNT753_G2, t2, pb, pb), "mnt753_point_add");
  lift(MNT753_G2, delta2, t2); ck(mnt753_point_scale(curve, MNT753_G2, s, t2, u2), "mnt753_point_scale");
  ck(mnt753_point_add(curve, MNT753_G2, pb, u2, pb), "mnt753_point_add");
  // C' = C + s A' + r beta
  lift(MNT753_G1, proof.data() + g1 + g2, pc);
  ck(mnt753_point_scale(curve, MNT753_G1, s, pa, u1), "mnt753_point_scale");
  ck(mnt753_point_add(curve, MNT753_G1, pc, u1, pc), "mnt753_point_add");
  lift(MNT753_G1, beta1, t1); ck(mnt753_point_scale(curve, MNT753_G1, r, t1, u1), "mnt753_point_scale");
  ck(mnt753_point_add(curve, MNT753_G1, pc, u1, pc), "mnt753_point_add");
  std::vector<uint64_t> out(2 * g1 + g2);
  ck(mnt753_point_to_affine(curve, MNT753_G1, pa, out.data()), "mnt753_point_to_affine");
  ck(mnt753_point_to_affine(curve, MNT753_G2, pb, out.data() + g1), "mnt753_point_to_affine");
  ck(mnt753_point_to_affine(curve, MNT753_G1, pc, out.data() + g1 + g2), "mnt753_point_to_affine");
  return write_file(out_path, {{out.data(), 8 * out.size()}}, std::string("cannot open output file ") + out_path, std::string("cannot write ") + out_path) ? 0 : 1;
}

// complete --validate: the points of the key file and of the challenge proof on their curves, r canonical -- on the device like every
// check (this is the one thing `complete` then needs a GPU for).  0, or 3 with the line on stderr; nothing is written.
static int validate_completion(int curve, const char* keys_path, const char* input_path, const char* challenge_path) {
  ck(mnt753_init(0), "mnt753_init");
  CompletionInputs in;
  if (!in.load(curve, keys_path, input_path, challenge_path)) return 1;
  const size_t g1 = in.g1, g2 = in.g2;
  const std::vector<uint64_t>& keys = in.keys, &proof = in.proof;
  struct Item { const char* name; int group; const uint64_t* p; size_t n; };
  const Item items[] = {{"keys alpha_g1 | beta_g1", MNT753_G1, keys.data(), 2}, {"keys beta_g2", MNT753_G2, keys.data() + 2 * g1, 1},
                        {"keys delta_g1", MNT753_G1, keys.data() + 2 * g1 + g2, 1}, {"keys delta_g2", MNT753_G2, keys.data() + 3 * g1 + g2, 1},
                        {"proof A", MNT753_G1, proof.data(), 1}, {"proof B", MNT753_G2, proof.data() + g1, 1}, {"proof C", MNT753_G1, proof.data() + g1 + g2, 1}};
  mnt753_check_report rep;
  for (const Item& it : items) {
    ck(mnt753_check_points(curve, it.group, it.p, 0, it.n, &rep, nullptr), "mnt753_check_points");
    if (rep.n_bad) { fprintf(stderr, "main_hip: %s: %llu bad, first at %llu: %s\n", it.name, (unsigned long long)rep.n_bad, (unsigned long long)rep.first_bad, reason_text(curve, (int)rep.first_reason)); return 3; }
  }
  ck(mnt753_check_scalars(curve, in.r, 0, 1, &rep, nullptr), "mnt753_check_scalars");
  if (rep.n_bad) { fprintf(stderr, "main_hip: r: 1 bad, first at 0: not canonical\n"); return 3; }
  return 0;
}

// The constraint system of the file as the device holds it, with the evaluation domain compute-r1cs chooses for it.
static void device_system(int curve, const R1csFile& sys, bool mixed, R1csHandle& r, DomainHandle& d) {
  const uint64_t* rpp[3] = {sys.rp[0].data(), sys.rp[1].data(), sys.rp[2].data()};
  const uint32_t* cp[3] = {sys.col[0].data(), sys.col[1].data(), sys.col[2].data()};
  const uint64_t* fp[3] = {sys.cf[0].data(), sys.cf[1].data(), sys.cf[2].data()};
  mnt753_r1cs* raw_r = nullptr;
  ck(mnt753_r1cs_create(curve, sys.head[0], sys.head[1], sys.head[2], rpp, cp, fp, &raw_r), "mnt753_r1cs_create");
  r.reset(raw_r);
  mnt753_domain* raw_d = nullptr;
  ck(mnt753_domain_create_for_ex(curve, mnt753_r1cs_domain_size(raw_r), mixed ? MNT753_DOMAIN_ALLOW_MIXED : 0u, &raw_d), "mnt753_domain_create_for");
  d.reset(raw_d);
}
static DevMem dev_alloc(size_t bytes) {
  void* p = nullptr;
  ck(mnt753_dev_alloc(&p, bytes), "mnt753_dev_alloc");
  return DevMem(p);
}

// `main_hip <curve> qap-at <r1cs> <t_file> <output> [--mixed-radix]`: r1cs_to_qap_instance_map_with_evaluation at the point of <t_file>
// (libsnark/reductions/r1cs_to_qap/r1cs_to_qap.tcc:105-175) on the domain compute-r1cs chooses; writes At | Bt | Ct | Ht | Zt.
static int qap_at(const Options& o, int curve, const char* r1cs_path, const char* t_path, const char* out_path) {
  uint64_t t[12];
  if (!read_exact(t_path, t, 96, true, std::string("cannot open ") + t_path, std::string(t_path) + " must hold exactly one Fr element (96 bytes)")) return 1;
  ck(mnt753_init(0), "mnt753_init");
  mnt753_check_report rep;
  ck(mnt753_check_scalars(curve, t, 0, 1, &rep, nullptr), "mnt753_check_scalars");
  if (rep.n_bad) { fprintf(stderr, "main_hip: %s: t is not below r\n", t_path); return 1; }
  R1csFile sys;
  if (!sys.load(r1cs_path)) return 1;
  R1csHandle r;
  DomainHandle d;
  device_system(curve, sys, o.mixed_radix, r, d);
  const size_t nv = sys.head[1] + 1, dm = mnt753_domain_size(d.get()), total = 3 * nv + dm + 1;
  const DevMem dev = dev_alloc(96 * total);
  uint64_t* v = static_cast<uint64_t*>(dev.get());
  std::vector<uint64_t> out(12 * (total + 1));
  ck(mnt753_r1cs_qap_at(r.get(), d.get(), t, v, v + 12 * nv, v + 24 * nv, v + 36 * nv, out.data() + 12 * total, nullptr), "mnt753_r1cs_qap_at");
  ck(mnt753_sync(nullptr), "mnt753_sync");
  ck(mnt753_copy_d2h(out.data(), dev.get(), 96 * total), "mnt753_copy_d2h");
  const std::string cannot_write = std::string("cannot write ") + out_path;
  return write_file(out_path, {{out.data(), 8 * out.size()}}, cannot_write, cannot_write) ? 0 : 1;
}

static bool write_words(const std::string& path, const std::vector<std::pair<const uint64_t*, size_t>>& parts) {
  std::vector<std::pair<const void*, size_t>> bytes;
  for (auto& p : parts) bytes.emplace_back(p.first, 8 * p.second);
  return write_file(path, bytes, "cannot write " + path, "cannot write " + path);
}

// `main_hip <curve> generate <r1cs> <out_dir> [--randomness <file>] [--mixed-radix]`: r1cs_gg_ppzksnark_generator (libsnark/zk_proof_systems/
// ppzksnark/r1cs_gg_ppzksnark/r1cs_gg_ppzksnark.tcc:212-362) on the device, mnt753_groth16_generate.  The randomness file is t | alpha |
// beta | delta (4 x 96 bytes) followed by the G1 generator (affine, 192 bytes); without one the four scalars come from the operating
// system's generator (getrandom, 753-bit draws rejected at r and, for alpha, beta and delta, at zero), the G1 generator is G1::one(),
// and the scalars are written nowhere.  Files: params.bin (the challenge layout, generate_parameters.cpp:60-85), keys.bin (what
// `complete` reads), vk_elements.bin (alpha_g1 | beta_g2 | delta_g2 | ABC_g1) and r1cs.bin (the system the key is for: a and b
// exchanged if swap_AB_if_beneficial fired -- the file compute-r1cs must be given).
static int generate_key(const Options& o, int curve, const char* r1cs_path, const char* out_dir, const char* rand_path) {
  uint64_t rnd[4 * 12 + 24];
  ck(mnt753_init(0), "mnt753_init");
  if (rand_path) {
    if (!read_exact(rand_path, rnd, sizeof rnd, true, std::string("cannot open ") + rand_path,
                    std::string(rand_path) + " must hold t | alpha | beta | delta and the G1 generator (" + std::to_string(sizeof rnd) + " bytes)"))
      return 1;
  } else {
    for (int k = 0; k < 4; ++k) {
      for (int tries = 0;; ++tries) {
        if (tries > 1000) { fprintf(stderr, "main_hip: the system's random generator gives no element below r\n"); return 1; }
        uint64_t* x = rnd + 12 * k;
        if (getrandom(x, 96, 0) != 96) { fprintf(stderr, "main_hip: getrandom failed\n"); return 1; }
        x[11] &= ((uint64_t)1 << (753 - 704)) - 1;      // r has 753 bits
        mnt753_check_report rep;
        ck(mnt753_check_scalars(curve, x, 0, 1, &rep, nullptr), "mnt753_check_scalars");
        bool zero = true;
        for (int i = 0; i < 12; ++i) zero = zero && x[i] == 0;
        if (!rep.n_bad && !(zero && k > 0)) break;
      }
    }
    ck(mnt753_group_generator(curve, MNT753_G1, rnd + 48), "mnt753_group_generator");
  }
  R1csFile sys;
  if (!sys.load(r1cs_path)) return 1;
  if (mkdir(out_dir, 0777) != 0 && errno != EEXIST) { fprintf(stderr, "main_hip: cannot create %s\n", out_dir); return 1; }
  R1csHandle r;
  DomainHandle d;
  device_system(curve, sys, o.mixed_radix, r, d);
  mnt753_keygen_sizes sz;
  ck(mnt753_groth16_sizes(r.get(), d.get(), &sz), "mnt753_groth16_sizes");
  const size_t w1 = mnt753_affine_words(curve, MNT753_G1), w2 = mnt753_affine_words(curve, MNT753_G2);
  const size_t words[6] = {w1 * sz.a_query, w1 * sz.b_g1_query, w2 * sz.b_g2_query, w1 * sz.l_query, w1 * sz.h_query, w1 * sz.abc_g1};
  size_t off[7] = {0};
  for (int k = 0; k < 6; ++k) off[k + 1] = off[k] + words[k];
  const DevMem dev = dev_alloc(8 * off[6]);
  uint64_t* v = static_cast<uint64_t*>(dev.get());
  std::vector<uint64_t> host(off[6] + 1), single(3 * w1 + 2 * w2);
  uint64_t *alpha_g1 = single.data(), *beta_g1 = alpha_g1 + w1, *beta_g2 = beta_g1 + w1, *delta_g1 = beta_g2 + w2, *delta_g2 = delta_g1 + w1;
  const mnt753_keygen_out out = {v + off[0], v + off[1], v + off[2], v + off[3], v + off[4], v + off[5], alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2};
  mnt753_keygen_report rep;
  const int rc = mnt753_groth16_generate(r.get(), d.get(), rnd, rnd + 12, rnd + 24, rnd + 36, rnd + 48, nullptr, &out, &rep, nullptr);
  if (rc == MNT753_EINVAL) { fprintf(stderr, "main_hip: %s\n", mnt753_last_error()); return 3; }
  ck(rc, "mnt753_groth16_generate");
  ck(mnt753_copy_d2h(host.data(), dev.get(), 8 * off[6]), "mnt753_copy_d2h");
  const uint64_t d_minus_1 = mnt753_domain_size(d.get()) - 1, header[2] = {d_minus_1, sys.head[1]};
  const std::string dir(out_dir);
  const uint64_t* h = host.data();
  if (!write_words(dir + "/params.bin", {{header, 2}, {h + off[0], words[0]}, {h + off[1], words[1]}, {h + off[2], words[2]}, {h + off[3], words[3]}, {h + off[4], words[4]}}))
    return 1;
  if (!write_words(dir + "/keys.bin", {{alpha_g1, w1}, {beta_g1, w1}, {beta_g2, w2}, {delta_g1, w1}, {delta_g2, w2}})) return 1;
  if (!write_words(dir + "/vk_elements.bin", {{alpha_g1, w1}, {beta_g2, w2}, {delta_g2, w2}, {h + off[5], words[5]}})) return 1;
  const int as_is[3] = {0, 1, 2}, exchanged[3] = {1, 0, 2};
  if (!sys.store((dir + "/r1cs.bin").c_str(), rep.swapped ? exchanged : as_is)) { fprintf(stderr, "main_hip: cannot write %s/r1cs.bin\n", out_dir); return 1; }
  if (!o.quiet)
    printf("generate: %llu variables, %llu constraints, domain of %llu elements; non-zero At %llu, Bt %llu; a and b %s\n", (unsigned long long)sys.head[1],
           (unsigned long long)sys.head[2], (unsigned long long)(d_minus_1 + 1), (unsigned long long)rep.non_zero_at, (unsigned long long)rep.non_zero_bt,
           rep.swapped ? "exchanged" : "as given");
  return 0;
}

// `main_hip <curve> vk <vk_elements.bin> <out>` writes the complete verification key (the reference's vk.txt: mnt753_vk_serialize);
// `main_hip <curve> verify <vk_elements.bin> <input_or_witness> <proof> [<proof> ...]` prints VERIFIED or REJECTED per proof
// (B::verify = mnt753_vk_create + mnt753_groth16_verify) and exits 0 if all are accepted, 3 otherwise.  With --check-subgroup the key's
// beta_g2 and delta_g2 go through B::check_subgroup first (a bad key: a message naming the element, exit 3, nothing verified), the
// proofs are verified with MNT753_VERIFY_CHECK_SUBGROUP, and a B outside G2 prints REJECTED (B not in the subgroup).  vk_elements.bin: alpha_g1 | beta_g2 | delta_g2 | ABC_g1, so
// its size gives num_inputs; the input (or witness) file starts with 1 and the num_inputs public inputs.
static bool read_all_words(const char* path, std::vector<uint64_t>& out) {
  return read_words(path, out, std::string("cannot read ") + path, std::string(path) + " is not a whole number of words");
}
// --fold: the batch through B::verify_folded first (one final exponentiation); its coefficients come from
// --fold-coefficients <file> (n x 16 bytes, none zero) or from getrandom.  Accepted: one line "VERIFIED <n> proofs (folded)", exit 0.
// Rejected: the per-proof pass of --check-subgroup names the proofs, exit 3.  The key's beta_g2 and delta_g2 are tested first, as
// with --check-subgroup: the fold is sound only with both in G2.
static bool fold_coefficients(const char* path, size_t n, std::vector<uint64_t>& out) {
  out.assign(2 * n, 0);
  if (path) {
    std::vector<uint64_t> w;
    if (!read_all_words(path, w)) return false;
    if (w.size() != 2 * n) { fprintf(stderr, "main_hip: %s does not hold one 128-bit coefficient per proof\n", path); return false; }
    out = w;
    return true;
  }
  for (size_t k = 0; k < n; ++k)
    while (!(out[2 * k] | out[2 * k + 1]))
      if (getrandom(&out[2 * k], 16, 0) != 16) { fprintf(stderr, "main_hip: getrandom failed\n"); return false; }
  return true;
}
struct VerifyOptions {
  bool check_subgroup = false, fold = false, fold_locate = false, compressed = false, input_tables = false, quiet = false;
  int input_window_bits = 0;   // --input-window-bits: 0 leaves the width to the library
  const char* fold_file = nullptr;
};
// --input-tables: the key of every B::verify* call below is prepared first (mnt753_vk_prepare_inputs); the
// first call that builds tables prints their plan unless --quiet
template <typename B>
struct TablePlanLine {
  typename B::input_table_plan plan{0, 0, 0};
  typename B::input_tables tables;
  bool printed = false;
  explicit TablePlanLine(const VerifyOptions& vo) {
    tables.enabled = vo.input_tables;
    tables.window_bits = vo.input_window_bits;
    tables.plan = &plan;
  }
  void print(const VerifyOptions& vo) {
    if (!vo.input_tables || vo.quiet || printed) return;
    printf("input tables: w = %d, W = %d, %llu bytes\n", plan.window_bits, plan.windows, (unsigned long long)plan.table_bytes);
    printed = true;
  }
};

// ---- compressed proofs: libff's stream of A | B | C with point compression on, 390 (MNT4753) or 486 (MNT6753) bytes ----
// the records of a proof: group and words of x, in the order of the file
struct ProofPart { const char* name; int group; size_t xw; };
static std::vector<ProofPart> proof_parts(int curve) {
  return {{"A", MNT753_G1, 12}, {"B", MNT753_G2, mnt753_compressed_words(curve, MNT753_G2)}, {"C", MNT753_G1, 12}};
}
static size_t proof_stream_bytes(int curve) { return 3 * 2 + 8 * (24 + mnt753_compressed_words(curve, MNT753_G2)); }
// the stream of one proof -> its packed form x_A | x_B | x_C and three flag bytes; false (with the line on stderr) for a file that is
// no such stream
static bool read_proof_stream(int curve, const char* path, uint64_t* x, uint8_t* flags) {
  std::vector<uint8_t> bytes(proof_stream_bytes(curve));
  const std::string wrong = std::string(path) + " is not a compressed proof (" + std::to_string(bytes.size()) + " bytes)";
  if (!read_exact(path, bytes.data(), bytes.size(), true, std::string("cannot open ") + path, wrong)) return false;
  size_t at = 0, k = 0;
  for (const ProofPart& p : proof_parts(curve)) {
    if (mnt753_points_from_stream(curve, p.group, bytes.data() + at, 8 * p.xw + 2, 1, x, flags + k) != 0) {
      fprintf(stderr, "main_hip: %s: %s: %s\n", path, p.name, mnt753_last_error());
      return false;
    }
    at += 8 * p.xw + 2; x += p.xw; ++k;
  }
  return true;
}
// `main_hip <curve> compress-proof <proof> <out>`: A | B | C in wire words -> the stream.  Validates nothing, like libff's operator<<.
template <typename B>
static int compress_proof(int curve, const char* in_path, const char* out_path) {
  const size_t w2 = mnt753_affine_words(curve, MNT753_G2);
  std::vector<uint64_t> proof(48 + w2);
  const std::string wrong = std::string(in_path) + " is not a proof A | B | C";
  if (!read_exact(in_path, proof.data(), 8 * proof.size(), true, std::string("cannot open ") + in_path, wrong)) return 1;
  if (mnt753_init(0) != 0) { fprintf(stderr, "main_hip: %s\n", mnt753_last_error()); return 1; }
  std::vector<uint8_t> out(proof_stream_bytes(curve));
  size_t at = 0, from = 0;
  for (const ProofPart& p : proof_parts(curve)) {
    const auto c = B::compress_points(p.group, proof.data() + from, 1);
    size_t len = 0;
    ck(mnt753_points_to_stream(curve, p.group, c.x.data(), c.flags.data(), 1, out.data() + at, out.size() - at, &len), "mnt753_points_to_stream");
    at += len; from += 2 * p.xw;
  }
  const std::string cannot_write = std::string("cannot write ") + out_path;
  return write_file(out_path, {{out.data(), out.size()}}, cannot_write, cannot_write) ? 0 : 1;
}
// `main_hip <curve> decompress-proof <in> <out>`: the stream -> A | B | C in wire words; a record that is not a point ("A: off curve",
// "B: not canonical") or a file that is no stream: exit 3, nothing written
template <typename B>
static int decompress_proof(int curve, const char* in_path, const char* out_path) {
  std::vector<uint64_t> x(24 + mnt753_compressed_words(curve, MNT753_G2));
  uint8_t flags[3];
  if (!read_proof_stream(curve, in_path, x.data(), flags)) return 3;
  if (mnt753_init(0) != 0) { fprintf(stderr, "main_hip: %s\n", mnt753_last_error()); return 1; }
  std::vector<uint64_t> proof;
  size_t from = 0, k = 0;
  bool ok = true;
  for (const ProofPart& p : proof_parts(curve)) {
    const auto d = B::decompress_points(p.group, x.data() + from, flags + k, 1);
    if (d.report.n_bad) { fprintf(stderr, "main_hip: %s: %s: %s\n", in_path, p.name, B::check_reason_text(d.report.reason)); ok = false; }
    proof.insert(proof.end(), d.affine.begin(), d.affine.end());
    from += p.xw; ++k;
  }
  if (!ok) return 3;
  const std::string cannot_write = std::string("cannot write ") + out_path;
  return write_file(out_path, {{proof.data(), 8 * proof.size()}}, cannot_write, cannot_write) ? 0 : 1;
}
// verify --compressed: the proof files are streams; a proof that does not decompress prints REJECTED (malformed)
template <typename B>
static int verify_compressed_batch(const VerifyOptions& vo, const std::vector<uint64_t>& el, size_t num_inputs, const std::vector<uint64_t>& x,
                                   const std::vector<uint8_t>& flags, const std::vector<uint64_t>& per_proof, size_t n) {
  if (vo.check_subgroup) {
    const auto e = B::check_subgroup(el.data() + 24, 2);
    if (e.n_bad) {
      fprintf(stderr, "main_hip: %s of the key: %s\n", e.first_bad == 0 ? "beta_g2" : "delta_g2", B::check_reason_text(e.reason));
      return 3;
    }
  }
  TablePlanLine<B> tp(vo);
  const std::vector<uint8_t> verdicts = B::verify_compressed(el.data(), num_inputs, x.data(), flags.data(), per_proof.data(), n, vo.check_subgroup, tp.tables);
  tp.print(vo);
  int bad = 0;
  for (size_t k = 0; k < n; ++k) {
    printf("%s\n", verdicts[k] == 0 ? "VERIFIED" : (verdicts[k] == 3 ? "REJECTED (B not in the subgroup)" : (verdicts[k] == 1 ? "REJECTED (malformed)" : "REJECTED")));
    bad += verdicts[k] != 0;
  }
  return bad ? 3 : 0;
}
// through the wrapper class, as a C++ caller would: B::verify makes the key, verifies the batch and drops the key
template <typename B>
static int verify_batch(const VerifyOptions& vo, const std::vector<uint64_t>& el, size_t num_inputs, const std::vector<uint64_t>& proofs,
                        const std::vector<uint64_t>& per_proof, size_t n, const std::vector<uint64_t>& coef) {
  std::vector<uint8_t> verdicts;
  TablePlanLine<B> tp(vo);
  if (vo.check_subgroup) {
    // beta_g2 | delta_g2 lie side by side in the file
    const auto e = B::check_subgroup(el.data() + 24, 2);
    if (e.n_bad) {
      fprintf(stderr, "main_hip: %s of the key: %s\n", e.first_bad == 0 ? "beta_g2" : "delta_g2", B::check_reason_text(e.reason));
      return 3;
    }
    if (vo.fold_locate) {
      // --fold-locate: one tail per segment; only the rejected segments pay the per-proof pass
      const auto located = B::verify_folded_locate(el.data(), num_inputs, proofs.data(), per_proof.data(), n, coef.data(), tp.tables);
      fprintf(stderr, "fold: %llu segments, %llu rejected, %llu proofs rechecked\n", (unsigned long long)located.report.segments,
              (unsigned long long)located.report.segments_rejected, (unsigned long long)located.report.proofs_rechecked);
      verdicts = located.verdicts;
    } else if (vo.fold && B::verify_folded(el.data(), num_inputs, proofs.data(), per_proof.data(), n, coef.data(), tp.tables).accepted) {
      tp.print(vo);
      printf("VERIFIED %zu proofs (folded)\n", n);
      return 0;
    } else {                                       // --check-subgroup alone, or a fold that rejected: the per-proof pass names the proofs
      verdicts = B::verify(el.data(), num_inputs, proofs.data(), per_proof.data(), n, true, tp.tables);
    }
  } else {
    verdicts = B::verify(el.data(), num_inputs, proofs.data(), per_proof.data(), n, false, tp.tables);
  }
  tp.print(vo);
  int bad = 0;
  for (size_t k = 0; k < n; ++k) {
    printf("%s\n", verdicts[k] == 0 ? "VERIFIED" : (verdicts[k] == 3 ? "REJECTED (B not in the subgroup)" : "REJECTED"));
    bad += verdicts[k] != 0;
  }
  return bad ? 3 : 0;
}
// pos: <vk_elements.bin> (read: el, num_inputs) <input_or_witness> <proof> [<proof> ...]
static int verify_proofs(int curve, const std::vector<const char*>& pos, const VerifyOptions& vo, const std::vector<uint64_t>& el, size_t num_inputs) {
  const size_t w2 = mnt753_affine_words(curve, MNT753_G2);
  std::vector<uint64_t> proofs, coef;
  std::vector<uint64_t> inputs(12 * (num_inputs + 1));
  const std::string cannot_read = "cannot read 1 + " + std::to_string(num_inputs) + " elements from " + pos[1];
  if (!read_exact(pos[1], inputs.data(), 8 * inputs.size(), false, cannot_read, cannot_read)) return 1;
  // the leading element is the constant 1: R mod r, the Montgomery one of Fr (modulus A on MNT4753, B on MNT6753)
  if (memcmp(inputs.data(), mnt753::FPC[curve].one64, 96) != 0) { fprintf(stderr, "main_hip: %s does not start with the constant 1\n", pos[1]); return 3; }
  const size_t n = pos.size() - 2;
  if (vo.compressed) {
    const size_t xw = 24 + mnt753_compressed_words(curve, MNT753_G2);
    std::vector<uint64_t> x(n * xw);
    std::vector<uint8_t> flags(3 * n);
    for (size_t k = 0; k < n; ++k)
      if (!read_proof_stream(curve, pos[k + 2], x.data() + k * xw, flags.data() + 3 * k)) return 3;
    if (mnt753_init(0) != 0) { fprintf(stderr, "main_hip: %s\n", mnt753_last_error()); return 1; }
    std::vector<uint64_t> rows;
    for (size_t k = 0; k < n; ++k) rows.insert(rows.end(), inputs.begin() + 12, inputs.end());
    return with_curve(curve, [&](auto b) { return verify_compressed_batch<decltype(b)>(vo, el, num_inputs, x, flags, rows, n); });
  }
  for (size_t k = 2; k < pos.size(); ++k) {
    std::vector<uint64_t> one;
    if (!read_all_words(pos[k], one)) return 1;
    if (one.size() != 48 + w2) { fprintf(stderr, "main_hip: %s is not a proof A | B | C\n", pos[k]); return 3; }
    proofs.insert(proofs.end(), one.begin(), one.end());
  }
  if ((vo.fold || vo.fold_locate) && !fold_coefficients(vo.fold_file, n, coef)) return 1;
  if (mnt753_init(0) != 0) { fprintf(stderr, "main_hip: %s\n", mnt753_last_error()); return 1; }
  std::vector<uint64_t> per_proof;
  for (size_t k = 0; k < n; ++k) per_proof.insert(per_proof.end(), inputs.begin() + 12, inputs.end());
  return with_curve(curve, [&](auto b) { return verify_batch<decltype(b)>(vo, el, num_inputs, proofs, per_proof, n, coef); });
}
// pos: <vk_elements.bin> <out>, or what verify_proofs reads
static int vk_or_verify(int curve, bool verify, const std::vector<const char*>& pos, const VerifyOptions& vo) {
  const size_t w2 = mnt753_affine_words(curve, MNT753_G2);
  std::vector<uint64_t> el;
  if (!read_all_words(pos[0], el)) return 1;
  if (el.size() < 48 + 2 * w2 || (el.size() - 24 - 2 * w2) % 24) { fprintf(stderr, "main_hip: %s does not hold alpha_g1 | beta_g2 | delta_g2 | ABC_g1\n", pos[0]); return 3; }
  const size_t num_inputs = (el.size() - 24 - 2 * w2) / 24 - 1;
  if (verify) return verify_proofs(curve, pos, vo, el, num_inputs);
  if (mnt753_init(0) != 0) { fprintf(stderr, "main_hip: %s\n", mnt753_last_error()); return 1; }
  mnt753_vk* raw = nullptr;
  const int rc = mnt753_vk_create(curve, el.data(), el.data() + 24, el.data() + 24 + w2, el.data() + 24 + 2 * w2, num_inputs, &raw);
  if (rc != 0) { fprintf(stderr, "main_hip: %s\n", mnt753_last_error()); return rc == MNT753_EINPUT || rc == MNT753_EINVAL ? 3 : 1; }
  const VkHandle vk(raw);
  size_t len = 0;
  mnt753_vk_serialize(vk.get(), nullptr, 0, &len);
  std::vector<uint8_t> bytes(len);
  if (mnt753_vk_serialize(vk.get(), bytes.data(), len, &len) != 0) { fprintf(stderr, "main_hip: %s\n", mnt753_last_error()); return 1; }
  const std::string cannot_write = std::string("cannot write ") + pos[1];
  return write_file(pos[1], {{bytes.data(), len}}, cannot_write, cannot_write) ? 0 : 1;
}

// ---- the command line ----

static int parse_curve(const char* name) { return !strcmp(name, "MNT4753") ? 0 : (!strcmp(name, "MNT6753") ? 1 : -1); }
static int unknown_curve(const char* name) { fprintf(stderr, "unknown curve %s\n", name); return 2; }
// the usage text with the program's name for every %s; the exit code of a command line that cannot be read
static int usage(const char* text, const char* prog) {
  for (const char* p = text; *p; ++p) {
    if (p[0] == '%' && p[1] == 's') { fputs(prog, stderr); ++p; }
    else fputc(*p, stderr);
  }
  return 2;
}

// One walk over a command's words from argv[i] on.  next() stops at each word in turn: a flag of the command's list (`flag` is its
// name, `value` its value if it takes one), or a positional (`flag` is null, `value` the word).  A word that starts with '-' and is no
// flag of the list, or a flag that has lost its value, ends the walk: "main_hip: unknown option <word>", `refused`.
struct Flag { const char* name; bool takes_value; };
struct ArgScan {
  int argc; char** argv; int i;
  std::vector<Flag> flags;
  bool lenient = false;   // words the list does not know are passed over, each with the word behind it (complete)
  const char *flag = nullptr, *value = nullptr;
  bool refused = false;
  bool next() {
    while (i < argc) {
      const char* w = argv[i++];
      flag = value = nullptr;
      for (const Flag& f : flags)
        if (!strcmp(w, f.name) && (!f.takes_value || i < argc)) { flag = f.name; if (f.takes_value) value = argv[i++]; return true; }
      if (lenient) { ++i; continue; }
      if (w[0] == '-') { fprintf(stderr, "main_hip: unknown option %s\n", w); refused = true; return false; }
      value = w;
      return true;
    }
    return false;
  }
  bool is(const char* name) const { return flag && !strcmp(flag, name); }
  // the word behind a positional if it is a positional too (taken), else null
  const char* positional_behind() { return i < argc && argv[i][0] != '-' ? argv[i++] : nullptr; }
};

struct Command {
  const char* name;
  int (*run)(const Command& self, Options& o, int argc, char** argv);   // reads its words into o (and its own options), then works
  bool second_form;   // of a function that serves two commands: compute-r1cs, check-r1cs, verify
  const char* usage;
};
static int prove_command(const Command&, Options&, int, char**);
static int complete_command(const Command&, Options&, int, char**);
static int check_command(const Command&, Options&, int, char**);
static int qap_at_command(const Command&, Options&, int, char**);
static int generate_command(const Command&, Options&, int, char**);
static int vk_command(const Command&, Options&, int, char**);
static int self_test_command(const Command&, Options&, int, char**);
static int proof_stream_command(const Command&, Options&, int, char**);

// also what a command line too short to name its files gets, whatever its command word
static const char compute_usage[] =
    "usage: %s MNT4753|MNT6753 compute <params> <input> <output> [<input2> <output2> ...] [--repeat N] [--serve] [--gpus N] [--tables | --one-shot] [--unfused-h] [--unfused-c] [--ref-order] [--fold rccl|host] [--validate] [--check-h] [--check-h-t <file>] [--mixed-radix] [--quiet]\n"
    "  --check-h: H(t) Z(t) = A(t) B(t) - C(t) at a random t after every compute_H (also compute-r1cs); a failing job writes nothing, exit code 3\n"
    "  --check-h-t <file>: the point t, one 96-byte element of Fr in wire form, for a reproducible run (implies --check-h)\n"
    "  further (input, output) pairs and --repeat prove against the parameters that are already resident on the GPU\n"
    "       %s MNT4753|MNT6753 qap-at <r1cs> <t_file> <output> [--mixed-radix]\n";
static const char check_usage[] =
    "usage: %s MNT4753|MNT6753 check <params> [<input>] [--subgroup] [--gpus N]\n       %s MNT4753|MNT6753 check-r1cs <params> <r1cs> <witness> [--gpus N]\n"
    "  --subgroup: the B2 points must also lie in G2, the order-r subgroup of the twist (\"not in the subgroup\")\n";
static const char vk_usage[] =
    "usage: %s MNT4753|MNT6753 vk <vk_elements.bin> <out>\n       %s MNT4753|MNT6753 verify <vk_elements.bin> <input_or_witness> <proof> [<proof> ...] [--check-subgroup] [--fold | --fold-locate [--fold-coefficients <file>]] [--compressed] [--input-tables [--input-window-bits w]] [--quiet]\n"
    "  vk: writes the complete verification key (with the GT element e(alpha_g1, beta_g2)) in the reference's vk.txt format.\n"
    "  verify: prints VERIFIED or REJECTED per proof; exit code 0 if every proof is accepted, 3 otherwise.\n"
    "  --check-subgroup: beta_g2 and delta_g2 of the key and B of every proof must lie in G2, the order-r subgroup of the twist;\n"
    "    a key that fails is named and nothing is verified (exit 3), such a proof prints REJECTED (B not in the subgroup).\n"
    "  --fold: the batch under one final exponentiation first (random coefficients, or n x 16 bytes from --fold-coefficients);\n"
    "    accepted: one line naming the count, exit 0; rejected: the per-proof lines of --check-subgroup, exit 3.\n"
    "  --fold-locate: one folded check per segment of 128 (MNT6753: 84) proofs, the per-proof pass on the rejected segments only\n"
    "    (coefficients as for --fold; implies --check-subgroup): the per-proof lines of --check-subgroup, and on stderr one line\n"
    "    \"fold: <segments> segments, <rejected> rejected, <rechecked> proofs rechecked\"; exit 0 or 3.  Not with --fold or --compressed.\n"
    "  --compressed: the proof files are libff's compressed streams (compress-proof); a proof that does not decompress prints\n"
    "    REJECTED (malformed).  Not with --fold.\n"
    "  --input-tables: the key is prepared before it verifies -- one window table per ABC point, W = ceil(754 / w) additions per public\n"
    "    input; the same lines and exit codes.  Prints one line \"input tables: w = .., W = .., .. bytes\" first unless --quiet.\n"
    "    --input-window-bits w: the width, 2 .. 16 (default: the widest whose tables fit 256 MiB).  Worth it from tens of inputs on.\n";
static const char proof_stream_usage[] =
    "usage: %s MNT4753|MNT6753 compress-proof <proof> <out>\n       %s MNT4753|MNT6753 decompress-proof <in> <out>\n"
    "  compress-proof: A | B | C in wire words -> libff's stream with point compression on (390 / 486 bytes); validates nothing.\n"
    "  decompress-proof: the reverse; a record that is no point of its curve is named (\"B: off curve\"), exit code 3, nothing is written.\n";
static const Command commands[] = {
    {"compute", prove_command, false, compute_usage},
    {"compute-r1cs", prove_command, true, "usage: %s <curve> compute-r1cs <params> <r1cs> <witness> <output>\n"},
    {"complete", complete_command, false, nullptr},   // never refuses its words: see complete_command
    {"check", check_command, false, check_usage},
    {"check-r1cs", check_command, true, check_usage},
    {"qap-at", qap_at_command, false, "usage: %s MNT4753|MNT6753 qap-at <r1cs> <t_file> <output> [--mixed-radix]\n"},
    {"generate", generate_command, false,
     "usage: %s MNT4753|MNT6753 generate <r1cs> <out_dir> [--randomness <file>] [--mixed-radix] [--quiet]\n"
     "  writes params.bin, keys.bin, vk_elements.bin (alpha_g1 | beta_g2 | delta_g2 | ABC_g1) and r1cs.bin into <out_dir>.\n"
     "  The GT element alpha_g1_beta_g2 of a libsnark verification key is a pairing of two of these: `vk <vk_elements.bin> <out>`\n"
     "  writes the complete key, `verify` checks proofs against it.\n"
     "  <file>: t | alpha | beta | delta (4 x 96 bytes) and the G1 generator (affine); without it the scalars are drawn from the\n"
     "  operating system's generator and written nowhere, and the G1 generator is the curve's standard one.\n"},
    {"vk", vk_command, false, vk_usage},
    {"verify", vk_command, true, vk_usage},
    {"compress-proof", proof_stream_command, false, proof_stream_usage},
    {"decompress-proof", proof_stream_command, true, proof_stream_usage},
    {"self-test", self_test_command, false, nullptr},   // takes no words
};
// A word that is no command (and `complete` short of its paths) has always been read as compute's line and refused only behind its
// options ("unknown mode"); it still is.
static const Command not_a_command = {nullptr, prove_command, false, compute_usage};

// compute <params> <input> <output> ... and compute-r1cs <params> <r1cs> <witness> <output> ...: one more positional argument.
static int prove_command(const Command& self, Options& o, int argc, char** argv) {
  const bool with_r1cs = self.second_form;
  if (argc < 6) return usage(compute_usage, argv[0]);
  if (with_r1cs && argc < 7) return usage(self.usage, argv[0]);
  const int a0 = with_r1cs ? 5 : 4;
  o.jobs.emplace_back(argv[a0], argv[a0 + 1]);
  ArgScan a{argc, argv, a0 + 2,
            {{"--repeat", true}, {"--gpus", true}, {"--fold", true}, {"--check-h-t", true}, {"--fused-h", false}, {"--unfused-h", false}, {"--quiet", false},
             {"--serve", false}, {"--h-first", false}, {"--h-last", false}, {"--ref-order", false}, {"--unfused-c", false}, {"--c-last", false},
             {"--touch-all", false}, {"--fused-c", false}, {"--peer-bench", false}, {"--tables", false}, {"--one-shot", false}, {"--validate", false},
             {"--check-h", false}, {"--mixed-radix", false}}};
  while (a.next()) {
    if (!a.flag) {
      // a further job is an input with its output behind it; an input without one is refused, not guessed at
      const char* output = a.positional_behind();
      if (!output) { fprintf(stderr, "main_hip: input %s without an output path\n", a.value); return 2; }
      o.jobs.emplace_back(a.value, output);
    }
    else if (a.is("--repeat")) o.repeat = atoi(a.value);
    else if (a.is("--gpus")) o.gpus = atoi(a.value);
    else if (a.is("--fold")) o.fold_rccl = !strcmp(a.value, "rccl") ? 1 : 0;
    else if (a.is("--check-h-t")) {
      const std::string not_an_element = std::string("--check-h-t ") + a.value + ": not a file of one 96-byte element";
      if (!read_exact(a.value, o.check_h_t, 96, true, not_an_element, not_an_element)) return 2;
      o.check_h = o.check_h_t_given = true;
    }
    else if (a.is("--fused-h")) o.fused_h = true;
    else if (a.is("--unfused-h")) o.fused_h = false;
    else if (a.is("--quiet")) o.quiet = true;
    else if (a.is("--serve")) o.serve = true;
    else if (a.is("--h-first")) o.h_first = true;
    else if (a.is("--h-last")) o.h_first = false;
    else if (a.is("--ref-order")) { o.h_first = false; o.explicit_c = false; }   // the call sequence of cuda_prover_piecewise.cu:64-90
    else if (a.is("--unfused-c")) o.fused_c = false;
    else if (a.is("--c-last")) o.c_first = false;
    else if (a.is("--touch-all")) o.touch_all = true;
    else if (a.is("--fused-c")) o.fused_c = true;
    else if (a.is("--peer-bench")) o.peer_bench = true;
    else if (a.is("--tables")) o.one_shot = 0;      // build the window tables even for a single proof
    else if (a.is("--one-shot")) o.one_shot = 1;    // no window tables, no warm-up MSM, whatever the job list
    else if (a.is("--validate")) o.validate = true;
    else if (a.is("--check-h")) o.check_h = true;
    else if (a.is("--mixed-radix")) o.mixed_radix = true;
  }
  if (a.refused) return 2;
  if (!self.name) { fprintf(stderr, "unknown mode %s\n", argv[2]); return 2; }
  if (o.repeat > 1) { const auto one = o.jobs; for (int k = 1; k < o.repeat; ++k) o.jobs.insert(o.jobs.end(), one.begin(), one.end()); }
  const int curve = parse_curve(argv[1]);
  if (curve < 0) return unknown_curve(argv[1]);
  const char* r1cs_path = with_r1cs ? argv[4] : nullptr;
  return with_curve(curve, [&](auto b) { return run_prover<decltype(b)>(o, argv[3], r1cs_path); });
}

static int complete_command(const Command&, Options& o, int argc, char** argv) {
  if (argc < 7) return prove_command(not_a_command, o, argc, argv);
  const int curve = parse_curve(argv[1]);
  if (curve < 0) return unknown_curve(argv[1]);
  const char* s_file = nullptr; uint64_t s_seed = 0x73656564ull;
  // kept as it was: the four paths by position, and behind them no word is refused -- one the list does not know is passed over
  ArgScan a{argc, argv, 7, {{"--validate", false}, {"--mixed-radix", false}, {"--s-file", true}, {"--s-seed", true}}, /*lenient=*/true};
  while (a.next()) {
    if (a.is("--validate")) o.validate = true;
    else if (a.is("--mixed-radix")) o.mixed_radix = true;
    else if (a.is("--s-file")) s_file = a.value;
    else if (a.is("--s-seed")) s_seed = strtoull(a.value, nullptr, 0);
  }
  mnt6753_hip::allow_mixed_radix(o.mixed_radix);
  if (o.validate) { if (int rc = validate_completion(curve, argv[3], argv[4], argv[5])) return rc; }
  return complete_proof(curve, argv[3], argv[4], argv[5], argv[6], s_file, s_seed);
}

static int check_command(const Command& self, Options& o, int argc, char** argv) {
  const bool with_r1cs = self.second_form;
  std::vector<Flag> flags = {{"--gpus", true}};
  if (!with_r1cs) flags.push_back({"--subgroup", false});
  ArgScan a{argc, argv, 3, flags};
  std::vector<const char*> pos;
  bool subgroup = false;
  while (a.next()) {
    if (a.is("--gpus")) o.gpus = atoi(a.value);
    else if (a.is("--subgroup")) subgroup = true;
    else pos.push_back(a.value);
  }
  if (a.refused) return 2;
  if (with_r1cs ? pos.size() != 3 : (pos.empty() || pos.size() > 2)) return usage(self.usage, argv[0]);
  const char* input = with_r1cs ? pos[2] : (pos.size() > 1 ? pos[1] : nullptr);
  const char* r1cs = with_r1cs ? pos[1] : nullptr;
  const int curve = parse_curve(argv[1]);
  if (curve < 0) return unknown_curve(argv[1]);
  return with_curve(curve, [&](auto b) { return run_check<decltype(b)>(o, pos[0], input, r1cs, subgroup); });
}

static int qap_at_command(const Command& self, Options& o, int argc, char** argv) {
  const int curve = parse_curve(argv[1]);
  if (curve < 0) return unknown_curve(argv[1]);
  ArgScan a{argc, argv, 3, {{"--mixed-radix", false}}};
  std::vector<const char*> pos;
  while (a.next()) {
    if (a.is("--mixed-radix")) o.mixed_radix = true;
    else pos.push_back(a.value);
  }
  if (a.refused) return 2;
  if (pos.size() != 3) return usage(self.usage, argv[0]);
  return qap_at(o, curve, pos[0], pos[1], pos[2]);
}

static int generate_command(const Command& self, Options& o, int argc, char** argv) {
  const int curve = parse_curve(argv[1]);
  if (curve < 0) return unknown_curve(argv[1]);
  ArgScan a{argc, argv, 3, {{"--mixed-radix", false}, {"--quiet", false}, {"--randomness", true}}};
  const char* rand_path = nullptr;
  std::vector<const char*> pos;
  while (a.next()) {
    if (a.is("--mixed-radix")) o.mixed_radix = true;
    else if (a.is("--quiet")) o.quiet = true;
    else if (a.is("--randomness")) rand_path = a.value;
    else pos.push_back(a.value);
  }
  if (a.refused) return 2;
  if (pos.size() != 2) return usage(self.usage, argv[0]);
  return generate_key(o, curve, pos[0], pos[1], rand_path);
}

static int vk_command(const Command& self, Options&, int argc, char** argv) {
  const bool verify = self.second_form;
  const int curve = parse_curve(argv[1]);
  if (curve < 0) return unknown_curve(argv[1]);
  std::vector<Flag> flags;
  if (verify) flags = {{"--check-subgroup", false}, {"--fold", false}, {"--fold-locate", false}, {"--fold-coefficients", true}, {"--compressed", false},
                       {"--input-tables", false}, {"--input-window-bits", true}, {"--quiet", false}};
  ArgScan a{argc, argv, 3, flags};
  std::vector<const char*> pos;
  VerifyOptions vo;
  while (a.next()) {
    if (a.is("--check-subgroup")) vo.check_subgroup = true;
    else if (a.is("--compressed")) vo.compressed = true;
    else if (a.is("--fold")) vo.fold = vo.check_subgroup = true;
    else if (a.is("--fold-locate")) vo.fold_locate = vo.check_subgroup = true;
    else if (a.is("--fold-coefficients")) vo.fold_file = a.value;
    else if (a.is("--input-tables")) vo.input_tables = true;
    else if (a.is("--quiet")) vo.quiet = true;
    else if (a.is("--input-window-bits")) {
      char* end = nullptr;
      const long w = strtol(a.value, &end, 10);
      if (!*a.value || *end || w < 2 || w > 16) { fprintf(stderr, "main_hip: --input-window-bits %s: not a width in 2 .. 16\n", a.value); return 2; }
      vo.input_window_bits = (int)w;
    }
    else pos.push_back(a.value);
  }
  if (a.refused) return 2;
  if (verify ? pos.size() < 3 : pos.size() != 2) return usage(self.usage, argv[0]);
  if (vo.fold_locate && vo.fold) { fprintf(stderr, "main_hip: --fold-locate and --fold are two verifiers: name one\n"); return 2; }
  if (vo.fold_locate && vo.compressed) { fprintf(stderr, "main_hip: --fold-locate takes no compressed proofs\n"); return 2; }
  if (vo.compressed && vo.fold) { fprintf(stderr, "main_hip: --fold takes no compressed proofs\n"); return 2; }
  if (vo.input_window_bits && !vo.input_tables) { fprintf(stderr, "main_hip: --input-window-bits goes with --input-tables\n"); return 2; }
  return vk_or_verify(curve, verify, pos, vo);
}

// compress-proof <proof> <out> and decompress-proof <in> <out>
static int proof_stream_command(const Command& self, Options&, int argc, char** argv) {
  const int curve = parse_curve(argv[1]);
  if (curve < 0) return unknown_curve(argv[1]);
  ArgScan a{argc, argv, 3, {}};
  std::vector<const char*> pos;
  while (a.next()) pos.push_back(a.value);
  if (a.refused) return 2;
  if (pos.size() != 2) return usage(self.usage, argv[0]);
  return with_curve(curve, [&](auto b) {
    return self.second_form ? decompress_proof<decltype(b)>(curve, pos[0], pos[1]) : compress_proof<decltype(b)>(curve, pos[0], pos[1]);
  });
}

// `main_hip <curve> self-test`: the known-answer checks of this build at their widest (level 2: also over window tables)
static int self_test_command(const Command&, Options&, int, char**) {
  if (mnt753_init(0) != 0) { fprintf(stderr, "main_hip: %s\n", mnt753_last_error()); return 1; }
  const int rc = mnt753_self_test(2);
  if (rc != 0) { fprintf(stderr, "main_hip: %s\n", mnt753_last_error()); return 1; }
  printf("self-test: all known answers of the reference agree (level 2)\n");
  return 0;
}

int main(int argc, char** argv) {
  setbuf(stdout, NULL);
  Options o;
  read_environment(o);
  const Command* command = &not_a_command;
  for (const Command& c : commands)
    if (argc >= 3 && !strcmp(argv[2], c.name)) command = &c;
  try {
    return command->run(*command, o, argc, argv);
  } catch (const std::exception& e) {
    fprintf(stderr, "main_hip: %s\n", e.what());
    return 1;
  }
}
