// mint_keygen.cpp -- mints Groth16 keys from GIVEN randomness with the reference's own functions (TEST INFRASTRUCTURE;
// tools/mint_keygen.sh compiles and runs it).
//
// OUR program, compiled against the REFERENCE's own libsnark / libff / libfqfft where they lie, with the flags and objects of
// oracle/build_ref.sh.  Nothing in it is this repository's arithmetic: the swap, the instance map, the window tables, the batch
// exponentiations, the pairing and the serialisation all come from MinaProtocol/snark-challenge-prover-reference code.  It walks the
// steps of r1cs_gg_ppzksnark_generator (libsnark/zk_proof_systems/ppzksnark/r1cs_gg_ppzksnark/r1cs_gg_ppzksnark.tcc:212-362) with the
// values that function draws inside itself (:216-219, :290) read from a file, so that the key is a function of its inputs.
//
//   mint_keygen <MNT4753|MNT6753> <r1cs_in.bin> <scalars.bin> <witness.bin> <out_dir> <g1_multiple>
//               <expect_touched_a> <expect_touched_b> <expect_class> <expect_m> <expect_untouched>
//
// scalars.bin: t | alpha | beta | delta, wire format.  The G1 generator is <g1_multiple> * G1::one().  witness.bin: w[0 .. m] | r.
// The expectations are properties the fixture is chosen for (tools/mint_keygen.sh); the program fails if one does not hold.
// Writes into <out_dir>:
//   randomness.bin     t | alpha | beta | delta | G1 generator (affine)
//   r1cs.bin           the system after swap_AB_if_beneficial (layout: oracle/ref_groth16.cpp)
//   params.bin         the challenge layout of generate_parameters.cpp:60-85 (d = domain size - 1)
//   keys.bin           alpha_g1 | beta_g1 | beta_g2 | delta_g1 | delta_g2
//   vk_elements.bin    alpha_g1 | beta_g2 | delta_g2 | ABC_g1 (num_inputs + 1 points)
//   vk.txt             operator<< of the verification key (alpha_g1_beta_g2 from reduced_pairing)
//   input.bin          as `ref_groth16 mint` writes it: w | ca | cb | cc (domain size each, of the swapped system) | r
// and prints one line of key=value pairs for the index.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include <omp.h>

#include <libff/common/profiling.hpp>
#include <libff/algebra/curves/mnt753/mnt4753/mnt4753_pp.hpp>
#include <libff/algebra/curves/mnt753/mnt6753/mnt6753_pp.hpp>
#include <libff/algebra/scalar_multiplication/multiexp.hpp>
#include <libfqfft/evaluation_domain/domains/basic_radix2_domain.hpp>
#include <libfqfft/evaluation_domain/domains/extended_radix2_domain.hpp>
#include <libfqfft/evaluation_domain/domains/step_radix2_domain.hpp>
#include <libsnark/serialization.hpp>
#include <libsnark/knowledge_commitment/kc_multiexp.hpp>
#include <libsnark/reductions/r1cs_to_qap/r1cs_to_qap.hpp>
#include <libsnark/zk_proof_systems/ppzksnark/r1cs_gg_ppzksnark/r1cs_gg_ppzksnark.hpp>

using namespace libsnark;
using namespace libff;

static FILE* open_or_die(const std::string& p, const char* mode) {
  FILE* f = fopen(p.c_str(), mode);
  if (!f) { perror(p.c_str()); exit(1); }
  return f;
}
static uint64_t get_u64(FILE* f) {
  uint64_t v = 0;
  if (fread(&v, 8, 1, f) != 1) { fprintf(stderr, "short read\n"); exit(1); }
  return v;
}
static void put_u64(FILE* f, uint64_t v) { fwrite(&v, 8, 1, f); }
#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "mint_keygen: expectation failed: " __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

template <typename ppT>
r1cs_constraint_system<Fr<ppT>> read_r1cs(const std::string& path) {
  typedef Fr<ppT> F;
  FILE* f = open_or_die(path, "rb");
  const uint64_t num_inputs = get_u64(f), m = get_u64(f), nc = get_u64(f);
  r1cs_constraint_system<F> cs;
  cs.primary_input_size = num_inputs;
  cs.auxiliary_input_size = m - num_inputs;
  cs.constraints.resize(nc);
  for (int which = 0; which < 3; ++which) {
    std::vector<uint64_t> row_ptr(nc + 1);
    for (auto& v : row_ptr) v = get_u64(f);
    std::vector<uint32_t> col(row_ptr[nc]);
    if (!col.empty() && fread(col.data(), 4, col.size(), f) != col.size()) { fprintf(stderr, "short read\n"); exit(1); }
    for (uint64_t i = 0; i < nc; ++i) {
      linear_combination<F>& lc = which == 0 ? cs.constraints[i].a : (which == 1 ? cs.constraints[i].b : cs.constraints[i].c);
      for (uint64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
        const F coeff = read_fr<ppT>(f);
        lc.terms.emplace_back(linear_term<F>(variable<F>(col[k]), coeff));
      }
    }
  }
  fclose(f);
  return cs;
}

template <typename ppT>
void write_r1cs(const std::string& path, const r1cs_constraint_system<Fr<ppT>>& cs) {
  FILE* f = open_or_die(path, "wb");
  const size_t nc = cs.num_constraints();
  put_u64(f, cs.num_inputs()); put_u64(f, cs.num_variables()); put_u64(f, nc);
  for (int which = 0; which < 3; ++which) {
    auto lc = [&](size_t i) -> const linear_combination<Fr<ppT>>& {
      return which == 0 ? cs.constraints[i].a : (which == 1 ? cs.constraints[i].b : cs.constraints[i].c);
    };
    uint64_t nnz = 0;
    put_u64(f, 0);
    for (size_t i = 0; i < nc; ++i) { nnz += lc(i).terms.size(); put_u64(f, nnz); }
    for (size_t i = 0; i < nc; ++i)
      for (auto& t : lc(i).terms) { uint32_t c = (uint32_t)t.index; fwrite(&c, 4, 1, f); }
    for (size_t i = 0; i < nc; ++i)
      for (auto& t : lc(i).terms) write_fr<ppT>(f, t.coeff);
  }
  fclose(f);
}

template <typename F>
const char* class_of(libfqfft::evaluation_domain<F>* d) {
  if (dynamic_cast<libfqfft::basic_radix2_domain<F>*>(d)) return "basic_radix2_domain";
  if (dynamic_cast<libfqfft::extended_radix2_domain<F>*>(d)) return "extended_radix2_domain";
  if (dynamic_cast<libfqfft::step_radix2_domain<F>*>(d)) return "step_radix2_domain";
  return "other";
}

// variables a term of the chosen matrix names (what swap_AB_if_beneficial counts, r1cs.tcc:199-219)
template <typename F>
std::vector<bool> touched(const r1cs_constraint_system<F>& cs, int which) {
  std::vector<bool> t(cs.num_variables() + 1, false);
  for (auto& c : cs.constraints) {
    const linear_combination<F>& lc = which == 0 ? c.a : (which == 1 ? c.b : c.c);
    for (auto& term : lc.terms) t[term.index] = true;
  }
  return t;
}
static size_t count_true(const std::vector<bool>& v) { size_t n = 0; for (bool b : v) n += b; return n; }

template <typename ppT>
int mint(char** argv) {
  typedef Fr<ppT> F;
  typedef G1<ppT> P1;
  typedef G2<ppT> P2;
  ppT::init_public_params();
  libff::inhibit_profiling_info = true;
  libff::inhibit_profiling_counters = true;
  const std::string r1cs_path(argv[2]), scalars_path(argv[3]), witness_path(argv[4]), dir(argv[5]);
  const unsigned long g1_multiple = strtoul(argv[6], nullptr, 0);
  const size_t expect_a = strtoul(argv[7], nullptr, 0), expect_b = strtoul(argv[8], nullptr, 0), expect_m = strtoul(argv[10], nullptr, 0),
               expect_untouched = strtoul(argv[11], nullptr, 0);
  const std::string expect_class(argv[9]);

  FILE* sf = open_or_die(scalars_path, "rb");
  const F t = read_fr<ppT>(sf), alpha = read_fr<ppT>(sf), beta = read_fr<ppT>(sf), delta = read_fr<ppT>(sf);
  fclose(sf);
  const P1 g1_gen = F(g1_multiple) * P1::one();
  REQUIRE(g1_multiple > 1 && !g1_gen.is_zero() && g1_gen != P1::one(), "the G1 generator must be a non-trivial multiple");

  const r1cs_constraint_system<F> cs_in = read_r1cs<ppT>(r1cs_path);
  const size_t ta = count_true(touched(cs_in, 0)), tb = count_true(touched(cs_in, 1));
  REQUIRE(ta == expect_a && tb == expect_b, "a touches %zu variables (expected %zu), b touches %zu (expected %zu)", ta, expect_a, tb, expect_b);
  r1cs_constraint_system<F> cs(cs_in);
  cs.swap_AB_if_beneficial();
  const bool swapped = tb > ta;
  {
    // the decision as the reference made it: a and b of the first constraint that tells them apart
    bool seen = false;
    for (size_t i = 0; i < cs.num_constraints() && !seen; ++i)
      if (!(cs_in.constraints[i].a == cs_in.constraints[i].b)) {
        seen = true;
        REQUIRE((cs.constraints[i].a == cs_in.constraints[i].b) == swapped, "swap_AB_if_beneficial decided otherwise than the counts say");
      }
  }
  size_t untouched = 0;
  {
    const std::vector<bool> a = touched(cs, 0), b = touched(cs, 1), c = touched(cs, 2);
    for (size_t i = cs.num_inputs() + 1; i <= cs.num_variables(); ++i) untouched += !a[i] && !b[i] && !c[i];
  }
  REQUIRE(untouched == expect_untouched, "%zu variables are touched by no matrix (expected %zu)", untouched, expect_untouched);

  // the witness satisfies the system the key is for
  const size_t m = cs.num_variables(), ni = cs.num_inputs(), nc = cs.num_constraints();
  FILE* wf = open_or_die(witness_path, "rb");
  REQUIRE(read_fr<ppT>(wf) == F::one(), "w[0] must be one");
  std::vector<F> full(m);
  for (auto& v : full) v = read_fr<ppT>(wf);
  const F r_elem = read_fr<ppT>(wf);
  fclose(wf);
  {
    r1cs_primary_input<F> prim(full.begin(), full.begin() + ni);
    r1cs_auxiliary_input<F> aux(full.begin() + ni, full.end());
    REQUIRE(cs.is_satisfied(prim, aux), "the witness does not satisfy the system");
  }

  // r1cs_gg_ppzksnark.tcc:220-281
  const F delta_inverse = delta.inverse();
  qap_instance_evaluation<F> qap = r1cs_to_qap_instance_map_with_evaluation(cs, t);
  const size_t dm = qap.domain->m;
  REQUIRE(std::string(class_of<F>(qap.domain.get())) == expect_class && dm == expect_m, "the domain is a %s of %zu elements (expected %s of %zu)",
          class_of<F>(qap.domain.get()), dm, expect_class.c_str(), expect_m);
  REQUIRE(!qap.Zt.is_zero(), "Z(t) = 0");
  size_t non_zero_At = 0, non_zero_Bt = 0;
  for (size_t i = 0; i <= m; ++i) { non_zero_At += !qap.At[i].is_zero(); non_zero_Bt += !qap.Bt[i].is_zero(); }
  std::vector<F> abc, Lt, Ht(qap.Ht.begin(), qap.Ht.end() - 2);
  for (size_t i = 0; i <= ni; ++i) abc.push_back(beta * qap.At[i] + alpha * qap.Bt[i] + qap.Ct[i]);
  for (size_t i = ni + 1; i <= m; ++i) Lt.push_back((beta * qap.At[i] + alpha * qap.Bt[i] + qap.Ct[i]) * delta_inverse);

  // :289-352
  const size_t bits = F::size_in_bits(), chunks = omp_get_max_threads();
  const size_t w1 = get_exp_window_size<P1>(non_zero_At + non_zero_Bt + m), w2 = get_exp_window_size<P2>(non_zero_Bt);
  const window_table<P1> table1 = get_window_table(bits, w1, g1_gen);
  const P2 g2_gen = P2::one();
  const window_table<P2> table2 = get_window_table(bits, w2, g2_gen);
  const P1 alpha_g1 = alpha * g1_gen, beta_g1 = beta * g1_gen, delta_g1 = delta * g1_gen;
  const P2 beta_g2 = beta * g2_gen, delta_g2 = delta * g2_gen;
  std::vector<P1> A_query = batch_exp(bits, w1, table1, qap.At);
  batch_to_special<P1>(A_query);
  knowledge_commitment_vector<P2, P1> B_query = kc_batch_exp(bits, w2, w1, table2, table1, F::one(), F::one(), qap.Bt, chunks);
  std::vector<P1> H_query = batch_exp_with_coeff(bits, w1, table1, qap.Zt * delta_inverse, Ht);
  batch_to_special<P1>(H_query);
  std::vector<P1> L_query = batch_exp(bits, w1, table1, Lt);
  batch_to_special<P1>(L_query);
  std::vector<P1> ABC_g1 = batch_exp(bits, w1, table1, abc);
  batch_to_special<P1>(ABC_g1);
  const GT<ppT> alpha_g1_beta_g2 = ppT::reduced_pairing(alpha_g1, beta_g2);
  REQUIRE(ABC_g1[0] == abc[0] * g1_gen, "ABC_0 through the table differs from the plain product");

  size_t identity_rows[4] = {0, 0, 0, 0};
  for (size_t i = 0; i <= m; ++i) {
    identity_rows[0] += A_query[i].is_zero();
    identity_rows[1] += B_query[i].h.is_zero();
    identity_rows[2] += B_query[i].g.is_zero();
  }
  for (auto& p : L_query) identity_rows[3] += p.is_zero();
  for (size_t k = 0; k < 4; ++k) REQUIRE(identity_rows[k] >= expect_untouched, "query %zu has %zu identity rows, fewer than the untouched variables", k, identity_rows[k]);

  {
    FILE* f = open_or_die(dir + "/randomness.bin", "wb");
    write_fr<ppT>(f, t); write_fr<ppT>(f, alpha); write_fr<ppT>(f, beta); write_fr<ppT>(f, delta);
    write_g1<ppT>(f, g1_gen);
    fclose(f);
  }
  write_r1cs<ppT>(dir + "/r1cs.bin", cs);
  {
    FILE* f = open_or_die(dir + "/params.bin", "wb");
    write_size_t(f, dm - 1); write_size_t(f, m);
    for (size_t i = 0; i <= m; ++i) write_g1<ppT>(f, A_query[i]);
    for (size_t i = 0; i <= m; ++i) write_g1<ppT>(f, B_query[i].h);
    for (size_t i = 0; i <= m; ++i) write_g2<ppT>(f, B_query[i].g);
    for (auto& p : L_query) write_g1<ppT>(f, p);
    for (auto& p : H_query) write_g1<ppT>(f, p);
    fclose(f);
  }
  {
    FILE* f = open_or_die(dir + "/keys.bin", "wb");
    write_g1<ppT>(f, alpha_g1); write_g1<ppT>(f, beta_g1); write_g2<ppT>(f, beta_g2); write_g1<ppT>(f, delta_g1); write_g2<ppT>(f, delta_g2);
    fclose(f);
  }
  {
    FILE* f = open_or_die(dir + "/vk_elements.bin", "wb");
    write_g1<ppT>(f, alpha_g1); write_g2<ppT>(f, beta_g2); write_g2<ppT>(f, delta_g2);
    for (auto& p : ABC_g1) write_g1<ppT>(f, p);
    fclose(f);
  }
  {
    P1 first = ABC_g1[0];
    std::vector<P1> rest(ABC_g1.begin() + 1, ABC_g1.end());
    accumulation_vector<P1> acc(std::move(first), std::move(rest));
    r1cs_gg_ppzksnark_verification_key<ppT> vk(alpha_g1_beta_g2, delta_g2, acc);
    std::ofstream out((dir + "/vk.txt").c_str());
    out << vk;
  }
  {
    // the evaluations of the (swapped) system on the assignment, generate_parameters.cpp:44-57, over the whole domain
    std::vector<F> ca(dm, F::zero()), cb(dm, F::zero()), cc(dm, F::zero());
    for (size_t i = 0; i <= ni; ++i) ca[i + nc] = i > 0 ? full[i - 1] : F::one();
    for (size_t i = 0; i < nc; ++i) {
      ca[i] += cs.constraints[i].a.evaluate(full);
      cb[i] += cs.constraints[i].b.evaluate(full);
      cc[i] += cs.constraints[i].c.evaluate(full);
    }
    FILE* f = open_or_die(dir + "/input.bin", "wb");
    write_fr<ppT>(f, F::one());
    for (auto& v : full) write_fr<ppT>(f, v);
    for (auto& v : ca) write_fr<ppT>(f, v);
    for (auto& v : cb) write_fr<ppT>(f, v);
    for (auto& v : cc) write_fr<ppT>(f, v);
    write_fr<ppT>(f, r_elem);
    fclose(f);
  }
  printf("keygen curve=%s num_inputs=%zu num_variables=%zu num_constraints=%zu m=%zu class=%s swapped=%d touched_a=%zu touched_b=%zu untouched=%zu "
         "non_zero_At=%zu non_zero_Bt=%zu g1_window=%zu g2_window=%zu g1_multiple=%lu\n",
         argv[1], ni, m, nc, dm, class_of<F>(qap.domain.get()), swapped ? 1 : 0, ta, tb, untouched, non_zero_At, non_zero_Bt, w1, w2, g1_multiple);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 12) {
    fprintf(stderr, "usage: %s <MNT4753|MNT6753> <r1cs_in.bin> <scalars.bin> <witness.bin> <out_dir> <g1_multiple> <touched_a> <touched_b> <class> <m> <untouched>\n", argv[0]);
    return 2;
  }
  const std::string curve(argv[1]);
  if (curve == "MNT4753") return mint<mnt4753_pp>(argv);
  if (curve == "MNT6753") return mint<mnt6753_pp>(argv);
  return 2;
}
