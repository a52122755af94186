// mint_qap.cpp -- mints the reference's values of the QAP at a point (TEST INFRASTRUCTURE; tools/mint_qap.sh compiles and runs it).
//
// OUR program, compiled against the REFERENCE's own libsnark / libff / libfqfft where they lie, with the flags and objects of
// oracle/build_ref.sh.  Nothing in it is this repository's arithmetic: the Lagrange coefficients, the vanishing polynomial and the
// instance map all come from MinaProtocol/snark-challenge-prover-reference code.
//
//   mint_qap <MNT4753|MNT6753> <out_dir> <t_file> <r1cs.bin>
//
// writes into <out_dir>, every element in the wire format (libsnark/serialization.hpp write_fr):
//   qap.bin          r1cs_to_qap_instance_map_with_evaluation(cs, t) on the constraint system of <r1cs.bin> (layout: oracle/ref_groth16.cpp):
//                    At | Bt | Ct (num_variables + 1 each) | Ht (m + 1) | Zt
//   lag_<m>.bin      for every domain size m of the curve's list, get_evaluation_domain<Fr>(m): seven records t | Z(t) | u[0 .. m), with
//                    u = evaluate_all_lagrange_polynomials(t), for t = the generic t of <t_file>, 0, and get_domain_element(idx),
//                    idx = 0, 1, m / 2 - 1, m / 2, m - 1
// and prints one line per file: what the reference chose (the class of the domain it built), for the index the script writes.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <libff/common/profiling.hpp>
#include <libff/algebra/curves/mnt753/mnt4753/mnt4753_pp.hpp>
#include <libff/algebra/curves/mnt753/mnt6753/mnt6753_pp.hpp>
#include <libfqfft/evaluation_domain/get_evaluation_domain.hpp>
#include <libfqfft/evaluation_domain/domains/basic_radix2_domain.hpp>
#include <libfqfft/evaluation_domain/domains/extended_radix2_domain.hpp>
#include <libfqfft/evaluation_domain/domains/step_radix2_domain.hpp>
#include <libsnark/serialization.hpp>
#include <libsnark/reductions/r1cs_to_qap/r1cs_to_qap.hpp>
#include <libsnark/relations/constraint_satisfaction_problems/r1cs/r1cs.hpp>

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

template <typename F>
const char* class_of(libfqfft::evaluation_domain<F>* d) {
  if (dynamic_cast<libfqfft::basic_radix2_domain<F>*>(d)) return "basic_radix2_domain";
  if (dynamic_cast<libfqfft::extended_radix2_domain<F>*>(d)) return "extended_radix2_domain";
  if (dynamic_cast<libfqfft::step_radix2_domain<F>*>(d)) return "step_radix2_domain";
  return "other";
}

template <typename ppT>
int mint(const std::string& name, const std::vector<size_t>& sizes, const std::string& dir, const std::string& t_path, const std::string& r1cs_path) {
  typedef Fr<ppT> F;
  ppT::init_public_params();
  libff::inhibit_profiling_info = true;
  libff::inhibit_profiling_counters = true;
  FILE* tf = open_or_die(t_path, "rb");
  const F t = read_fr<ppT>(tf);
  fclose(tf);
  {
    const r1cs_constraint_system<F> cs = read_r1cs<ppT>(r1cs_path);
    const qap_instance_evaluation<F> q = r1cs_to_qap_instance_map_with_evaluation(cs, t);
    FILE* f = open_or_die(dir + "/qap.bin", "wb");
    for (auto& v : q.At) write_fr<ppT>(f, v);
    for (auto& v : q.Bt) write_fr<ppT>(f, v);
    for (auto& v : q.Ct) write_fr<ppT>(f, v);
    for (auto& v : q.Ht) write_fr<ppT>(f, v);
    write_fr<ppT>(f, q.Zt);
    fclose(f);
    printf("qap %s num_inputs=%zu num_variables=%zu num_constraints=%zu m=%zu class=%s\n", name.c_str(), cs.num_inputs(), cs.num_variables(),
           cs.num_constraints(), q.domain->m, class_of<F>(q.domain.get()));
  }
  for (size_t m : sizes) {
    auto dom = libfqfft::get_evaluation_domain<F>(m);
    std::vector<std::pair<std::string, F>> ts;
    ts.emplace_back("generic", t);
    ts.emplace_back("zero", F::zero());
    const size_t idx[5] = {0, 1, dom->m / 2 - 1, dom->m / 2, dom->m - 1};
    for (size_t i : idx) ts.emplace_back("element:" + std::to_string(i), dom->get_domain_element(i));
    FILE* f = open_or_die(dir + "/lag_" + std::to_string(m) + ".bin", "wb");
    printf("lag %s min_size=%zu m=%zu class=%s t=", name.c_str(), m, dom->m, class_of<F>(dom.get()));
    for (size_t k = 0; k < ts.size(); ++k) {
      write_fr<ppT>(f, ts[k].second);
      write_fr<ppT>(f, dom->compute_vanishing_polynomial(ts[k].second));
      const std::vector<F> u = dom->evaluate_all_lagrange_polynomials(ts[k].second);
      if (u.size() != dom->m) { fprintf(stderr, "unexpected vector length\n"); return 1; }
      for (auto& v : u) write_fr<ppT>(f, v);
      printf("%s%s", k ? "," : "", ts[k].first.c_str());
    }
    printf("\n");
    fclose(f);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 5) { fprintf(stderr, "usage: %s <MNT4753|MNT6753> <out_dir> <t_file> <r1cs.bin>\n", argv[0]); return 2; }
  const std::string curve(argv[1]);
  const std::vector<size_t> common = {2, 8, 1024, 24, (1u << 10) + (1u << 7)};
  if (curve == "MNT4753") return mint<mnt4753_pp>(curve, common, argv[2], argv[3], argv[4]);
  if (curve == "MNT6753") {
    std::vector<size_t> s = common;
    s.push_back(40); s.push_back(200); s.push_back((size_t)1 << 16);
    return mint<mnt6753_pp>(curve, s, argv[2], argv[3], argv[4]);
  }
  return 2;
}
