// GPU box: B::check_H from the caller's side (include/prover_hip_functions.hpp).
//   h_check_wrapper_test MNT4753|MNT6753 <params> <input>
// With B::check_H(true), B::compute_H_fused takes A(t), B(t), C(t) before its transforms and compares them with Z(t) H(t) behind
// them, at a random t, on one device or with ca / cb / cc on three (MNT753_GPUS).  Prints "ok" (exit code 0), or "refused: <message>"
// where the identity fails (exit code 3); anything else is exit code 1.  tests/test_hcheck_gpu.py runs it.
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "../../include/mnt753_hip.h"
#include "../../include/prover_hip_functions.hpp"

template <typename B>
static int run(const char* params_path, const char* input_path) {
  B::init_public_params();
  B::check_H(true);
  auto params = B::read_params(params_path);
  auto input = B::read_input(input_path, params);
  auto ca = B::input_ca(input), cb = B::input_cb(input), cc = B::input_cc(input);
  auto domain = B::get_evaluation_domain(B::params_d(params) + 1);
  int rc = 0;
  try {
    auto h = B::compute_H_fused(domain, ca, cb, cc);
    B::delete_vector_Fr(h);
    printf("ok\n");
  } catch (const typename B::h_check_failed& e) {
    printf("refused: %s\n", e.what());
    rc = 3;
  }
  B::delete_evaluation_domain(domain);
  B::delete_vector_Fr(ca); B::delete_vector_Fr(cb); B::delete_vector_Fr(cc);
  B::delete_groth16_input(input);
  B::delete_groth16_params(params);
  return rc;
}

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s MNT4753|MNT6753 <params> <input>\n", argv[0]); return 2; }
  try {
    if (!strcmp(argv[1], "MNT4753")) return run<mnt4753_hip>(argv[2], argv[3]);
    if (!strcmp(argv[1], "MNT6753")) return run<mnt6753_hip>(argv[2], argv[3]);
    fprintf(stderr, "unknown curve %s\n", argv[1]);
    return 2;
  } catch (const std::exception& e) {
    fprintf(stderr, "h_check_wrapper_test: %s\n", e.what());
    return 1;
  }
}
