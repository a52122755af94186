// Host twin of the raw-limb field hook (mnt753_test_field_raw, include/mnt753_hip_test.h): the same dispatch
// (csrc/field_raw_ops.hip.h) compiled by g++ into a shared object, driven by tests/test_field_raw_cpu.py against the exact reference
// of tests/field_raw_ref.py, and by tests/test_field_raw_gpu.py as the bit-exact twin of the device build.
//   g++ -O2 -std=c++17 -shared -fPIC -o libfield_raw_host.so tools/host_tests/field_raw_host.cpp
#include <stddef.h>
#include <stdint.h>

#include "../../snark-challenge-prover-reference_amd/csrc/field_raw_ops.hip.h"

using namespace mnt753;

extern "C" int mnt753_test_field_raw(int mod, int op, const uint32_t* in, size_t n, uint32_t k, uint32_t* out) {
  if (mod < 0 || mod > 1 || op < 0 || op >= FR_NUM_OPS || (n && (!in || !out))) return -1;
  for (size_t i = 0; i < n; ++i) {
    if (mod == MOD_A) field_raw_op<MOD_A>(op, in + FR_IN_WORDS * i, k, out + FR_OUT_WORDS * i);
    else field_raw_op<MOD_B>(op, in + FR_IN_WORDS * i, k, out + FR_OUT_WORDS * i);
  }
  return 0;
}
