// B::pairing and B::verify (include/prover_hip_functions.hpp) from the caller's side; run by tests/test_pairing_gpu.py.
//   pairing_wrapper_test MNT4753|MNT6753 <keys.bin> <vk.txt> <vk_elements.bin> <input.bin> <proof>
// e(alpha_g1, beta_g2) of keys.bin (alpha_g1 | beta_g1 | beta_g2 | ..) must be the GT element at the head of vk.txt, twice in one batch;
// the proof must verify against vk_elements.bin with the public inputs behind the leading 1 of input.bin, and must be rejected with
// its C replaced by its A.  Prints "wrapper pairing OK" and exits 0, or says what differs and exits 1.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/mnt753_hip.h"
#include "../../include/prover_hip_functions.hpp"

static std::vector<uint64_t> words_of(const char* path, size_t at_most = ~(size_t)0) {
  std::vector<uint64_t> out;
  FILE* f = fopen(path, "rb");
  if (!f) return out;
  uint64_t w;
  while (out.size() < at_most && fread(&w, 8, 1, f) == 1) out.push_back(w);
  fclose(f);
  return out;
}

template <class B, int CURVE> int run(char** argv) {
  const size_t w2 = mnt753_affine_words(CURVE, MNT753_G2), wt = mnt753_gt_words(CURVE);
  const std::vector<uint64_t> keys = words_of(argv[2]), head = words_of(argv[3], wt), el = words_of(argv[4]), proof = words_of(argv[6]);
  if (keys.size() < 48 + w2 || head.size() != wt || el.size() < 48 + 2 * w2 || proof.size() != 48 + w2) { fprintf(stderr, "bad input files\n"); return 1; }
  const size_t num_inputs = (el.size() - 24 - 2 * w2) / 24 - 1;
  const std::vector<uint64_t> input = words_of(argv[5], 12 * (num_inputs + 1));
  if (mnt753_init(0) != 0) { fprintf(stderr, "%s\n", mnt753_last_error()); return 1; }
  std::vector<uint64_t> g1(keys.begin(), keys.begin() + 24), g2(keys.begin() + 48, keys.begin() + 48 + w2);
  g1.insert(g1.end(), keys.begin(), keys.begin() + 24);
  g2.insert(g2.end(), keys.begin() + 48, keys.begin() + 48 + w2);
  const std::vector<uint64_t> gt = B::pairing(g1.data(), g2.data(), 2);
  if (gt.size() != 2 * wt || memcmp(gt.data(), head.data(), 8 * wt) != 0 || memcmp(gt.data() + wt, head.data(), 8 * wt) != 0) { fprintf(stderr, "B::pairing differs from vk.txt\n"); return 1; }
  std::vector<uint64_t> proofs(proof), inputs(input.begin() + 12, input.end());
  proofs.insert(proofs.end(), proof.begin(), proof.end());
  memcpy(proofs.data() + (48 + w2) + 24 + w2, proof.data(), 8 * 24);   // the second proof: C := A
  inputs.insert(inputs.end(), input.begin() + 12, input.end());
  const std::vector<uint8_t> v = B::verify(el.data(), num_inputs, proofs.data(), inputs.data(), 2);
  if (v.size() != 2 || v[0] != 0 || v[1] != 2) { fprintf(stderr, "B::verify: verdicts %d %d, expected 0 2\n", v.size() > 0 ? v[0] : -1, v.size() > 1 ? v[1] : -1); return 1; }
  printf("wrapper pairing OK\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 7) { fprintf(stderr, "usage: %s MNT4753|MNT6753 <keys.bin> <vk.txt> <vk_elements.bin> <input.bin> <proof>\n", argv[0]); return 2; }
  try {
    if (!strcmp(argv[1], "MNT4753")) return run<mnt4753_hip, 0>(argv);
    if (!strcmp(argv[1], "MNT6753")) return run<mnt6753_hip, 1>(argv);
  } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 1; }
  return 2;
}
