// The host-side plan of mnt753_groth16_verify_folded_locate (csrc/fold_locate_plan.hpp) on its own: segment ranges, chunk rounding
// under a workspace cap, and the merge of rejected segments into rechecked runs.  A stand-alone program without HIP:
//   g++ -std=c++17 -o host_fold_locate_plan_check tools/host_fold_locate_plan_check.cpp && ./host_fold_locate_plan_check
// (tests/test_fold_locate_cpu.py builds it plainly and under -fsanitize=address,undefined and runs both).  Prints ALL OK, exit 0.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../snark-challenge-prover-reference_amd/csrc/fold_locate_plan.hpp"

using namespace mnt753;

static int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

// every proof lies in exactly one segment, the segments are in order and only the last one is short
static void check_segments(size_t n, size_t g) {
  const size_t segs = fold_segments(n, g);
  EXPECT(segs == (n + g - 1) / g);
  size_t next = 0;
  for (size_t s = 0; s < segs; ++s) {
    const FoldRange r = fold_segment_range(s, n, g);
    EXPECT(r.first == next && r.first == s * g);
    EXPECT(r.count >= 1 && r.count <= g);
    EXPECT(s + 1 == segs || r.count == g);
    next = r.first + r.count;
  }
  EXPECT(next == n);
}

static void check_runs(const std::vector<uint8_t>& accepted, size_t n, size_t g, const std::vector<FoldRange>& want) {
  const std::vector<FoldRange> got = fold_rejected_runs(accepted, n, g);
  EXPECT(got.size() == want.size());
  for (size_t k = 0; k < got.size() && k < want.size(); ++k) EXPECT(got[k].first == want[k].first && got[k].count == want[k].count);
  // whatever the pattern: the runs cover exactly the proofs of the rejected segments, rising, never adjacent
  std::vector<uint8_t> covered(n, 0);
  size_t last_end = 0;
  for (size_t k = 0; k < got.size(); ++k) {
    EXPECT(got[k].count >= 1 && got[k].first + got[k].count <= n);
    EXPECT(k == 0 || got[k].first > last_end);
    last_end = got[k].first + got[k].count;
    for (size_t i = got[k].first; i < last_end && i < n; ++i) covered[i] = 1;
  }
  for (size_t i = 0; i < n; ++i) EXPECT(covered[i] == (accepted[i / g] ? 0 : 1));
}

int main() {
  for (size_t g : {(size_t)128, (size_t)84}) {
    for (size_t n : {(size_t)1, g - 1, g, g + 1, 2 * g + 1}) check_segments(n, g);
    EXPECT(fold_segments(1, g) == 1 && fold_segments(g, g) == 1 && fold_segments(g + 1, g) == 2 && fold_segments(2 * g + 1, g) == 3);
    EXPECT(fold_segment_range(2, 2 * g + 1, g).first == 2 * g && fold_segment_range(2, 2 * g + 1, g).count == 1);
    EXPECT(fold_segment_range(0, g - 1, g).count == g - 1);

    // chunks: per proof 1000 bytes and per segment 5000, so one segment needs `one` bytes
    const size_t pp = 1000, ps = 5000, one = g * pp + ps, n = 5 * g + 3, most = (size_t)1 << 16;
    EXPECT(fold_chunk_proofs(n, g, pp, ps, 0, most) == 6 * g);                  // no cap: all six segments
    EXPECT(fold_chunk_proofs(n, g, pp, ps, one - 1, most) == g);                // less than one segment: still one
    EXPECT(fold_chunk_proofs(n, g, pp, ps, 1, most) == g);
    EXPECT(fold_chunk_proofs(n, g, pp, ps, one, most) == g);                    // exactly one
    EXPECT(fold_chunk_proofs(n, g, pp, ps, one + one / 2, most) == g);          // one and a half: one
    EXPECT(fold_chunk_proofs(n, g, pp, ps, 2 * one, most) == 2 * g);
    EXPECT(fold_chunk_proofs(n, g, pp, ps, 3 * one - 1, most) == 2 * g);
    EXPECT(fold_chunk_proofs(n, g, pp, ps, 100 * one, most) == 6 * g);          // more than n needs: n's segments
    EXPECT(fold_chunk_proofs(1, g, pp, ps, 0, most) == g && fold_chunk_proofs(g + 1, g, pp, ps, 0, most) == 2 * g);
    // the ceiling of a launch, rounded down to whole segments
    EXPECT(fold_chunk_proofs((size_t)1 << 20, g, pp, ps, 0, most) == (most / g) * g);
    EXPECT(fold_chunk_proofs((size_t)1 << 20, g, pp, ps, 0, most) % g == 0 && fold_chunk_proofs((size_t)1 << 20, g, pp, ps, 0, most) <= most);
    EXPECT(fold_chunk_proofs(n, g, pp, ps, 0, 1) == g);                         // (a ceiling below one segment: one)
    // every chunk of a walk over n starts on a segment boundary
    for (size_t cap : {(size_t)0, one, 2 * one, 4 * one}) {
      const size_t chunk = fold_chunk_proofs(n, g, pp, ps, cap, most);
      EXPECT(chunk >= g && chunk % g == 0);
      for (size_t first = 0; first < n; first += chunk) EXPECT(first % g == 0);
    }

    // runs, five segments with a short last one
    const size_t m = 4 * g + 5;
    check_runs({1, 1, 1, 1, 1}, m, g, {});
    check_runs({0, 0, 0, 0, 0}, m, g, {{0, m}});
    check_runs({0, 1, 0, 1, 0}, m, g, {{0, g}, {2 * g, g}, {4 * g, 5}});
    check_runs({1, 0, 1, 0, 1}, m, g, {{g, g}, {3 * g, g}});
    check_runs({0, 1, 1, 1, 1}, m, g, {{0, g}});
    check_runs({1, 1, 1, 1, 0}, m, g, {{4 * g, 5}});
    check_runs({1, 0, 0, 1, 0}, m, g, {{g, 2 * g}, {4 * g, 5}});
    check_runs({0}, 1, g, {{0, 1}});
    check_runs({1}, g, g, {});
  }
  if (failures) {
    printf("%d check(s) failed\n", failures);
    return 1;
  }
  printf("ALL OK\n");
  return 0;
}
