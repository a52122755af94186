// The host-side plan of mnt753_groth16_verify_folded_locate (csrc/mnt753_fold_locate.hip): the proofs of a
// segment, the chunk of a call under the key's workspace cap, and the runs of adjacent rejected segments that the per-proof verifier
// rechecks.  Plain C++, no HIP: tools/host_fold_locate_plan_check.cpp exercises it stand-alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mnt753 {

// proofs [first, first + count)
struct FoldRange {
  size_t first, count;
};

// segments of g proofs that n proofs fill, the last one possibly short
inline size_t fold_segments(size_t n, size_t g) { return (n + g - 1) / g; }

// the proofs of segment s < fold_segments(n, g)
inline FoldRange fold_segment_range(size_t s, size_t n, size_t g) {
  const size_t first = s * g;
  return FoldRange{first, n - first < g ? n - first : g};
}

// Proofs per chunk of a call over n >= 1 proofs: a whole number of segments, at least one, at most max_chunk rounded down to whole
// segments, and no more segments than n fills.  cap: the bytes a call may allocate (0: none), of which a proof takes per_proof and a
// segment per_segment on top; a cap below one segment's need still runs one segment.
inline size_t fold_chunk_proofs(size_t n, size_t g, size_t per_proof, size_t per_segment, size_t cap, size_t max_chunk) {
  size_t segs = fold_segments(n, g);
  const size_t most = max_chunk / g ? max_chunk / g : 1;
  if (segs > most) segs = most;
  if (cap) {
    const size_t fits = cap / (g * per_proof + per_segment);
    if (fits < segs) segs = fits ? fits : 1;
  }
  return segs * g;
}

// The runs of adjacent segments with accepted[s] == 0, as proofs: in rising order, disjoint, no two of them adjacent.  accepted: one
// byte per segment of the n proofs.
inline std::vector<FoldRange> fold_rejected_runs(const std::vector<uint8_t>& accepted, size_t n, size_t g) {
  std::vector<FoldRange> runs;
  const size_t segs = fold_segments(n, g);
  for (size_t s = 0; s < segs && s < accepted.size(); ++s) {
    if (accepted[s]) continue;
    const FoldRange r = fold_segment_range(s, n, g);
    if (!runs.empty() && runs.back().first + runs.back().count == r.first) runs.back().count += r.count;
    else runs.push_back(r);
  }
  return runs;
}

}  // namespace mnt753
