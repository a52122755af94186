// Host check of the plan arithmetic of a verification key's input tables (csrc/vk_input_plan.hpp): the very functions the walk
// kernel and the host call, compiled for the CPU.  Input: a file of scalars, 96 bytes each (the integer, 24 little-endian 32-bit
// words -- what k_inputs_to_integer hands the walk).  For every width mnt753_vk_prepare_inputs accepts (2 .. 16), every number of
// inputs k in {1, 2, 1000} and every scalar, taken as the scalar of the first, of a middle and of the last base:
//   * every non-zero digit names a row inside ITS OWN base's part of the long table (vki_first_row(p) <= row < vki_first_row(p + 1)),
//     in the window it was read from;
//   * the multiples |d| 2^(jw) those rows hold, signed, sum to the scalar (for a scalar below 2^753; any 768 bits stay in range);
// and, without scalars: the table bytes and the default width at their edges, and the slices of a proof -- they tile [0, k) in order,
// only the last one is ragged, and a chunk gets the lanes the host promises.
// Stand-alone: g++ -std=c++17 tools/host_vk_inputs_check.cpp; tests/test_vk_inputs_cpu.py builds it plain and under ASan + UBSan.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../snark-challenge-prover-reference_amd/csrc/vk_input_plan.hpp"

using namespace mnt753;

namespace {
constexpr int ACC_WORDS = 27;
struct Acc {
  uint32_t w[ACC_WORDS];
};
// acc += sign * (mult << shift)
void acc_add(Acc& a, uint32_t mult, int shift, bool negative) {
  uint32_t term[ACC_WORDS];
  memset(term, 0, sizeof(term));
  const int wi = shift >> 5, sh = shift & 31;
  const uint64_t v = (uint64_t)mult << sh;
  term[wi] = (uint32_t)v;
  term[wi + 1] = (uint32_t)(v >> 32);
  uint64_t carry = negative ? 1 : 0;
  for (int i = 0; i < ACC_WORDS; ++i) {
    const uint64_t t = (uint64_t)a.w[i] + (negative ? ~term[i] : term[i]) + carry;
    a.w[i] = (uint32_t)t;
    carry = t >> 32;
  }
}
size_t failures = 0;
void fail(const char* what, long a = 0, long b = 0, long c = 0) {
  if (failures < 10) printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  ++failures;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <scalars.bin>\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  std::vector<uint32_t> words;
  uint32_t buf[24];
  while (fread(buf, sizeof(buf), 1, f) == 1) words.insert(words.end(), buf, buf + 24);
  fclose(f);
  const size_t n = words.size() / 24;
  if (n == 0) {
    fprintf(stderr, "no scalars\n");
    return 2;
  }
  size_t digits_seen = 0;
  const uint32_t ks[3] = {1, 2, 1000};
  for (int w = VKI_MIN_WINDOW_BITS; w <= VKI_MAX_WINDOW_BITS; ++w) {
    const int W = fb_windows(w);
    const uint32_t half = fb_rows_per_window(w);
    for (uint32_t k : ks) {
      const uint64_t points = (uint64_t)k + 1;
      const uint64_t rows = vki_table_rows(points, w);
      if (rows != points * (uint64_t)W * half || vki_table_bytes(points, w) != rows * VKI_ROW_BYTES) { fail("table size", w, k); continue; }
      const uint32_t bases[3] = {0, k / 2, k};
      for (uint32_t p : bases) {
        const uint64_t lo = vki_first_row(p, w), hi = vki_first_row(p + 1, w);
        if (hi - lo != fb_table_rows(w) || hi > rows) { fail("base range", w, k, p); continue; }
        for (size_t i = 0; i < n; ++i) {
          const uint32_t* s = &words[24 * i];
          Acc acc;
          memset(&acc, 0, sizeof(acc));
          bool ok = true;
          for (int j = 0; j < W && ok; ++j) {
            const int32_t d = fb_digit(s, 1, j, w);
            const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
            if (mag > half) ok = false;
            if (d == 0 || !ok) continue;
            ++digits_seen;
            const FbRow r = vki_row_of(p, j, d, w);
            if ((uint64_t)r.row < lo || (uint64_t)r.row >= hi || r.negate != (d < 0)) { ok = false; break; }
            const FbMultiple m = fb_multiple_of(r.row - (uint32_t)lo, w);   // inside the base: the row holds m.multiple 2^(m.window w) ABC[p]
            if ((int)m.window != j || m.multiple != mag) { ok = false; break; }
            acc_add(acc, m.multiple, (int)m.window * w, r.negate);
          }
          // (words of 753 bits and more -- an input that was not below r is still walked -- only have to stay inside the tables)
          const bool is_scalar = (s[23] >> 17) == 0;
          for (int q = 0; q < ACC_WORDS && ok && is_scalar; ++q) ok = acc.w[q] == (q < 24 ? s[q] : 0u);
          if (!ok) fail("scalar", w, p, (long)i);
        }
      }
    }
  }
  // the default width under a cap, at its edges
  for (uint64_t points : {2ull, 3ull, 34ull, 258ull, 1001ull, 1ull << 20}) {
    const int w = vki_default_window_bits(points, VKI_DEFAULT_TABLE_BYTES);
    if (w) {
      if (vki_table_bytes(points, w) > VKI_DEFAULT_TABLE_BYTES) fail("default width does not fit", (long)points, w);
      if (w < VKI_MAX_WINDOW_BITS && vki_table_rows(points, w + 1) && vki_table_bytes(points, w + 1) <= VKI_DEFAULT_TABLE_BYTES) fail("a wider table fits", (long)points, w);
    } else if (vki_table_bytes(points, VKI_MIN_WINDOW_BITS) <= VKI_DEFAULT_TABLE_BYTES) {
      fail("width 2 fits but none was chosen", (long)points);
    }
  }
  if (vki_default_window_bits(2, VKI_DEFAULT_TABLE_BYTES) != 14 || vki_default_window_bits(2, 1) != 0 ||
      vki_default_window_bits(2, vki_table_bytes(2, 2)) != 2 || vki_default_window_bits(2, vki_table_bytes(2, 2) - 1) != 0)
    fail("default width of two points");
  if (vki_table_rows((uint64_t)1 << 32, 2) != 0) fail("row index overflow not reported");
  // the slices of a proof
  for (uint32_t k : {1u, 2u, 3u, 33u, 257u, 1000u, 1u << 20}) {
    for (uint32_t ipl : {1u, 2u, 3u, 16u, k > 1 ? k - 1 : 1u, k, k + 5}) {
      const uint32_t S = vki_slices(k, ipl);
      // every slice of a short list; the ends and the middle of a long one
      std::vector<uint32_t> which;
      if (S <= 4096) for (uint32_t s = 0; s < S; ++s) which.push_back(s);
      else which = {0, 1, S / 2, S - 2, S - 1};
      uint32_t at = 0;
      for (uint32_t s : which) {
        const VkiSlice sl = vki_slice(s, k, ipl);
        if (S <= 4096 && sl.first != at) fail("slices do not tile", k, ipl, s);
        if (sl.first != (uint64_t)s * ipl || sl.end <= sl.first || sl.end > k || (s + 1 < S && sl.end - sl.first != ipl)) fail("slice", k, ipl, s);
        if (s + 1 == S && sl.end != k) fail("last slice", k, ipl, s);
        at = sl.end;
      }
      if (vki_workspace_per_proof(k, ipl) != (uint64_t)VKI_PARTIAL_BYTES * (S + 1) + 112) fail("workspace", k, ipl);
    }
    for (uint64_t np : {1ull, 2ull, 65ull, 257ull, 32768ull, 65536ull, 131072ull}) {
      const uint32_t ipl = vki_inputs_per_lane(np, k);
      const uint64_t lanes = np * vki_slices(k, ipl);
      if (ipl < 1 || ipl > k) fail("inputs per lane", k, (long)np, ipl);
      if (np == 1 && k <= VKI_TARGET_LANES && ipl != 1) fail("one proof: one input per lane", k);
      if (np >= VKI_TARGET_LANES && ipl != k) fail("a full chunk: one lane per proof", k, (long)np);
      if (ipl > 1 && np * vki_slices(k, ipl - 1) <= VKI_TARGET_LANES) fail("fewer lanes than the chip takes", k, (long)np, ipl);
      (void)lanes;
    }
  }
  if (failures) {
    printf("%zu FAILURES\n", failures);
    return 1;
  }
  printf("ALL OK: %zu scalars, widths %d .. %d, %zu non-zero digits\n", n, VKI_MIN_WINDOW_BITS, VKI_MAX_WINDOW_BITS, digits_seen);
  return 0;
}
