// Host check of the plan arithmetic of mnt753_batch_exp (csrc/batch_exp_plan.hpp): the very functions the walk kernel calls, compiled
// for the CPU.  Input: a file of scalars, 96 bytes each (the integer, 24 little-endian 32-bit words -- what fp_wire_to_integer hands
// the kernel).  For every width mnt753_fixed_base_create accepts and every scalar:
//   * every non-zero digit names a row inside the table (fb_row_of < fb_table_rows), in the window it was read from;
//   * the row formula read backwards (fb_multiple_of) names |d| 2^(jw), and those multiples, signed, sum to the scalar;
//   * |d| <= 2^(w-1), and the top window never produces a carry (the sum is exact in W windows).
// Stand-alone: g++ -std=c++17 tools/host_batch_exp_check.cpp; tests/test_batch_exp_cpu.py builds it plain and under ASan + UBSan.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../snark-challenge-prover-reference_amd/csrc/batch_exp_plan.hpp"

using namespace mnt753;

namespace {
constexpr int ACC_WORDS = 27;   // 864 bits: 22 * 35 = 770 bits of shift plus a 22-bit multiple, two's complement
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
  size_t digits_seen = 0, failures = 0;
  for (int w = FB_MIN_WINDOW_BITS; w <= FB_MAX_WINDOW_BITS; ++w) {
    const int W = fb_windows(w);
    const uint64_t rows = fb_table_rows(w);
    const uint32_t half = fb_rows_per_window(w);
    if (W * w < FB_SCALAR_BITS + 1 || (W - 1) * w >= FB_SCALAR_BITS + 1 || rows != (uint64_t)W * half || rows > 0xffffffffull) {
      printf("FAIL width %d: W = %d, rows = %llu\n", w, W, (unsigned long long)rows);
      ++failures;
      continue;
    }
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
        const FbRow r = fb_row_of(j, d, w);
        if ((uint64_t)r.row >= rows || r.negate != (d < 0)) { ok = false; break; }
        const FbMultiple m = fb_multiple_of(r.row, w);     // the row holds m.multiple 2^(m.window w) P
        if ((int)m.window != j || m.multiple != mag) { ok = false; break; }
        acc_add(acc, m.multiple, (int)m.window * w, r.negate);
      }
      for (int k = 0; k < ACC_WORDS && ok; ++k) ok = acc.w[k] == (k < 24 ? s[k] : 0u);
      if (!ok) {
        if (failures < 10) printf("FAIL width %d scalar %zu\n", w, i);
        ++failures;
      }
    }
  }
  // the default-width rule and the tile rounding, at their edges
  if (fb_default_window_bits(256, (uint64_t)256 << 20) != 15 || fb_table_rows(15) * 256 > ((uint64_t)256 << 20) || fb_table_rows(16) * 256 <= ((uint64_t)256 << 20)) {
    printf("FAIL default width of 256-byte rows\n");
    ++failures;
  }
  if (fb_round_tile(0) != FB_DEFAULT_TILE || fb_round_tile(1) != FB_INV_BATCH || fb_round_tile(FB_INV_BATCH + 1) != 2 * FB_INV_BATCH ||
      fb_round_tile(~(uint64_t)0 >> 1) != FB_MAX_TILE) {
    printf("FAIL tile rounding\n");
    ++failures;
  }
  if (failures) {
    printf("%zu FAILURES\n", failures);
    return 1;
  }
  printf("ALL OK: %zu scalars, widths %d .. %d, %zu non-zero digits\n", n, FB_MIN_WINDOW_BITS, FB_MAX_WINDOW_BITS, digits_seen);
  return 0;
}
