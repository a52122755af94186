// Host build of the plan's index-width guard (csrc/msm_limits.hpp), driven by tests/test_table_rows_cpu.py:
//   row_limits_check ROW_QUADS ROWS...   prints one line per ROWS: "<rows> <1 if the level-1 table offsets fit 32 bits, else 0>"
#include <cstdio>
#include <cstdlib>
#include "../../snark-challenge-prover-reference_amd/csrc/msm_limits.hpp"

static_assert(mnt753::pair_row_offsets_fit(((uint64_t)1 << 28) - 1, 16) && !mnt753::pair_row_offsets_fit((uint64_t)1 << 28, 16), "256-byte rows: 2^28 rows is the first table that does not fit");

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const uint32_t row_quads = (uint32_t)strtoul(argv[1], nullptr, 10);
  for (int i = 2; i < argc; ++i) {
    const uint64_t rows = strtoull(argv[i], nullptr, 10);
    printf("%llu %d\n", (unsigned long long)rows, mnt753::pair_row_offsets_fit(rows, row_quads) ? 1 : 0);
  }
  return 0;
}
