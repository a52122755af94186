// Plan arithmetic of the fixed-base batch scalar multiplication (mnt753_batch_exp) that needs no device: the windows of a width, the
// signed digit of a window, and the table row a digit names.  Plain integer code, __host__ __device__ where a HIP compiler reads it:
// the walk kernel (batch_exp_kernels.hip.h) and the host check (tools/host_batch_exp_check.cpp, compiled by the CPU tests) share
// exactly these functions.
//
// libff's get_window_table / windowed_exp (depends/libff/libff/algebra/scalar_multiplication/multiexp.tcc:547-612) keep, per window
// j of `window` bits, the multiples 0 .. 2^window - 1 of 2^(j window) P and add one row per window.  Here the digits are signed
// (Booth, the recoding of the MSM's k_scalar_digits): |d| <= 2^(w-1), so a window keeps the multiples 1 .. 2^(w-1) -- half the rows --
// and a negative digit adds the row with y negated.  The sum over the windows is the same group element s P.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MNT753_PLAN_HD __host__ __device__ inline
#else
#define MNT753_PLAN_HD inline
#endif

namespace mnt753 {

constexpr int FB_SCALAR_BITS = 753;       // both scalar fields: r < 2^753
constexpr int FB_MIN_WINDOW_BITS = 2;
constexpr int FB_MAX_WINDOW_BITS = 22;    // 35 windows of 2^21 rows: 18.8 GB of 256-byte rows; the bit reader takes up to 25 bits

// W = ceil(754 / w): one bit more than a scalar has, so that the top window's highest bit is never set and its digit takes the carry
// of the window below without producing one itself
MNT753_PLAN_HD int fb_windows(int w) { return (FB_SCALAR_BITS + 1 + w - 1) / w; }
// rows per window: the multiples 1 .. 2^(w-1)
MNT753_PLAN_HD uint32_t fb_rows_per_window(int w) { return 1u << (w - 1); }
MNT753_PLAN_HD uint64_t fb_table_rows(int w) { return (uint64_t)fb_windows(w) * fb_rows_per_window(w); }

// bits [pos, pos + n) of the integer whose 32-bit word k is s[k * stride], k < 24; n <= 25; bits from 768 on are zero
MNT753_PLAN_HD uint32_t fb_bits(const uint32_t* s, int stride, int pos, int n) {
  if (pos >= 768) return 0;
  const int wi = pos >> 5, sh = pos & 31;
  const uint64_t lo = s[wi * stride];
  const uint64_t hi = (wi + 1 < 24) ? s[(wi + 1) * stride] : 0u;
  return (uint32_t)((lo | (hi << 32)) >> sh) & ((1u << n) - 1u);
}
// digit j of the integer s at width w:  d_j = s[jw .. jw+w) + s[jw-1] - 2^w s[jw+w-1],  |d_j| <= 2^(w-1),  sum_j d_j 2^(jw) = s
MNT753_PLAN_HD int32_t fb_digit(const uint32_t* s, int stride, int j, int w) {
  const int pos = j * w;
  const uint32_t win = fb_bits(s, stride, pos, w);
  const uint32_t below = pos ? fb_bits(s, stride, pos - 1, 1) : 0u;
  const uint32_t top = (win >> (w - 1)) & 1u;
  return (int32_t)win + (int32_t)below - (int32_t)(top << w);
}
// the row of digit d != 0 of window j, and whether it is taken with y negated; rows of a window are consecutive, windows follow
// each other: row(j, d) = j 2^(w-1) + |d| - 1 holds |d| 2^(jw) P
struct FbRow {
  uint32_t row;
  bool negate;
};
MNT753_PLAN_HD FbRow fb_row_of(int j, int32_t d, int w) {
  const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
  return FbRow{(uint32_t)j * fb_rows_per_window(w) + mag - 1u, d < 0};
}
// the inverse, for the table builder and the checks: row -> (window j, multiple m): the row holds m 2^(jw) P
struct FbMultiple {
  uint32_t window, multiple;
};
MNT753_PLAN_HD FbMultiple fb_multiple_of(uint32_t row, int w) {
  return FbMultiple{row >> (w - 1), (row & (fb_rows_per_window(w) - 1u)) + 1u};
}

// ---- the plan of an object ---------------------------------------------------------------------------------------------------
// results per field inversion of the normalisation (Montgomery's simultaneous inversion over runs of B consecutive results: 3
// products per result for the trick against one inversion of ~300 products' time per run)
constexpr uint32_t FB_INV_BATCH = 16;
// scalars per pass when the caller leaves the tile to the library: two rounds of the 65536 lanes a 256-CU part runs at one wave
// per SIMD
constexpr uint64_t FB_DEFAULT_TILE = (uint64_t)1 << 17;
constexpr uint64_t FB_MAX_TILE = (uint64_t)1 << 24;
MNT753_PLAN_HD uint64_t fb_round_tile(uint64_t tile) {
  if (tile == 0) tile = FB_DEFAULT_TILE;
  if (tile > FB_MAX_TILE) tile = FB_MAX_TILE;
  return (tile + FB_INV_BATCH - 1) / FB_INV_BATCH * FB_INV_BATCH;
}
// The width the library picks: the widest table that stays within `budget_bytes` (the 256 MiB Infinity Cache of the MI355X: the
// walk gathers one row per window and scalar), rows of row_bytes.
MNT753_PLAN_HD int fb_default_window_bits(uint32_t row_bytes, uint64_t budget_bytes) {
  int best = FB_MIN_WINDOW_BITS;
  for (int w = FB_MIN_WINDOW_BITS; w <= FB_MAX_WINDOW_BITS; ++w)
    if (fb_table_rows(w) * row_bytes <= budget_bytes) best = w;
  return best;
}

}  // namespace mnt753
