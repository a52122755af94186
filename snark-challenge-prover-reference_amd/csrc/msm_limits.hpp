// Index-width limits of an MSM plan that need no device: plain arithmetic, also compiled for the host by the CPU tests.
#pragma once
#include <stdint.h>

namespace mnt753 {
// The first batched-affine level of a base field keeps the table offsets of its LDS-DMA pieces in 32-bit registers, in uint4 units:
// piece q of row r of a table of `rows` rows, `row_quads` uint4s from row to row, sits at r * row_quads + q with q < row_quads.  All
// of them fit exactly while rows * row_quads stays below 2^32 (256-byte rows, 16 uint4s: a table below 64 GiB, 2^28 rows).
// (rows * row_quads < 2^32, written without the product: it must not wrap for a row count nobody can allocate)
constexpr bool pair_row_offsets_fit(uint64_t rows, uint32_t row_quads) { return row_quads != 0 && rows <= 0xffffffffull / row_quads; }
}  // namespace mnt753
