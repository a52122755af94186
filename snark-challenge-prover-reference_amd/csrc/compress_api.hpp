// Decompression for the other translation units of the library (mnt753_pairing.hip: mnt753_groth16_verify_compressed); the kernels and
// their instantiations live in mnt753_compress.hip alone.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace mnt753 {
// Enqueues k_decompress (compress_kernels.hip.h) for n <= 2^24 points of (curve, group) on st.  Device pointers; strides in 32-bit
// words (flags: bytes).  stand_x: the x coordinate of a point of the group in wire form (the generator's), which a point that is not
// decompressed runs the arithmetic on.  rec: a device record of decompress_report_bytes() bytes, {n_bad, key = index << 3 | reason},
// set up by decompress_report_init; index = base + position.  Returns 0 or a negative MNT753_E* code.
int decompress_enqueue(int curve, int group, const uint32_t* x, size_t x_stride, const uint8_t* flags, size_t f_stride, const uint32_t* stand_x,
                       uint32_t* out, size_t out_stride, size_t n, unsigned long long base, void* rec, hipStream_t st);
size_t decompress_report_bytes();
int decompress_report_init(void* rec, hipStream_t st);
}  // namespace mnt753
