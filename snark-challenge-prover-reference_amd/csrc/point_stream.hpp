// libff's stream records of the packed compressed form (include/mnt753_hip.h: mnt753_points_to_stream / mnt753_points_from_stream):
// host code only, bytes in and bytes out, no arithmetic -- shared by the product (mnt753_compress.hip) and the stub of the C ABI the
// sanitizer builds link (tools/stub_abi), so that main_hip's compress-proof / decompress-proof run the same codec under both.
// A record, under BINARY_OUTPUT + MONTGOMERY_OUTPUT with an empty OUTPUT_SEPARATOR: '0' / '1' (is the identity), the bytes of x,
// '0' / '1' (the parity).  xb: bytes of x (96, 192 or 288).  Return 0, or 1 .. 3 for the three ways an input can be refused.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace mnt753 {
enum { STREAM_OK = 0, STREAM_BAD_FLAG = 1, STREAM_SHORT = 2 };

inline int stream_write(size_t xb, const uint64_t* x, const uint8_t* flags, size_t n, uint8_t* buf) {
  const size_t rec = xb + 2;
  for (size_t i = 0; i < n; ++i) {
    if (flags[i] & 0xfcu) return STREAM_BAD_FLAG;
    uint8_t* o = buf + i * rec;
    if (flags[i] & 2u) {                           // libff's zero() after to_affine_coordinates(): X = 0, Y = 1
      o[0] = '1';
      memset(o + 1, 0, xb);
      o[1 + xb] = '1';
    } else {
      o[0] = '0';
      memcpy(o + 1, reinterpret_cast<const uint8_t*>(x) + i * xb, xb);
      o[1 + xb] = (flags[i] & 1u) ? '1' : '0';
    }
  }
  return STREAM_OK;
}

inline int stream_read(size_t xb, const uint8_t* buf, size_t len, size_t n, uint64_t* x, uint8_t* flags) {
  const size_t rec = xb + 2;
  if (len / rec < n) return STREAM_SHORT;
  for (size_t i = 0; i < n; ++i) {
    const uint8_t* p = buf + i * rec;
    const uint8_t zero = p[0], par = p[1 + xb];
    if ((zero != '0' && zero != '1') || (par != '0' && par != '1')) return STREAM_BAD_FLAG;
    uint8_t* xo = reinterpret_cast<uint8_t*>(x) + i * xb;
    if (zero == '1') {                             // either parity byte: the identity comes back as x = 0, flag 2
      memset(xo, 0, xb);
      flags[i] = 2;
    } else {
      memcpy(xo, p + 1, xb);
      flags[i] = par == '1' ? 1 : 0;
    }
  }
  return STREAM_OK;
}
}  // namespace mnt753
