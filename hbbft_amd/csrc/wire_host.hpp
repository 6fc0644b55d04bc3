// Byte-level half of compressed point decoding on the host, and the per-point flags it hands to the
// wire-format kernels (wire.hpp).  No HIP here: tests/native/engine_host_test.cpp compiles this
// header for the CPU.
#pragma once
#include <cstdint>

namespace hbl {

// per-point flags prepared by the host from the compressed encoding's top bits
constexpr uint8_t WIRE_INFINITY = 1;  // valid encoding of the point at infinity
constexpr uint8_t WIRE_GREATEST = 2;  // the "y is the larger root" bit
constexpr uint8_t WIRE_REJECT = 4;    // malformed flags (not compressed, bad infinity encoding)

}  // namespace hbl

// Byte-level half of pairing 0.14's compressed decoding: flags (0x80 compressed, 0x40 infinity --
// then 0xc0 || 0...0 exactly --, 0x20 larger y) and the big-endian -> little-endian word reversal.
// The encoding holds nfe 48-byte field elements, highest Fp2 coefficient first (G2: x.c1 || x.c0);
// words come out as coefficient 0 first (12 words each).
inline void parse_compressed(const uint8_t* b, int nfe, uint32_t* words, uint8_t& f) {
  f = 0;
  if (!(b[0] & 0x80)) {
    f = hbl::WIRE_REJECT;
  } else if (b[0] & 0x40) {
    bool zero = (b[0] & 0x3f) == 0;
    for (int k = 1; k < 48 * nfe && zero; k++) zero = b[k] == 0;
    f = zero ? hbl::WIRE_INFINITY : hbl::WIRE_REJECT;
  } else if (b[0] & 0x20) {
    f = hbl::WIRE_GREATEST;
  }
  for (int c = 0; c < nfe; c++) {
    const uint8_t* e = b + 48 * (nfe - 1 - c);
    for (int w = 0; w < 12; w++) {
      uint32_t v = 0;
      for (int k = 0; k < 4; k++) {
        const int pos = 47 - (w * 4 + k);  // little-endian byte w*4+k of the element
        const uint8_t byte = (e == b && pos == 0) ? (uint8_t)(b[0] & 0x1f) : e[pos];
        v |= (uint32_t)byte << (8 * k);
      }
      words[c * 12 + w] = v;
    }
  }
}
