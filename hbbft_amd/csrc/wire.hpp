// Host launcher of the wire-format kernels (k_wire.hip).  Kept out of launch.hpp so that the
// pairing translation units do not depend on it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wire_host.hpp"  // hbl::WIRE_* flags, parse_compressed

namespace hbl {

// G1Compressed::into_affine for n points: xw = 12 canonical LE words of x per point (flag bits
// cleared); out = ABI G1 points (all-zero when ok[i] == 0 or for infinity); ok[i] = 1 iff the
// encoding decodes to a point of the prime-order subgroup.
hipError_t g1_decompress(hipStream_t s, int n, const uint32_t* xw, const uint8_t* flags, void* out, uint8_t* ok);
// G2Compressed::into_affine: xw = 24 words per point (x.c0 then x.c1), out = ABI G2 points.
hipError_t g2_decompress(hipStream_t s, int n, const uint32_t* xw, const uint8_t* flags, void* out, uint8_t* ok);

// The latency form of the two decoders (k_wire_split.hip, HBH_DEC_SPLIT): the same arguments, the
// same bytes and verdicts; four lanes share one point's subgroup test, 16 points per workgroup.
hipError_t g1_decompress_split(hipStream_t s, int n, const uint32_t* xw, const uint8_t* flags, void* out, uint8_t* ok);
hipError_t g2_decompress_split(hipStream_t s, int n, const uint32_t* xw, const uint8_t* flags, void* out, uint8_t* ok);

// Device-side flag parsing + word reversal of n encodings (nfe = 1 for G1, 2 for G2) already in
// device memory: xw = 12 * nfe words per point, flags as above.
hipError_t wire_parse(hipStream_t s, int n, int nfe, const uint8_t* in, uint32_t* xw, uint8_t* flags);

}  // namespace hbl
