// HBH_IMPL_OCT: the lane-octo pairing-equality kernel (gfx950) for batches of a few thousand checks.
//
// The check of pair_side.hpp lane_verify on EIGHT lanes: four lane pairs holding the check's state side
// by side, each step's independent products spread four per round (ofp.hpp).  A check's latency is
// ~0.6 of the lane quad's, and 8,192 checks are 1,024 waves (one per SIMD), so it serves the band
// between the wave-per-check kernel (interpreter-bound above ~4,000 checks) and the lane quad.
// (Kernel template; k_oct_g0/g1/g2.hip instantiate it per generator mode.)
#pragma once
#include "pair_side.hpp"
#include "ofp.hpp"

namespace hbs {

// GEN: 0 = both P read per check, 1 = P1 is the generator, 2 = P2 is the generator
template <bool W1, bool W2, int GEN>
// (one wave per SIMD: the four pairs' gather buffers are live across every round)
__global__ void __launch_bounds__(256, 1) k_oct_verify(PairArgs a) {
  extern __shared__ uint32_t stash_lds[];
  lane_verify<LaneOcto, ExpGs<LaneOcto>, W1, W2, GEN>(a, stash_lds);
}

}  // namespace hbs

namespace hbl {

struct OctKernels {
  static constexpr int LANES = hbs::LaneOcto::LANES;
  template <bool W1, bool W2, int GEN>
  static constexpr auto kernel = hbs::k_oct_verify<W1, W2, GEN>;
};

// one per translation unit (k_oct_g0/g1/g2.hip)
hipError_t oct_verify_g0(hipStream_t s, int n, const PairSideDesc& d1, const PairSideDesc& d2, int flags,
                         uint8_t* verdict, uint32_t* value_out);
hipError_t oct_verify_g1(hipStream_t s, int n, const PairSideDesc& d1, const PairSideDesc& d2, int flags,
                         uint8_t* verdict, uint32_t* value_out);
hipError_t oct_verify_g2(hipStream_t s, int n, const PairSideDesc& d1, const PairSideDesc& d2, int flags,
                         uint8_t* verdict, uint32_t* value_out);

}  // namespace hbl
