// HBH_IMPL_QUAD: the lane-quad pairing-equality kernel (gfx950) for mid-size batches.
// (Kernel template; k_quad_g0/g1/g2.hip instantiate it per generator mode so the three ~3-minute
// compiles run in parallel.)
//
// The check of pair_side.hpp lane_verify -- FE(f_{|x|,Q1}(P1) f_{|x|,Q2}(-P2)) == 1, pairing 0.14's Miller
// loop and final exponentiation -- on FOUR lanes per check: two lane pairs that hold the check's state
// side by side and split each step's independent products between them (qfp.hpp).  The lane-pair
// kernel's latency floor is one lane pair's whole check (10.6 ms); below ~32,768 checks it cannot
// fill the SIMDs, and the wave-per-check kernel's interpreter overhead caps it at ~0.8 M checks/s.
// Here a batch of 16,384 checks is 1,024 waves, one per SIMD, and a check takes ~0.55 of the lane
// pair's per-lane products (7.1 ms per batch of <= 16,384, profiles/r04/c8_sweep_wave_quad_pair.txt):
// the protocol's natural batch points (BA replays, remove_invalid_shares:
// src/binary_agreement/binary_agreement.rs:250-264, 507-519; src/threshold_decrypt.rs:204-217).
//
// One wave per SIMD is the design point: __launch_bounds__(256, 1) gives a lane up to 512 registers
// (256 VGPR + 256 AGPR), so the two pairs' operand sets of a dual product stay in registers.  The
// final exponentiation parks one Fp12 per lane in LDS (72 KiB per 256-lane workgroup), as k_pair.
#pragma once
#include "pair_side.hpp"

namespace hbs {

// GEN: 0 = both P read per check, 1 = P1 is the generator, 2 = P2 is the generator
template <bool W1, bool W2, int GEN>
// (two waves per SIMD -- 256 registers, 4,112 VGPR spills -- measured slower: 16,384 checks 9.29 vs
// 7.09 ms, 32,768 checks 15.5 vs 14.2 ms, profiles/r04/c10_ab.txt)
__global__ void __launch_bounds__(256, 1) k_quad_verify(PairArgs a) {
  extern __shared__ uint32_t stash_lds[];
  lane_verify<LaneQuad, ExpGs<LaneQuad>, W1, W2, GEN>(a, stash_lds);
}

}  // namespace hbs

namespace hbl {

struct QuadKernels {
  static constexpr int LANES = hbs::LaneQuad::LANES;
  template <bool W1, bool W2, int GEN>
  static constexpr auto kernel = hbs::k_quad_verify<W1, W2, GEN>;
};

// one per translation unit (k_quad_g0/g1/g2.hip)
hipError_t quad_verify_g0(hipStream_t s, int n, const PairSideDesc& d1, const PairSideDesc& d2, int flags,
                          uint8_t* verdict, uint32_t* value_out);
hipError_t quad_verify_g1(hipStream_t s, int n, const PairSideDesc& d1, const PairSideDesc& d2, int flags,
                          uint8_t* verdict, uint32_t* value_out);
hipError_t quad_verify_g2(hipStream_t s, int n, const PairSideDesc& d1, const PairSideDesc& d2, int flags,
                          uint8_t* verdict, uint32_t* value_out);

}  // namespace hbl
