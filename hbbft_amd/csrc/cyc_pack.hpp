// Lane layout of the packed cyclotomic-squaring runs (k_wavep.hip, k_wave.hpp cyc_run_packed): one
// wave squares the Fp12 values of `pack` checks side by side.  A check takes 18 lanes,
//   lane = 18 c + 6 role + 2 j + h,
// c < pack the check, role < 3 the Fp4 squaring of the Granger-Scott split ((f0, f3), (f1, f4),
// (f2, f5)), j < 3 the Fp2 square it computes (A, B, A + B) and h the Fp2 component, so the two lanes
// of an Fp2 value are (even, odd) neighbours (the DPP swap of the lane-pair arithmetic).  Lanes j < 2
// hold the value's components between squarings (position role + 3 j of the w-basis); lanes from
// 18 pack on idle.  Plain constexpr functions, no HIP constructs: the host includes this header too
// (tests/test_cyc_pack_layout.py).
#pragma once

namespace cycpack {

constexpr int CHECK_LANES = 18;  // 3 roles x 3 squares x 2 components
constexpr int WAVE_LANES = 64;

constexpr int max_pack() { return WAVE_LANES / CHECK_LANES; }
constexpr int active_lanes(int pack) { return CHECK_LANES * pack; }
constexpr bool is_active(int lane, int pack) { return lane >= 0 && lane < active_lanes(pack); }

constexpr int lane_of(int c, int role, int j, int h) { return CHECK_LANES * c + 6 * role + 2 * j + h; }
constexpr int check_of(int lane) { return lane / CHECK_LANES; }
constexpr int role_of(int lane) { return (lane % CHECK_LANES) / 6; }
constexpr int square_of(int lane) { return (lane % 6) / 2; }
constexpr int comp_of(int lane) { return lane & 1; }

// lanes that keep a component of the value between squarings (A and B of each role)
constexpr bool is_holder(int lane, int pack) { return is_active(lane, pack) && square_of(lane) < 2; }

// the lane of this lane's (check, role) that holds / squares A (k = 0), B (k = 1), A + B (k = 2),
// same component; an idle lane names itself
constexpr int source_lane(int lane, int k, int pack) {
  return is_active(lane, pack) ? lane_of(check_of(lane), role_of(lane), k, comp_of(lane)) : lane;
}
// the lane that holds the input at this lane's output position: roles 1 and 2 trade, role 0 and
// idle lanes keep their own
constexpr int partner_lane(int lane, int pack) {
  return !is_active(lane, pack) || role_of(lane) == 0
             ? lane
             : lane_of(check_of(lane), 3 - role_of(lane), square_of(lane), comp_of(lane));
}

}  // namespace cycpack
