// Host-side planning of the batched independent checks (hbh_verify_signatures_batched,
// hbh_verify_ciphertexts_uv_batched, hbh_dbg_pairing_product): the groups of BATCH_GROUP consecutive
// items, the tiles of the G2 group sums (group_plan.hpp), the tiles of the Miller-product launch per lane
// width, and the items of the per-item fallback.  No HIP here: tests/csrc/batch_plan_check.cpp compiles
// this header for the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "group_plan.hpp"

constexpr uint32_t BATCH_GROUP = 256;  // == HBH_BATCH_GROUP

// Items per tile of the Miller-product launch: one 256-thread workgroup of `lanes` lanes per slot, two
// items per slot (2, 4, 8 lanes: 256, 128, 64 items).  A tile never straddles two groups.
constexpr uint32_t batch_tile_items(uint32_t lanes) { return 2 * 256 / lanes; }
constexpr uint32_t batch_tiles_per_group(uint32_t lanes) { return BATCH_GROUP / batch_tile_items(lanes); }
static_assert(batch_tiles_per_group(2) == 1 && batch_tiles_per_group(4) == 2 && batch_tiles_per_group(8) == 4,
              "a group is 1, 2 or 4 tiles");

struct BatchPlan {
  GroupPlan groups;    // group g = the items [256 g, min(n, 256 g + 256)); the combined groups come first
  uint32_t ngroup;     // combined groups (each one final exponentiation)
  uint32_t nitems;     // items in the combined groups: [0, nitems), the Miller-product launch's n
};

// min_combine = 2 for the verify calls (a last group of one item is a single), 1 for
// hbh_dbg_pairing_product (every group has a value).
inline void plan_batch(size_t n, uint32_t min_combine, BatchPlan& B) {
  std::vector<uint32_t> idx(n);
  for (size_t i = 0; i < n; i++) idx[i] = (uint32_t)(i / BATCH_GROUP);
  plan_groups(n, idx.data(), (n + BATCH_GROUP - 1) / BATCH_GROUP, min_combine, B.groups);
  B.ngroup = (uint32_t)B.groups.comb.size();
  B.nitems = (uint32_t)(n - B.groups.singles.size());
}

// Tiles of the Miller-product launch: every combined group gets batch_tiles_per_group(lanes) tiles, the
// last group's tiles past its items hold inactive pairs only (their product is 1), so every group feeds
// the same number of values to the product.
inline uint32_t batch_miller_tiles(const BatchPlan& B, uint32_t lanes) { return B.ngroup * batch_tiles_per_group(lanes); }

// Lane-kernel slots of the launch (two items each): what HBH_IMPL_AUTO's ladder is read against.
inline size_t batch_slots(const BatchPlan& B) { return ((size_t)B.nitems + 1) / 2; }

// The items of the per-item check once the group verdicts are known: plan_fallback's list.
inline void plan_batch_fallback(const BatchPlan& B, const uint8_t* verdict, std::vector<uint32_t>& list) {
  plan_fallback(B.groups, verdict, list);
}
