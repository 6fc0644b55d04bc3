// Host-side planning of the grouped random-combination share checks (hbh_verify_*_shares_grouped):
// which items share a table entry (a document's H, a ciphertext's H_uv and W), how a group is cut
// into the tiles that one workgroup of k_group_sum sums, and which items take the per-share check
// afterwards.  No HIP here: tests/csrc/group_plan_check.cpp compiles this header for the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// Items per tile: one workgroup of k_group_sum (k_rlc.hip) sums a tile, one chain per (item, digit).
// 128 items x 2 digits fill the 256 threads of the G2 sum; the G1 sum runs one chain per item.
constexpr uint32_t GROUP_TILE = 128;

// One group per table entry that occurs in idx, in order of the entry; group g holds the call's items
// perm[goff[g] .. goff[g + 1]) in their order in the call (perm is a bijection of [0, n)).  A group of
// at least min_combine items is COMBINED: it is combined group c (comb[c] = g, in group order) and
// owns the tiles [ctile[c], ctile[c + 1]); tile t covers tile_len[t] <= GROUP_TILE positions of perm
// from tile_off[t].  Every other group's items go to `singles`: they are not combined and take the
// per-share check.  min_combine = 2 for the verify calls, 1 for hbh_dbg_group_sums.
struct GroupPlan {
  std::vector<uint32_t> entry, goff, perm;
  std::vector<uint32_t> comb, ctile, tile_off, tile_len;
  std::vector<uint32_t> singles;
};

// False when an index is >= table (nothing is planned then).
inline bool plan_groups(size_t n, const uint32_t* idx, size_t table, uint32_t min_combine, GroupPlan& P) {
  P = GroupPlan();
  for (size_t i = 0; i < n; i++)
    if (idx[i] >= table) return false;
  std::vector<uint32_t> start(table + 1, 0);
  for (size_t i = 0; i < n; i++) start[(size_t)idx[i] + 1]++;
  P.goff.push_back(0);
  for (size_t k = 0; k < table; k++) {
    const uint32_t cnt = start[k + 1];
    start[k + 1] += start[k];
    if (!cnt) continue;  // an absent entry yields no group
    P.entry.push_back((uint32_t)k);
    P.goff.push_back(start[k + 1]);
  }
  P.perm.resize(n);
  for (size_t i = 0; i < n; i++) P.perm[start[idx[i]]++] = (uint32_t)i;  // counting sort: stable
  P.ctile.push_back(0);
  for (size_t g = 0; g < P.entry.size(); g++) {
    const uint32_t lo = P.goff[g], hi = P.goff[g + 1];
    if (hi - lo < min_combine) {
      for (uint32_t p = lo; p < hi; p++) P.singles.push_back(P.perm[p]);
      continue;
    }
    P.comb.push_back((uint32_t)g);
    for (uint32_t p = lo; p < hi; p += GROUP_TILE) {
      P.tile_off.push_back(p);
      P.tile_len.push_back(hi - p < GROUP_TILE ? hi - p : GROUP_TILE);
    }
    P.ctile.push_back((uint32_t)P.tile_off.size());
  }
  return true;
}

// The items of the per-share check once the verdicts of the combined groups are known (verdict[c] of
// combined group c, nonzero = the group equation held): every item of a failed group, in group order,
// then the singles.
inline void plan_fallback(const GroupPlan& P, const uint8_t* verdict, std::vector<uint32_t>& list) {
  list.clear();
  for (size_t c = 0; c < P.comb.size(); c++) {
    if (verdict[c]) continue;
    const uint32_t g = P.comb[c];
    list.insert(list.end(), P.perm.begin() + P.goff[g], P.perm.begin() + P.goff[g + 1]);
  }
  list.insert(list.end(), P.singles.begin(), P.singles.end());
}
