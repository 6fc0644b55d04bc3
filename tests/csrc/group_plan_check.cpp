// Stand-alone check of hbbft_amd/csrc/group_plan.hpp (host planning of the grouped share checks):
// the CSR groups, the permutation, the tiles, the singles and the fallback gather list, on shuffled
// index arrays.  Prints "GROUP_TILE <n>" and "group_plan: 0 bad of <checks>"; exit status 1 on any
// failure.  tests/test_group_plan_host.py builds it plain and with the address and undefined-behaviour
// sanitizers.
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "group_plan.hpp"

static long g_checks = 0, g_bad = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    g_checks++;                                                  \
    if (!(cond)) {                                               \
      if (g_bad++ < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
    }                                                            \
  } while (0)

// sizes[k] items name table entry k (0 = the entry is absent), in an order shuffled by `seed`
static std::vector<uint32_t> shuffled_idx(const std::vector<uint32_t>& sizes, unsigned seed) {
  std::vector<uint32_t> idx;
  for (size_t k = 0; k < sizes.size(); k++) idx.insert(idx.end(), sizes[k], (uint32_t)k);
  std::mt19937 rng(seed);
  std::shuffle(idx.begin(), idx.end(), rng);
  return idx;
}

static void check_plan(const std::vector<uint32_t>& sizes, uint32_t min_combine, unsigned seed) {
  const std::vector<uint32_t> idx = shuffled_idx(sizes, seed);
  const size_t n = idx.size(), table = sizes.size();
  GroupPlan P;
  CHECK(plan_groups(n, idx.data(), table, min_combine, P));
  // one group per entry that occurs, in entry order; absent entries yield none
  std::vector<uint32_t> present;
  for (size_t k = 0; k < table; k++)
    if (sizes[k]) present.push_back((uint32_t)k);
  CHECK(P.entry == present);
  CHECK(P.goff.size() == present.size() + 1 && P.goff.front() == 0 && P.goff.back() == n);
  // perm is a bijection of [0, n)
  CHECK(P.perm.size() == n);
  std::vector<uint32_t> sorted = P.perm;
  std::sort(sorted.begin(), sorted.end());
  for (size_t i = 0; i < n; i++) CHECK(sorted[i] == i);
  // CSR: group g holds exactly the items of its entry, in call order
  for (size_t g = 0; g + 1 < P.goff.size(); g++) {
    CHECK(P.goff[g + 1] - P.goff[g] == sizes[P.entry[g]]);
    for (uint32_t p = P.goff[g]; p < P.goff[g + 1]; p++) {
      CHECK(idx[P.perm[p]] == P.entry[g]);
      if (p > P.goff[g]) CHECK(P.perm[p - 1] < P.perm[p]);
    }
  }
  // combined groups and singles
  std::vector<uint32_t> want_comb, want_singles;
  for (size_t g = 0; g < P.entry.size(); g++) {
    if (sizes[P.entry[g]] >= min_combine)
      want_comb.push_back((uint32_t)g);
    else
      for (uint32_t p = P.goff[g]; p < P.goff[g + 1]; p++) want_singles.push_back(P.perm[p]);
  }
  CHECK(P.comb == want_comb);
  CHECK(P.singles == want_singles);
  for (uint32_t i : P.singles) CHECK(sizes[idx[i]] < min_combine);
  // tiles: group c's tiles cover its positions in order, each of 1..GROUP_TILE items, all full but the last
  CHECK(P.ctile.size() == P.comb.size() + 1 && P.ctile.front() == 0 && P.ctile.back() == P.tile_off.size());
  CHECK(P.tile_len.size() == P.tile_off.size());
  for (size_t c = 0; c < P.comb.size(); c++) {
    const uint32_t g = P.comb[c], size = P.goff[g + 1] - P.goff[g];
    CHECK(P.ctile[c + 1] - P.ctile[c] == (size + GROUP_TILE - 1) / GROUP_TILE);
    uint32_t pos = P.goff[g];
    for (uint32_t t = P.ctile[c]; t < P.ctile[c + 1]; t++) {
      CHECK(P.tile_off[t] == pos);
      CHECK(P.tile_len[t] >= 1 && P.tile_len[t] <= GROUP_TILE);
      if (t + 1 < P.ctile[c + 1]) CHECK(P.tile_len[t] == GROUP_TILE);
      pos += P.tile_len[t];
    }
    CHECK(pos == P.goff[g + 1]);
  }
  // the fallback list for a group-verdict vector: the items of the failed groups, then the singles
  std::mt19937 rng(seed + 77);
  for (int round = 0; round < 4; round++) {
    std::vector<uint8_t> verdict(P.comb.size() + 1, 1);  // + 1: data() of an empty vector may be null
    for (size_t c = 0; c < P.comb.size(); c++) verdict[c] = round == 0 ? 1 : round == 1 ? 0 : (uint8_t)(rng() & 1);
    std::vector<uint32_t> list, want;
    plan_fallback(P, verdict.data(), list);
    for (size_t c = 0; c < P.comb.size(); c++)
      if (!verdict[c])
        for (uint32_t p = P.goff[P.comb[c]]; p < P.goff[P.comb[c] + 1]; p++) want.push_back(P.perm[p]);
    want.insert(want.end(), P.singles.begin(), P.singles.end());
    CHECK(list == want);
    std::vector<uint32_t> uniq = list;
    std::sort(uniq.begin(), uniq.end());
    CHECK(std::adjacent_find(uniq.begin(), uniq.end()) == uniq.end());
  }
}

int main() {
  std::printf("GROUP_TILE %u\n", GROUP_TILE);
  const uint32_t T = GROUP_TILE;
  const std::vector<std::vector<uint32_t>> shapes = {
      {1, 2, T - 1, T, T + 1, 2 * T + 5},           // the tile bounds
      {0, 1, 0, 2, 0, 0, T + 1, 0},                 // absent entries
      {1, 1, 1, 1},                                 // singles only
      {0, 0, 0},                                    // nothing
      {3 * T, 1, 64, 64, 64, 100, 0, 2 * T + 5, 2}, // mixed
      {},                                           // empty table
  };
  for (size_t k = 0; k < shapes.size(); k++)
    for (unsigned seed = 1; seed <= 3; seed++) {
      check_plan(shapes[k], 2, 100 * (unsigned)k + seed);
      check_plan(shapes[k], 1, 100 * (unsigned)k + seed);
    }
  // an index past the table plans nothing
  {
    const uint32_t idx[3] = {0, 3, 1};
    GroupPlan P;
    CHECK(!plan_groups(3, idx, 3, 2, P));
    CHECK(P.perm.empty() && P.comb.empty() && P.singles.empty());
    CHECK(plan_groups(3, idx, 4, 2, P));
    CHECK(P.singles.size() == 3 && P.comb.empty() && P.tile_off.empty());
  }
  std::printf("group_plan: %ld bad of %ld\n", g_bad, g_checks);
  return g_bad ? 1 : 0;
}
