// Stand-alone check of hbbft_amd/csrc/batch_plan.hpp (host planning of the batched independent checks):
// the groups of BATCH_GROUP consecutive items, the single, the tiles of the G2 sums, the tiles of the
// Miller-product launch at each lane width, the slots AUTO reads, and the fallback lists.  Prints
// "BATCH_GROUP <n>" and "batch_plan: 0 bad of <checks>"; exit status 1 on any failure.
// tests/test_batch_plan_host.py builds it plain and with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <vector>

#include "batch_plan.hpp"

static long g_checks = 0, g_bad = 0;
#define CHECK(cond)                                                                \
  do {                                                                             \
    g_checks++;                                                                    \
    if (!(cond)) {                                                                 \
      if (g_bad++ < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
    }                                                                              \
  } while (0)

static void check_plan(size_t n, uint32_t min_combine) {
  BatchPlan B;
  plan_batch(n, min_combine, B);
  const GroupPlan& P = B.groups;
  const size_t ngroups = (n + BATCH_GROUP - 1) / BATCH_GROUP;
  const bool single = min_combine == 2 && n % BATCH_GROUP == 1;
  // the groups are the runs of 256 items in call order: perm is the identity
  CHECK(P.entry.size() == ngroups && P.goff.size() == ngroups + 1 && P.perm.size() == n);
  for (size_t i = 0; i < n; i++) CHECK(P.perm[i] == i);
  for (size_t g = 0; g < ngroups; g++) {
    CHECK(P.entry[g] == g && P.goff[g] == g * BATCH_GROUP);
    CHECK(P.goff[g + 1] == (n < (g + 1) * BATCH_GROUP ? n : (g + 1) * BATCH_GROUP));
  }
  // a last group of one item is the single; every other group is combined, in order
  CHECK(B.ngroup == ngroups - (single ? 1 : 0) && P.comb.size() == B.ngroup);
  for (size_t c = 0; c < P.comb.size(); c++) CHECK(P.comb[c] == c);
  CHECK(P.singles.size() == (single ? 1u : 0u));
  if (single) CHECK(P.singles[0] == n - 1);
  CHECK(B.nitems == n - (single ? 1 : 0));
  CHECK(batch_slots(B) == (B.nitems + 1) / 2);
  // tiles of the G2 sums: each group's positions in order, GROUP_TILE items but the last
  CHECK(P.ctile.size() == B.ngroup + 1 && P.ctile.back() == P.tile_off.size());
  for (size_t c = 0; c < B.ngroup; c++) {
    const uint32_t size = P.goff[c + 1] - P.goff[c];
    CHECK(P.ctile[c + 1] - P.ctile[c] == (size + GROUP_TILE - 1) / GROUP_TILE);
    uint32_t pos = P.goff[c];
    for (uint32_t t = P.ctile[c]; t < P.ctile[c + 1]; t++) {
      CHECK(P.tile_off[t] == pos && P.tile_len[t] >= 1 && P.tile_len[t] <= GROUP_TILE);
      pos += P.tile_len[t];
    }
    CHECK(pos == P.goff[c + 1]);
  }
  // tiles of the Miller-product launch: 1, 2, 4 per group on 2, 4, 8 lanes; tile b holds the items
  // [b T, (b + 1) T), which never straddle a group, and together the tiles cover [0, nitems)
  const uint32_t lanes[3] = {2, 4, 8}, items[3] = {256, 128, 64}, per_group[3] = {1, 2, 4};
  for (int k = 0; k < 3; k++) {
    const uint32_t T = batch_tile_items(lanes[k]), tpg = batch_tiles_per_group(lanes[k]);
    CHECK(T == items[k] && tpg == per_group[k] && T * tpg == BATCH_GROUP);
    const uint32_t nt = batch_miller_tiles(B, lanes[k]);
    CHECK(nt == B.ngroup * tpg);
    CHECK((size_t)nt * T >= B.nitems && (B.ngroup == 0 || (size_t)(nt - tpg) * T < B.nitems));
    for (uint32_t b = 0; b < nt; b++) CHECK((b * T) / BATCH_GROUP == ((b + 1) * T - 1) / BATCH_GROUP && (b * T) / BATCH_GROUP == b / tpg);
  }
  // fallback lists: every item of a failed group in order, then the single
  for (int round = 0; round < 3; round++) {
    std::vector<uint8_t> verdict(B.ngroup + 1, 1);
    for (size_t c = 0; c < B.ngroup; c++) verdict[c] = round == 0 ? 1 : round == 1 ? 0 : (uint8_t)((c + n) & 1);
    std::vector<uint32_t> list, want;
    plan_batch_fallback(B, verdict.data(), list);
    for (size_t c = 0; c < B.ngroup; c++)
      if (!verdict[c])
        for (uint32_t i = P.goff[c]; i < P.goff[c + 1]; i++) want.push_back(i);
    if (single) want.push_back((uint32_t)n - 1);
    CHECK(list == want);
  }
}

int main() {
  std::printf("BATCH_GROUP %u\n", BATCH_GROUP);
  const size_t sizes[] = {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 511, 512, 513, 1024, 10100};
  for (size_t n : sizes) {
    check_plan(n, 2);
    check_plan(n, 1);
  }
  // n = 0 plans nothing; n = 1 is one single (verify) or one group (the debug entry)
  BatchPlan B;
  plan_batch(0, 2, B);
  CHECK(B.ngroup == 0 && B.nitems == 0 && batch_slots(B) == 0 && batch_miller_tiles(B, 2) == 0);
  plan_batch(1, 2, B);
  CHECK(B.ngroup == 0 && B.nitems == 0 && B.groups.singles.size() == 1);
  plan_batch(1, 1, B);
  CHECK(B.ngroup == 1 && B.nitems == 1 && B.groups.singles.empty() && batch_miller_tiles(B, 8) == 4);
  plan_batch(257, 2, B);
  CHECK(B.ngroup == 1 && B.nitems == 256 && batch_slots(B) == 128 && B.groups.singles[0] == 256);
  std::printf("batch_plan: %ld bad of %ld\n", g_bad, g_checks);
  return g_bad ? 1 : 0;
}
