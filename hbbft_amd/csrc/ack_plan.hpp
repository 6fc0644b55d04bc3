// Host-side planning of the Ack checks: which rows to compute, in which order the acks run, and which
// of them take the finite-difference kernels.  No HIP here: tests/native/engine_host_test.cpp compiles
// this header for the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

// One row(x) per distinct (part, x), in order of first appearance: evaluate(x, y) = sum_j row(x)_j y^j.
// row_of[a] is the row of ack a.  False when a part index is >= nparts.
inline bool dedup_rows(size_t nack, size_t nparts, const uint32_t* part_idx, const uint32_t* xs,
                       std::vector<uint32_t>& row_part, std::vector<uint32_t>& row_x, std::vector<uint32_t>& row_of) {
  row_part.clear();
  row_x.clear();
  row_of.resize(nack);
  std::unordered_map<uint64_t, uint32_t> seen;
  seen.reserve(nack < 4096 ? nack : 4096);
  for (size_t a = 0; a < nack; a++) {
    if (part_idx[a] >= nparts) return false;
    const uint64_t key = ((uint64_t)part_idx[a] << 32) | xs[a];
    auto it = seen.emplace(key, (uint32_t)row_part.size());
    if (it.second) {
      row_part.push_back(part_idx[a]);
      row_x.push_back(xs[a]);
    }
    row_of[a] = it.first->second;
  }
  return true;
}

// Finite-difference plan of an Ack drain (hbl::bivar_fd): a row slot whose acks form a dense run of y
// -- at least 2 (t + 1) acks spanning at most twice as many consecutive y, as a node's drain has (one
// Ack per sender per Part) -- is evaluated at every y of its span from the difference table at y0 (the
// seed levels: (t+1)(t+2)/2 small products) and t additions per further y; its acks then compare
// against those points (epos).  y0 = 0 when the run starts at y <= t + 1 (the seed's products are then
// one per entry, worth the few extra steps), else the run's first y.  Every other ack takes the Horner
// kernel (other, in order of y).  FD rows are sorted by span length (the run kernel's workgroups step
// their rows together); a span is at least 2 (t + 1) points (the seed's two tables live in it).
struct FdPlan {
  std::vector<uint32_t> slot, y0, off, len;  // per FD row
  std::vector<uint32_t> epos;                // per ack (FD acks only)
  std::vector<uint32_t> fd_acks, other;      // ack lists
  size_t npts = 0;                           // E points of all FD rows
};
inline void plan_fd(size_t n, const std::vector<uint32_t>& slot, const uint32_t* ys, int t, FdPlan& P) {
  const uint64_t T1 = (uint64_t)t + 1;
  uint32_t nslot = 0;
  for (size_t a = 0; a < n; a++) nslot = std::max(nslot, slot[a] + 1);
  std::vector<uint32_t> cnt(nslot, 0), ymin(nslot, 0xffffffffu), ymax(nslot, 0);
  for (size_t a = 0; a < n; a++) {
    const uint32_t s = slot[a];
    cnt[s]++;
    ymin[s] = std::min(ymin[s], ys[a]);
    ymax[s] = std::max(ymax[s], ys[a]);
  }
  std::vector<uint32_t> cand;
  for (uint32_t s = 0; s < nslot; s++) {
    if (!cnt[s] || T1 > 128) continue;
    if (ymin[s] <= T1) ymin[s] = 0;  // seed at y0 = 0
    const uint64_t span = (uint64_t)ymax[s] - ymin[s] + 1;
    if (cnt[s] >= 2 * T1 && span >= 2 * T1 && span <= 2 * (uint64_t)cnt[s] && span < ((uint64_t)1 << 20))
      cand.push_back(s);
  }
  std::stable_sort(cand.begin(), cand.end(), [&](uint32_t a, uint32_t b) {
    const uint32_t la = ymax[a] - ymin[a], lb = ymax[b] - ymin[b];
    return la != lb ? la > lb : ymin[a] < ymin[b];
  });
  std::vector<int32_t> fd_of(nslot, -1);
  for (uint32_t s : cand) {
    fd_of[s] = (int32_t)P.slot.size();
    P.slot.push_back(s);
    P.y0.push_back(ymin[s]);
    P.off.push_back((uint32_t)P.npts);
    P.len.push_back(ymax[s] - ymin[s] + 1);  // >= 2 (t + 1)
    P.npts += ymax[s] - ymin[s] + 1;
  }
  P.epos.assign(n, 0);
  for (size_t a = 0; a < n; a++) {
    const int32_t f = fd_of[slot[a]];
    if (f < 0) {
      P.other.push_back((uint32_t)a);
    } else {
      P.epos[a] = P.off[f] + (ys[a] - P.y0[f]);
      P.fd_acks.push_back((uint32_t)a);
    }
  }
}

// Acks in order of y (stable): the lanes of a wave then run the same small-scalar double-and-add.
// y is a node index + 1, so a counting sort does it in O(n) (10^6 acks of a network-wide check).
// Round 4 measured (row tile, y) orders, whose waves re-read one tile's rows while they sit in L2:
// HBM traffic per 10^6 acks falls from 4.68 GB (this order) to 0.74 GB (tiles of 256 row slots) and
// 0.24 GB (1,024), but the launch is SLOWER at every tile size -- 54.2 ms here, 57.5 (64), 61.8-62.2
// (256), 60.6-60.8 (1,024), 57.4 (4,096) (profiles/r04/c11_ack_tile_traffic.txt; with an XCD-
// contiguous workgroup map as well: 57.5-58.2 ms, c3_ab.txt).  The kernel is VALU-bound at two
// waves per SIMD (255 VGPRs) and its row fetches overlap the Horner arithmetic, so this order stays.
inline void order_by_y(size_t n, const uint32_t* ys, std::vector<uint32_t>& order) {
  order.resize(n);
  uint32_t ymax = 0;
  for (size_t a = 0; a < n; a++) ymax = std::max(ymax, ys[a]);
  if (ymax < (1u << 20)) {
    std::vector<uint32_t> start((size_t)ymax + 2, 0);
    for (size_t a = 0; a < n; a++) start[(size_t)ys[a] + 1]++;
    for (size_t y = 1; y < start.size(); y++) start[y] += start[y - 1];
    for (size_t a = 0; a < n; a++) order[start[ys[a]]++] = (uint32_t)a;
    return;
  }
  for (size_t a = 0; a < n; a++) order[a] = (uint32_t)a;
  std::stable_sort(order.begin(), order.end(), [ys](uint32_t i, uint32_t j) { return ys[i] < ys[j]; });
}

// The plan of one Ack drain: with use_fd, plan_fd's rows in fd and the acks left to the Horner kernel
// (fd.other) in order of y in `order`; without it, or when no row qualifies, no FD row and every ack in
// `order`.  A caller that cannot run the FD kernels after all plans again with use_fd = false BEFORE it
// uploads anything: fd and order are rebuilt from nothing on every call.
inline void plan_drain(size_t n, const std::vector<uint32_t>& slot, const uint32_t* ys, int t, bool use_fd, FdPlan& fd,
                       std::vector<uint32_t>& order) {
  fd = FdPlan();
  if (use_fd) plan_fd(n, slot, ys, t, fd);
  if (fd.slot.empty()) {
    fd = FdPlan();
    return order_by_y(n, ys, order);
  }
  std::vector<uint32_t> oy(fd.other.size());
  for (size_t k = 0; k < fd.other.size(); k++) oy[k] = ys[fd.other[k]];
  order_by_y(oy.size(), oy.data(), order);
  for (auto& o : order) o = fd.other[o];
}
