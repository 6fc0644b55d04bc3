// Device-resident commitment sets (hbh_commit_set_*) and the row and Ack checks that read them.
#include <unordered_map>

#include "ack_plan.hpp"  // host planning (no HIP, tested on the CPU: tests/test_engine_host.py)
#include "engine_impl.hpp"

using namespace hbe;

// ProposalState::commit (src/sync_key_gen.rs:254-262) lives as long as the SyncKeyGen instance and
// is read by every row check (:496) and every Ack check (:542): a set keeps such commitments in HBM
// (uploaded once) together with the Jacobian rows row(x) computed so far, so an Ack drain uploads
// only its indices and values.
struct hbh_commit_set {
  hbh_engine* e = nullptr;
  int t = 0;
  size_t ncoef = 0;
  size_t nparts = 0;
  void* commits = nullptr;  // nparts * ncoef ABI G1 points
  size_t commits_cap = 0;   // bytes
  // cached rows row(x), two layouts: [0] Jacobian signed-limb rows of the lane-quad check
  // (hbl::bivar_rows_quad_bytes(1, t) each), [1] affine ABI rows of the one-lane check
  // ((t + 1) G1 points each)
  struct Rows {
    std::unordered_map<uint64_t, uint32_t> slot;  // (part << 32 | x) -> row
    size_t n = 0;
    void* p = nullptr;
    size_t cap = 0;  // bytes
  } rows[2];
  DevBuf stage;      // indices of rows computed by a call
};

void hbe::release_set_device(hbh_commit_set* cs) {
  if (cs->commits) (void)hipFree(cs->commits);
  cs->commits = nullptr;
  cs->commits_cap = 0;
  cs->nparts = 0;
  for (auto& R : cs->rows) {
    if (R.p) (void)hipFree(R.p);
    R.p = nullptr;
    R.cap = 0;
    R.n = 0;
    R.slot.clear();
  }
  cs->stage.release();
  cs->e = nullptr;
}

namespace {
// Grow a device allocation to at least `want` bytes, keeping its first `used` bytes.
int grow_keep(hipStream_t s, void** p, size_t* cap, size_t used, size_t want) {
  if (want <= *cap) return HBH_OK;
  const size_t nc = std::max(want, *cap * 2);
  void* q = nullptr;
  HBH_CHECK(hipMalloc(&q, nc));
  if (used) HBH_CHECK(hipMemcpyAsync(q, *p, used, hipMemcpyDeviceToDevice, s));
  HBH_CHECK(hipStreamSynchronize(s));
  if (*p) HBH_CHECK(hipFree(*p));
  *p = q;
  *cap = nc;
  return HBH_OK;
}

// Row slots for n (part, x) requests; rows not cached yet are computed on stream s (k_bivar_row_quad
// into the set's row buffer).  Caller holds the engine lock.
int set_rows(hbh_commit_set* cs, hipStream_t s, bool affine, size_t n, const uint32_t* part_idx, const uint32_t* xs,
             std::vector<uint32_t>& slot) {
  hbh_commit_set::Rows& R = cs->rows[affine ? 1 : 0];
  std::vector<uint32_t> np, nx;
  slot.resize(n);
  uint64_t last_key = ~(uint64_t)0;
  uint32_t last_slot = 0;
  for (size_t a = 0; a < n; a++) {
    const uint64_t key = ((uint64_t)part_idx[a] << 32) | xs[a];
    if (key != last_key) {  // consecutive acks of one (part, x) skip the map
      auto it = R.slot.emplace(key, (uint32_t)(R.n + np.size()));
      if (it.second) {
        np.push_back(part_idx[a]);
        nx.push_back(xs[a]);
      }
      last_key = key;
      last_slot = it.first->second;
    }
    slot[a] = last_slot;
  }
  if (np.empty()) return HBH_OK;
  const size_t row_bytes = affine ? (size_t)(cs->t + 1) * HBH_G1_BYTES : hbl::bivar_rows_quad_bytes(1, cs->t);
  const size_t first = R.n;
  auto compute = [&]() -> int {
    int rc = grow_keep(s, &R.p, &R.cap, first * row_bytes, (first + np.size()) * row_bytes);
    if (rc) return rc;
    HBH_CHECK(cs->stage.ensure(np.size() * 8));
    uint32_t* d_p = (uint32_t*)cs->stage.p;
    HBH_CHECK(h2d(s, d_p, np.data(), np.size() * 4));
    HBH_CHECK(h2d(s, d_p + np.size(), nx.data(), nx.size() * 4));
    StageScope tm(cs->e, s, HBH_STAGE_CURVE);
    void* dst = (uint8_t*)R.p + first * row_bytes;
    if (affine)
      HBH_CHECK(hbl::bivar_row(s, (int)np.size(), cs->t, cs->commits, d_p, d_p + np.size(), dst));
    else
      HBH_CHECK(hbl::bivar_row_quad(s, (int)np.size(), cs->t, cs->commits, d_p, d_p + np.size(), dst));
    tm.stop();
    // the staged indices are read by the kernel: the host vectors die at return
    HBH_CHECK(hipStreamSynchronize(s));
    return HBH_OK;
  };
  const int rc = compute();
  if (rc) {  // the new slots were never filled: forget them, so no later ack reads an empty row
    for (size_t k = 0; k < np.size(); k++) R.slot.erase(((uint64_t)np[k] << 32) | nx[k]);
    return rc;
  }
  R.n = first + np.size();
  return HBH_OK;
}

int check_parts(const hbh_commit_set* cs, size_t n, const uint32_t* part_idx) {
  for (size_t a = 0; a < n; a++)
    if (part_idx[a] >= cs->nparts) return fail(HBH_ERR_ARG, "part index out of range");
  return HBH_OK;
}

// The 16-bit comb of g1 (the FD ack check), built on s the first time a drain plans FD rows.
int ensure_fb16(hbh_engine* e, hipStream_t s) {
  if (e->fb16_ready) return HBH_OK;
  HBH_CHECK(e->fb16.ensure(hbl::fb16_table_bytes()));
  DevBuf scratch;  // ~192 MiB: freed before return, also on failure
  hipError_t err = scratch.ensure(hbl::fb16_scratch_bytes());
  if (err == hipSuccess) err = hbl::fb16_table(s, e->fb16.p, scratch.p);
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  scratch.release();
  HBH_CHECK(err);
  e->fb16_ready = true;
  return HBH_OK;
}
}  // namespace

extern "C" {

int hbh_commit_set_create(hbh_engine* e, int t, hbh_commit_set** out) {
  if (!e || !out) return fail(HBH_ERR_ARG, "null pointer");
  *out = nullptr;
  int rc = check_t(t);
  if (rc) return rc;
  hbh_commit_set* cs = new hbh_commit_set();
  cs->e = e;
  cs->t = t;
  cs->ncoef = (size_t)(t + 1) * (t + 2) / 2;
  {
    std::lock_guard<std::mutex> lk(e->mu);
    e->sets.insert(cs);
  }
  *out = cs;
  return HBH_OK;
}

int hbh_commit_set_destroy(hbh_commit_set* cs) {
  if (!cs) return HBH_OK;
  if (hbh_engine* e = cs->e) {  // else: detached by hbh_engine_destroy, device memory already freed
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    (void)hipEventSynchronize(e->done);
    (void)hipStreamSynchronize(e->stream);
    e->sets.erase(cs);
    release_set_device(cs);
  }
  delete cs;
  return HBH_OK;
}

int hbh_commit_set_add(hbh_commit_set* cs, size_t nparts, const uint8_t* commits, size_t* first) {
  if (!cs) return fail(HBH_ERR_ARG, "null commitment set");
  if (!cs->e) return fail(HBH_ERR_ARG, "commitment set detached: its engine was destroyed");
  if (first) *first = cs->nparts;
  if (nparts == 0) return HBH_OK;
  if (!commits) return fail(HBH_ERR_ARG, "null pointer");
  if (cs->nparts + nparts > ((size_t)1 << 24)) return fail(HBH_ERR_ARG, "too many commitments");
  hbh_engine* e = cs->e;
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  const size_t cb = cs->ncoef * HBH_G1_BYTES;
  int rc = grow_keep(s, &cs->commits, &cs->commits_cap, cs->nparts * cb, (cs->nparts + nparts) * cb);
  if (rc) return rc;
  HBH_CHECK(h2d(s, (uint8_t*)cs->commits + cs->nparts * cb, commits, nparts * cb));
  rc = call.finish();
  if (rc) return rc;
  cs->nparts += nparts;
  return HBH_OK;
}

int hbh_commit_set_size(const hbh_commit_set* cs, size_t* nparts, size_t* nrows) {
  if (!cs) return fail(HBH_ERR_ARG, "null commitment set");
  if (nparts) *nparts = cs->nparts;
  if (nrows) *nrows = cs->rows[0].n + cs->rows[1].n;
  return HBH_OK;
}

int hbh_bivar_row_set(hbh_commit_set* cs, size_t nrow, const uint32_t* part_idx, const uint32_t* xs, uint8_t* out) {
  if (!cs) return fail(HBH_ERR_ARG, "null commitment set");
  if (!cs->e) return fail(HBH_ERR_ARG, "commitment set detached: its engine was destroyed");
  if (nrow == 0) return HBH_OK;
  if (!part_idx || !xs || !out) return fail(HBH_ERR_ARG, "null pointer");
  int rc = check_parts(cs, nrow, part_idx);
  if (rc) return rc;
  hbh_engine* e = cs->e;
  const int t = cs->t;
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  const size_t nout = nrow * (t + 1);
  HBH_CHECK(e->in_b.ensure(nrow * 8));
  HBH_CHECK(e->out_x.ensure(nout * HBH_G1_BYTES));
  uint32_t* d_p = (uint32_t*)e->in_b.p;
  HBH_CHECK(h2d(s, d_p, part_idx, nrow * 4));
  HBH_CHECK(h2d(s, d_p + nrow, xs, nrow * 4));
  {
    StageScope tm(e, s, HBH_STAGE_CURVE);
    HBH_CHECK(hbl::bivar_row(s, (int)nrow, t, cs->commits, d_p, d_p + nrow, e->out_x.p));
  }
  HBH_CHECK(download(s, out, e->out_x, nout * HBH_G1_BYTES));
  return call.finish();
}

int hbh_bivar_ack_check_set(hbh_commit_set* cs, size_t nack, const uint32_t* part_idx, const uint32_t* xs,
                            const uint32_t* ys, const uint8_t* vals, uint8_t* verdicts) {
  if (!cs) return fail(HBH_ERR_ARG, "null commitment set");
  if (!cs->e) return fail(HBH_ERR_ARG, "commitment set detached: its engine was destroyed");
  if (nack == 0) return HBH_OK;
  if (!part_idx || !xs || !ys || !vals || !verdicts) return fail(HBH_ERR_ARG, "null pointer");
  if (nack > ((size_t)1 << 28)) return fail(HBH_ERR_ARG, "batch too large");
  int rc = check_parts(cs, nack, part_idx);
  if (rc) return rc;
  std::vector<uint32_t> slot, order;  // read by queued copies: declared before the call, which drains the stream
  FdPlan fd;
  hbh_engine* e = cs->e;
  const int t = cs->t;
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  // lane quads (four lanes per ack, one wave per SIMD) for latency; one lane per ack on affine
  // rows (two waves per SIMD, mixed additions) for throughput
  const bool lane = e->ack_impl == HBH_ACK_LANE || e->ack_impl == HBH_ACK_LANE_HORNER ||
                    (e->ack_impl == HBH_ACK_AUTO && nack >= HBH_ACK_LANE_MIN);
  rc = set_rows(cs, s, lane, nack, part_idx, xs, slot);
  if (rc) return rc;
  plan_drain(nack, slot, ys, t, lane && e->ack_fd && e->ack_impl != HBH_ACK_LANE_HORNER, fd, order);
  if (!fd.slot.empty() && ensure_fb16(e, s) != HBH_OK) {
    // the 16-bit comb (96 MiB + ~192 MiB of build scratch) could not be built: the Horner kernel
    // checks every ack (same verdicts), and this engine stops planning FD runs.  Nothing
    // of the plan is on the device yet, and the failed allocation's error is not left for a later launch.
    (void)hipGetLastError();
    e->fb16.release();
    e->ack_fd = false;
    static std::once_flag warned;
    std::call_once(warned, [] { fprintf(stderr, "hbbft_hip: no memory for the FD ack comb; Horner ack checks\n"); });
    plan_drain(nack, slot, ys, t, false, fd, order);
  }
  HBH_CHECK(e->in_b.ensure(nack * 12));
  HBH_CHECK(e->out_v.ensure(nack));
  uint32_t* d_ro = (uint32_t*)e->in_b.p;
  uint32_t* d_y = d_ro + nack;
  uint32_t* d_ord = d_y + nack;
  HBH_CHECK(h2d(s, d_ro, slot.data(), nack * 4));
  HBH_CHECK(h2d(s, d_y, ys, nack * 4));
  if (!order.empty()) HBH_CHECK(h2d(s, d_ord, order.data(), order.size() * 4));
  HBH_CHECK(upload(s, e->in_c, vals, nack * HBH_FR_BYTES));
  rc = ensure_fbtab(e, s);
  if (rc) return rc;
  const size_t nfd = fd.slot.size();
  uint32_t* d_fd = nullptr;
  if (nfd) {
    const size_t words = 4 * nfd + 2 * nack;
    HBH_CHECK(e->fd_meta.ensure(words * 4));
    HBH_CHECK(e->fd_e.ensure(fd.npts * hbl::fd_point_bytes()));
    d_fd = (uint32_t*)e->fd_meta.p;
    HBH_CHECK(h2d(s, d_fd, fd.slot.data(), nfd * 4));
    HBH_CHECK(h2d(s, d_fd + nfd, fd.y0.data(), nfd * 4));
    HBH_CHECK(h2d(s, d_fd + 2 * nfd, fd.off.data(), nfd * 4));
    HBH_CHECK(h2d(s, d_fd + 3 * nfd, fd.len.data(), nfd * 4));
    HBH_CHECK(h2d(s, d_fd + 4 * nfd, fd.epos.data(), nack * 4));
    HBH_CHECK(h2d(s, d_fd + 4 * nfd + nack, fd.fd_acks.data(), fd.fd_acks.size() * 4));
  }
  StageScope tm(e, s, HBH_STAGE_CURVE);
  if (nfd) {  // lane form only: the plan has FD rows under no other
    HBH_CHECK(hbl::bivar_fd(s, (int)nfd, t, cs->rows[1].p, d_fd, d_fd + nfd, d_fd + 2 * nfd, d_fd + 3 * nfd,
                            e->fd_e.p));
    HBH_CHECK(hbl::bivar_fd_check(s, (int)fd.fd_acks.size(), e->fd_e.p, d_fd + 4 * nfd, (const uint32_t*)e->in_c.p,
                                  e->fb16.p, d_fd + 4 * nfd + nack, (uint8_t*)e->out_v.p));
  }
  if (lane)
    HBH_CHECK(hbl::bivar_check(s, (int)order.size(), t, cs->rows[1].p, d_ro, d_y, (const uint32_t*)e->in_c.p,
                               e->fbtab.p, (uint8_t*)e->out_v.p, d_ord));
  else
    HBH_CHECK(hbl::bivar_check_quad(s, (int)nack, t, cs->rows[0].p, d_ro, d_y, (const uint32_t*)e->in_c.p,
                                    e->fbtab.p, (uint8_t*)e->out_v.p, d_ord));
  tm.stop();
  HBH_CHECK(download(s, verdicts, e->out_v, nack));
  return call.finish();
}

}  // extern "C"
