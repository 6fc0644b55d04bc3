// What the engine*.hip files share (host only, no kernels): the engine and its device buffers, the
// scope of one call, and the helpers that cross files (namespace hbe).  One file per call family:
//   engine.hip             last error, create / destroy, setters, profiling
//   engine_pairing.hip     the pairing checks, resident G2 sets
//   engine_hash.hip        hashing to G2 and the calls that hash on the device
//   engine_curve.hip       multiplications, interpolation, the split master check, rows, decoders
//   engine_commit_set.hip  device-resident commitment sets
//   engine_grouped.hip     grouped and batched random-combination checks
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/hbbft_hip.h"
#include "g2_slots.hpp"
#include "launch.hpp"

// host_hash.cpp, not part of the public ABI: seeds[i] = sha3_256 of message i (u == nullptr) or of
// hash_g1_g2's message for (u_i, message i)
extern "C" void hbh__hash_seeds(size_t n, const uint8_t* u, const uint8_t* data, const size_t* offsets, uint8_t* seeds);

namespace hbe {

// sets the calling thread's hbh_last_error (engine.hip) and returns code
int fail(int code, const std::string& msg);

#define HBH_CHECK(expr)                                                                           \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return hbe::fail(HBH_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));       \
  } while (0)

// A growable device buffer that owns its memory: freed with its owner (the engine's device current).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  ~DevBuf() { release(); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    size_t want = bytes + bytes / 4 + 4096;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Staging on a call's stream: upload grows the buffer first; h2d fills a part of a buffer that holds
// several arrays.
inline hipError_t h2d(hipStream_t s, void* dst, const void* src, size_t bytes) {
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
}
inline hipError_t upload(hipStream_t s, DevBuf& b, const void* src, size_t bytes) {
  const hipError_t err = b.ensure(bytes);
  return err == hipSuccess ? h2d(s, b.p, src, bytes) : err;
}
inline hipError_t download(hipStream_t s, void* dst, const DevBuf& b, size_t bytes) {
  return hipMemcpyAsync(dst, b.p, bytes, hipMemcpyDeviceToHost, s);
}

// Per-stage kernel timing (hbh_engine_set_profiling): HIP events recorded around each stage's
// launch on the stream it runs on, summed by hbh_engine_stage_time.
struct StageTimer {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[HBH_NUM_STAGES];
  hipEvent_t begin(hipStream_t s, int stage, bool on) {
    if (!on) return nullptr;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess) return nullptr;
    if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return nullptr; }
    (void)hipEventRecord(a, s);
    ev[stage].push_back({a, b});
    return b;
  }
  void end(hipStream_t s, hipEvent_t b) {
    if (b) (void)hipEventRecord(b, s);
  }
  void clear() {
    for (auto& v : ev) {
      for (auto& p : v) {
        (void)hipEventDestroy(p.first);
        (void)hipEventDestroy(p.second);
      }
      v.clear();
    }
  }
};

}  // namespace hbe

struct hbh_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  bool profiling = false;
  int impl = HBH_IMPL_AUTO;  // pairing implementation (hbh_engine_set_pairing_impl)
  int ack_impl = HBH_ACK_AUTO;  // Ack-check kernel of commitment sets (hbh_engine_set_ack_impl)
  int dec_impl = HBH_DEC_AUTO;  // point-decoding kernels (hbh_engine_set_decode_impl)
  int gsum_impl = HBH_GSUM_AUTO;  // group sums of the grouped share checks (hbh_engine_set_group_sum_impl)
  int gscalar_form = HBH_GSCALAR_INT128;  // how the grouped share checks read and draw scalars (hbh_engine_set_group_scalar_form)
  int hash_impl = HBH_HASH_AUTO;  // where the curve half of hash_g2 runs (hbh_engine_set_hash_impl)
  int hash_rounds = HBH_HASH_ROUNDS;  // sampler rounds of the device form (hbh_dbg_set_hash_rounds)
  int hash_form = HBH_HFORM_AUTO;  // lanes per message of the device form (hbh_engine_set_hash_form)
  hbe::StageTimer timer;
  // Completion of the last call's device work on whichever stream it ran.  Every call waits for it
  // on its own stream before touching the engine-owned workspaces, so a _dev call on a caller
  // stream can never overwrite tables another stream's kernels are still reading.
  hipEvent_t done = nullptr;
  // HBH_IMPL_PAIR device-pointer calls alternate between two table slots, each with its own
  // completion event: consecutive calls on different streams then overlap (one call's verify tail
  // with the next call's table walk and first waves) without sharing a workspace.  Every other
  // call waits for both slots and records both.
  hipEvent_t slot_done[2] = {nullptr, nullptr};
  int slot = 0;
  hbe::DevBuf ptab[2][2], pinf[2][2];
  // Device-pointer point decoding (hbh_g*_decompress_dev) alternates between two staging slots of
  // its own (wire words + flags), with its own completion events: a node's decode of one batch then
  // runs beside the previous batch's verify on another stream (the whole-node sign line, bench.py
  // --from-wire) instead of waiting for it.  It touches no other engine workspace.
  hipEvent_t wire_done[2] = {nullptr, nullptr};
  int wire_slot = 0;
  hbe::DevBuf wire_w[2], wire_f[2];
  // host staging of combine digits (kept alive until the call's stream synchronises)
  std::vector<uint64_t> h_digits;
  std::vector<int> h_status;
  // workspaces
  hbe::DevBuf work, status, fbtab, ipart;
  bool fbtab_ready = false;  // fixed-base comb table of g1 (built on first use)
  // staging for host-pointer entry points
  hbe::DevBuf in_p1, in_q1, in_i1, in_p2, in_q2, in_i2, out_v, in_a, in_b, in_c, in_d, out_x;
  // split master check (hbh_combine_verify_g2): a second stream runs the partial Miller loops while
  // the engine stream interpolates; partial Miller values in fval.  Created on the first split call:
  // HIP maps streams onto GPU_MAX_HW_QUEUES (4) hardware queues round-robin, and an idle extra stream
  // made at engine creation put the caller's two alternating verify streams on one queue
  // (sign bench: 23.3 instead of 21.1 ms per 65,536-check step)
  hipStream_t side = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  hbe::DevBuf fval, split_in, split_out, tree_cnt;
  uint8_t* h_stage = nullptr;  // pinned host staging of the split check (one upload, one download)
  size_t h_stage_cap = 0;
  bool split_check = true;  // HBH_SPLIT_CHECK=0 in the environment: interpolate, then verify (A/B)
  bool split_tree = true;   // HBH_SPLIT_TREE=0: a separate product + FE launch (wave_prod_fe) (A/B)
  // Ack checks of dense y runs by finite differences (hbl::bivar_fd); HBH_ACK_FD=0: Horner only (A/B)
  bool ack_fd = true;
  hbe::DevBuf fd_e, fd_meta, fb16;
  hbe::DevBuf hash_work, hash_state;  // the device form of hash_g2: worklists and sampled points, state bytes
  std::vector<uint8_t> g1k;  // G1K = [KCOF^-1] g1 (hbh_hash_bp_g1), made on first use (hbe::engine_g1k)
  bool fb16_ready = false;  // 16-bit comb of g1 (the FD ack check), built on first use
  size_t split_max = 0;  // HBH_SPLIT_MAX: most combines per call on the split check (0: the wave rule)
  // commitment sets created on this engine: hbh_engine_destroy frees their device memory and
  // detaches them, so a set destroyed after its engine never touches the freed engine
  std::unordered_set<hbh_commit_set*> sets;
  std::unordered_set<hbh_g2_set*> g2_sets;  // the same for resident G2 sets
};

// A device-resident set of prepared G2 points (hbh_g2_set_*): `slots.capacity()` slots in one
// allocation made at creation, so no base address ever moves -- the line tables (k_oct_prep's format,
// hbl::pair_table_bytes(1) per slot), then the affine ABI points (for the kernels that walk a side),
// then the infinity bytes.  Which slots are live is host state under the engine lock.
struct hbh_g2_set {
  hbh_engine* e = nullptr;
  G2Slots slots;
  void* mem = nullptr;
  void* lines = nullptr;
  void* q = nullptr;
  uint8_t* qinf = nullptr;
};

namespace hbe {

// One call on the engine, opened after the argument checks: holds the engine lock, makes the engine's
// device current, picks the stream (a _dev call's `stream`, NULL = the engine stream) and orders the
// call after the engine's earlier work.
//   GENERAL    waits for done and both table slots; records all three on close
//   PAIR_SLOT  takes the next table slot: waits for done and that slot's previous user; records the slot
//   WIRE_SLOT  the same with the staging slots of device-pointer point decoding
// finish() closes the call: it records the mode's events and, for a host-pointer call (sync), waits
// for the stream -- after the downloads the call queued.  A call that returns without finish(), as
// every failing one does, is closed the same way by the destructor, best effort: the next call on
// another stream still waits for this call's queued kernels, and no queued copy outlives the caller's
// buffers or the function's locals.
struct EngineCall {
  enum Mode { GENERAL, PAIR_SLOT, WIRE_SLOT };
  hbh_engine* const e;
  const bool sync;
  const Mode mode;
  std::lock_guard<std::mutex> lk;
  hipStream_t s = nullptr;
  int slot = 0;
  int rc;  // HBH_OK: the call is open
  bool closed = false;

  EngineCall(hbh_engine* e, void* stream, bool sync, Mode mode = GENERAL) : e(e), sync(sync), mode(mode), lk(e->mu) {
    rc = open(stream);
    closed = rc != HBH_OK;
  }
  ~EngineCall() {
    if (closed) return;
    hipEvent_t ev[3];
    for (int k = 0, n = events(ev); k < n; k++) (void)hipEventRecord(ev[k], s);
    if (sync) (void)hipStreamSynchronize(s);
  }
  EngineCall(const EngineCall&) = delete;
  EngineCall& operator=(const EngineCall&) = delete;

  int finish() {
    closed = true;
    hipEvent_t ev[3];
    hipError_t err = hipSuccess;
    for (int k = 0, n = events(ev); k < n && err == hipSuccess; k++) err = hipEventRecord(ev[k], s);
    if (err != hipSuccess) {
      if (sync) (void)hipStreamSynchronize(s);
      return fail(HBH_ERR_DEVICE, std::string("hipEventRecord: ") + hipGetErrorString(err));
    }
    if (sync) HBH_CHECK(hipStreamSynchronize(s));
    return HBH_OK;
  }

 private:
  int open(void* stream) {
    HBH_CHECK(hipSetDevice(e->device));
    s = stream ? (hipStream_t)stream : e->stream;
    HBH_CHECK(hipStreamWaitEvent(s, e->done, 0));
    if (mode == GENERAL) {
      HBH_CHECK(hipStreamWaitEvent(s, e->slot_done[0], 0));
      HBH_CHECK(hipStreamWaitEvent(s, e->slot_done[1], 0));
    } else if (mode == PAIR_SLOT) {
      slot = e->slot;
      e->slot ^= 1;
      HBH_CHECK(hipStreamWaitEvent(s, e->slot_done[slot], 0));
    } else {
      slot = e->wire_slot;
      e->wire_slot ^= 1;
      HBH_CHECK(hipStreamWaitEvent(s, e->wire_done[slot], 0));
    }
    return HBH_OK;
  }
  int events(hipEvent_t ev[3]) const {
    if (mode == PAIR_SLOT) return ev[0] = e->slot_done[slot], 1;
    if (mode == WIRE_SLOT) return ev[0] = e->wire_done[slot], 1;
    ev[0] = e->done;
    ev[1] = e->slot_done[0];
    ev[2] = e->slot_done[1];
    return 3;
  }
};

// A timed stage on stream s: the begin event now, the end event at stop() or on leaving the scope,
// so every exit records it (hbh_engine_stage_time reads both events of every pair).
struct StageScope {
  hbh_engine* const e;
  const hipStream_t s;
  hipEvent_t b;
  StageScope(hbh_engine* e, hipStream_t s, int stage) : e(e), s(s), b(e->timer.begin(s, stage, e->profiling)) {}
  ~StageScope() { stop(); }
  StageScope(const StageScope&) = delete;
  StageScope& operator=(const StageScope&) = delete;
  void stop() {
    e->timer.end(s, b);
    b = nullptr;
  }
};

inline int check_t(int t) { return (t < 0 || t > 4096) ? fail(HBH_ERR_ARG, "threshold out of range") : HBH_OK; }

// ---------------------------------------------------------------- engine_pairing.hip
// Which sides of a call come from a resident G2 set (hbh_g2_set): such a side arrives with its table
// (lines, qinf), its affine points (q) and nq = the set's capacity all filled in.
struct Resident {
  bool side[2] = {false, false};
};
int check_idx(const uint32_t* idx, size_t n, size_t table);
// e(P1_i, Q1[i1_i]) == e(P2_i, Q2[i2_i]) for device-resident inputs, one descriptor per side; a null P
// means the G1 generator for every check.  flags as hbl::pair_verify.
int run_pairing_sides(hbh_engine* e, hipStream_t s, size_t n, const hbl::PairSideDesc& d1, const hbl::PairSideDesc& d2,
                      const Resident& res, int flags, uint8_t* d_v, uint32_t* d_value = nullptr, int slot = 0);
// the same with both sides' G2 points given by the call (no resident set)
int run_pairing_dev(hbh_engine* e, hipStream_t s, size_t n, const void* d_p1, const void* d_q1, size_t nq1,
                    const uint32_t* d_i1, const void* d_p2, const void* d_q2, size_t nq2, const uint32_t* d_i2,
                    int flags, uint8_t* d_v, uint32_t* d_value = nullptr, int slot = 0);
// Host-pointer pairing-eq: stage to device, run, copy verdicts back, synchronise.  p1 / p2 ==
// nullptr: the G1 generator (nothing is uploaded for it).
// A side with a resident set (set1 / set2) names slots in its index array and brings no Q table.
int run_pairing_eq_host(hbh_engine* e, size_t n, const uint8_t* p1, const uint8_t* q1, size_t nq1, const uint32_t* i1,
                        const uint8_t* p2, const uint8_t* q2, size_t nq2, const uint32_t* i2, uint8_t* v,
                        hbh_g2_set* set1 = nullptr, hbh_g2_set* set2 = nullptr);
// Frees a set's device memory and detaches it from its engine (gs->e = nullptr).  Caller holds the engine
// lock with the engine's streams drained.
void release_g2_set_device(hbh_g2_set* gs);

// ---------------------------------------------------------------- engine_hash.hip
int check_msgs(size_t n, const uint8_t* data, const size_t* offsets);
// where the curve half of this call's hash runs (hbh_engine_set_hash_impl); takes the engine lock
bool hash_runs_on_device(hbh_engine* e, size_t n);
// out = G1K = [KCOF^-1] g1 (hbh_hash_bp_g1), made by the first call that needs it; takes the engine lock
int engine_g1k(hbh_engine* e, std::vector<uint8_t>& out);
// The host arrays of hash_to_table.  The caller fills `seeds` (hbh__hash_seeds) and declares the struct
// BEFORE its EngineCall: the call's destructor then drains the stream, and with it the queued patch
// copies that read `fixed`, before these vectors die on every exit path.
struct HashStage {
  std::vector<uint8_t> seeds, state, fixed;
};
// The device form of hash_g2 (FULL) / Q_bp (BP) of st.seeds into dst, a table of n G2 points that stays
// in HBM: seeds up, the kernels, the state bytes down (s is synchronised for them), the leftovers of the
// sampler rounds hashed on the host stage and patched into the table.
int hash_to_table(hbh_engine* e, hipStream_t s, size_t n, hbl::HashForm form, DevBuf& dst, HashStage& st);

// ---------------------------------------------------------------- engine_curve.hip, engine_commit_set.hip
// The g1 comb table, built on s the first time a call needs it.
int ensure_fbtab(hbh_engine* e, hipStream_t s);
// Frees a set's device memory and detaches it from its engine (cs->e = nullptr): every later call on
// the set fails with HBH_ERR_ARG, and hbh_commit_set_destroy only deletes the host object.  Caller
// holds the engine lock with the engine's streams drained.
void release_set_device(hbh_commit_set* cs);

}  // namespace hbe
