// Host side of the C ABI (include/hbbft_hip.h): device/stream/workspace management and batch
// orchestration of the HIP kernels behind launch.hpp.  No CPU fallback: every verdict comes from
// the GPU; without a usable device the calls fail with HBH_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/hbbft_hip.h"
#include "launch.hpp"
#include "interp_pair.hpp"
#include "wire.hpp"
// host arithmetic and planning (no HIP, tested on the CPU: tests/test_engine_host.py)
#include "host_fr.hpp"
#include "wire_host.hpp"
#include "ack_plan.hpp"
#include "g2_slots.hpp"
#include "constants.hpp"  // the field modulus, for hbh_g2_set_add's canonical-coordinate check

namespace {

thread_local std::string g_last_error = "";

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define HBH_CHECK(expr)                                                                           \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return fail(HBH_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));            \
  } while (0)

// A growable device buffer.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
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
hipError_t h2d(hipStream_t s, void* dst, const void* src, size_t bytes) {
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
}
hipError_t upload(hipStream_t s, DevBuf& b, const void* src, size_t bytes) {
  const hipError_t err = b.ensure(bytes);
  return err == hipSuccess ? h2d(s, b.p, src, bytes) : err;
}
hipError_t download(hipStream_t s, void* dst, const DevBuf& b, size_t bytes) {
  return hipMemcpyAsync(dst, b.p, bytes, hipMemcpyDeviceToHost, s);
}

}  // namespace

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

// split master check when the call has at most split_waves_max(t) one-pair Miller waves
// (ncomb x (t + 2)).  Crossover against interpolate-then-verify, interpolated linearly between the
// measured batch sizes of profiles/r03/split_sweep_auto.jsonl: t = 21 at ~45 combines (~1,046 waves;
// 32 combines split 2.81 vs 3.60 ms, 48 combines 3.80 vs 3.70 ms), t = 33 at ~38 combines (~1,340
// waves; 33 combines 4.26 vs 4.66 ms, 40 combines 4.75 vs 4.59 ms).  One wave cap cannot fit both
// (ADVICE r3), so the cap grows with t through those two points: 540 + 24 t.
// HBH_SPLIT_MAX=<combines> in the environment replaces the rule by a plain combine count (A/B).
inline size_t split_waves_max(int t) { return 540 + 24 * (size_t)t; }
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
  StageTimer timer;
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
  DevBuf ptab[2][2], pinf[2][2];
  // Device-pointer point decoding (hbh_g*_decompress_dev) alternates between two staging slots of
  // its own (wire words + flags), with its own completion events: a node's decode of one batch then
  // runs beside the previous batch's verify on another stream (the whole-node sign line, bench.py
  // --from-wire) instead of waiting for it.  It touches no other engine workspace.
  hipEvent_t wire_done[2] = {nullptr, nullptr};
  int wire_slot = 0;
  DevBuf wire_w[2], wire_f[2];
  // host staging of combine digits (kept alive until the call's stream synchronises)
  std::vector<uint64_t> h_digits;
  std::vector<int> h_status;
  // workspaces
  DevBuf work, status, fbtab, ipart;
  bool fbtab_ready = false;  // fixed-base comb table of g1 (built on first use)
  // staging for host-pointer entry points
  DevBuf in_p1, in_q1, in_i1, in_p2, in_q2, in_i2, out_v, in_a, in_b, in_c, in_d, out_x;
  // split master check (hbh_combine_verify_g2): a second stream runs the partial Miller loops while
  // the engine stream interpolates; partial Miller values in fval.  Created on the first split call:
  // HIP maps streams onto GPU_MAX_HW_QUEUES (4) hardware queues round-robin, and an idle extra stream
  // made at engine creation put the caller's two alternating verify streams on one queue
  // (sign bench: 23.3 instead of 21.1 ms per 65,536-check step)
  hipStream_t side = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  DevBuf fval, split_in, split_out, tree_cnt;
  uint8_t* h_stage = nullptr;  // pinned host staging of the split check (one upload, one download)
  size_t h_stage_cap = 0;
  bool split_check = true;  // HBH_SPLIT_CHECK=0 in the environment: interpolate, then verify (A/B)
  bool split_tree = true;   // HBH_SPLIT_TREE=0: a separate product + FE launch (wave_prod_fe) (A/B)
  // Ack checks of dense y runs by finite differences (hbl::bivar_fd); HBH_ACK_FD=0: Horner only (A/B)
  bool ack_fd = true;
  DevBuf fd_e, fd_meta, fb16;
  DevBuf hash_work, hash_state;  // the device form of hash_g2: worklists and sampled points, state bytes
  std::vector<uint8_t> g1k;  // G1K = [KCOF^-1] g1 (hbh_hash_bp_g1), made by the first hbh_verify_ciphertexts_uv
  bool fb16_ready = false;  // 16-bit comb of g1 (the FD ack check), built on first use
  size_t split_max = 0;  // HBH_SPLIT_MAX: most combines per call on the split check (0: the wave rule)
  // commitment sets created on this engine: hbh_engine_destroy frees their device memory and
  // detaches them, so a set destroyed after its engine never touches the freed engine
  std::unordered_set<hbh_commit_set*> sets;
  std::unordered_set<hbh_g2_set*> g2_sets;  // the same for resident G2 sets
};
void release_set_device(hbh_commit_set* cs);

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
void release_g2_set_device(hbh_g2_set* gs);

namespace {

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

int resolve_impl(const hbh_engine* e, size_t n) {
  if (e->impl != HBH_IMPL_AUTO) return e->impl;
  if (n >= HBH_AUTO_WAVEP_MIN && n <= HBH_AUTO_WAVEP_MAX) return HBH_IMPL_WAVEP;
  if (n <= HBH_AUTO_WAVE2_MAX) return HBH_IMPL_WAVE2;
  if (n <= HBH_AUTO_WAVE_MAX) return HBH_IMPL_WAVE;
  if (n <= HBH_AUTO_OCT_MAX) return HBH_IMPL_OCT;
  return n <= HBH_AUTO_QUAD_MAX ? HBH_IMPL_QUAD : HBH_IMPL_PAIR;
}

// the checks [off, n) of a side: per-check P and index map (or per-check Q when there is no map)
// advance by off; tables and shared Q tables stay
hbl::PairSideDesc offset_side(const hbl::PairSideDesc& d, size_t off) {
  hbl::PairSideDesc o = d;
  if (o.p) o.p = (const uint8_t*)o.p + off * HBH_G1_BYTES;
  if (o.idx) {
    o.idx += off;
  } else {  // identity map: Q is per check (nq == n, check_idx)
    o.q = (const uint8_t*)o.q + off * HBH_G2_BYTES;
    o.nq -= off;
  }
  return o;
}

#define HBH_WAVE_TT_MIN 1024  // WAVE calls that table two shared G2 sides (launch_pair)

// HBH_IMPL_WAVE2 (two waves per check) takes plain checks only; the split master check's modes
// (Miller-only, Jacobian P, one side) run on WAVE
hipError_t wave2_verify(hipStream_t s, int n, const hbl::PairSideDesc& a, const hbl::PairSideDesc& b, int flags,
                        uint8_t* v, uint32_t* val) {
  if (flags & ~(hbl::WAVE_NEG_P2 | hbl::WAVE_CONJ_VALUE)) return hbl::wave_verify(s, n, a, b, flags, v, val);
  return hbl::wave64_verify(s, n, a, b, flags, v, val);
}

// Which sides of a call come from a resident G2 set (hbh_g2_set): such a side arrives with its table
// (lines, qinf), its affine points (q) and nq = the set's capacity all filled in.
struct Resident {
  bool side[2] = {false, false};
};

// the pairing kernel of one implementation kind (not AUTO: verify_auto splits a call among these).
// The lane kernels read a resident side as a TABLE side.  The wave kernels (WAVE, WAVEP, WAVE2) read
// tables only when both sides have one (the TT program, at any n); otherwise this kernel walks a
// resident side from the set's affine point, as it walks a shared side of a small call.
hipError_t verify_kind(int kind, hipStream_t s, int n, const hbl::PairSideDesc& a0, const hbl::PairSideDesc& b0,
                       const Resident& res, int flags, uint8_t* v, uint32_t* val) {
  hbl::PairSideDesc a = a0, b = b0;
  const bool wave = kind == HBH_IMPL_WAVE2 || kind == HBH_IMPL_WAVE || kind == HBH_IMPL_WAVEP;
  if (wave && !(a.lines && b.lines)) {
    if (res.side[0]) a.lines = nullptr;
    if (res.side[1]) b.lines = nullptr;
  }
  if (kind == HBH_IMPL_WAVE2) return wave2_verify(s, n, a, b, flags, v, val);
  if (kind == HBH_IMPL_WAVE) return hbl::wave_verify(s, n, a, b, flags, v, val);
  if (kind == HBH_IMPL_WAVEP) return hbl::wavep_verify(s, n, a, b, flags, v, val);
  if (kind == HBH_IMPL_QUAD) return hbl::quad_verify(s, n, a, b, flags, v, val);
  if (kind == HBH_IMPL_OCT) return hbl::oct_verify(s, n, a, b, flags, v, val);
  return hbl::pair_verify(s, n, a, b, flags, v, val);
}

// HBH_IMPL_AUTO's launches for n checks on one stream (profiles/r04/c8, c19, c20 sweeps): whole
// rounds of HBH_AUTO_PAIR_ROUND checks (two lane-pair waves per SIMD) on PAIR, then the remainder by
// size -- above HBH_AUTO_SPLIT_HI one more (partial) PAIR round; above HBH_AUTO_SPLIT_LO PAIR on
// HBH_AUTO_SPLIT_LO checks (one wave per SIMD) first; what is left runs on WAVE up to
// HBH_AUTO_WAVE_MAX, OCT up to HBH_AUTO_OCT_MAX, QUAD up to HBH_AUTO_QUAD_MAX, PAIR (one wave per
// SIMD) above; a remainder in [HBH_AUTO_WAVEP_MIN, HBH_AUTO_WAVEP_MAX] runs on WAVEP first.  A partial
// lane-pair round costs as much as a full one once any SIMD needs a second wave (40,960 checks:
// PAIR alone 20.5-20.7 ms, PAIR + QUAD 19.4 ms, profiles/r04/c20_auto_split.txt).
hipError_t verify_auto(hipStream_t s, size_t n, const hbl::PairSideDesc& s1, const hbl::PairSideDesc& s2,
                       const Resident& res, int flags, uint8_t* d_v, uint32_t* d_value) {
  size_t off = 0;
  auto at = [&](size_t o, size_t cnt, int kind) -> hipError_t {
    const hbl::PairSideDesc a = o ? offset_side(s1, o) : s1, b = o ? offset_side(s2, o) : s2;
    uint8_t* v = d_v ? d_v + o : nullptr;
    uint32_t* val = d_value ? d_value + o * 144 : nullptr;
    return verify_kind(kind, s, (int)cnt, a, b, res, flags, v, val);
  };
  if (n > HBH_AUTO_SPLIT_HI) {  // whole two-wave lane-pair rounds
    off = (n / HBH_AUTO_PAIR_ROUND) * HBH_AUTO_PAIR_ROUND;
    if (off) {
      const hipError_t r = at(0, off, HBH_IMPL_PAIR);
      if (r != hipSuccess) return r;
    }
  }
  size_t rem = n - off;
  if (rem == 0) return hipSuccess;
  if (rem > HBH_AUTO_SPLIT_HI) return at(off, rem, HBH_IMPL_PAIR);  // one partial two-wave round
  if (rem > HBH_AUTO_SPLIT_LO) {  // one lane-pair wave per SIMD, then the rest by size
    const hipError_t r = at(off, HBH_AUTO_SPLIT_LO, HBH_IMPL_PAIR);
    if (r != hipSuccess) return r;
    off += HBH_AUTO_SPLIT_LO;
    rem -= HBH_AUTO_SPLIT_LO;
  }
  if (rem >= HBH_AUTO_WAVEP_MIN && rem <= HBH_AUTO_WAVEP_MAX) return at(off, rem, HBH_IMPL_WAVEP);
  if (rem <= HBH_AUTO_WAVE2_MAX) return at(off, rem, HBH_IMPL_WAVE2);
  if (rem <= HBH_AUTO_WAVE_MAX) return at(off, rem, HBH_IMPL_WAVE);
  if (rem <= HBH_AUTO_OCT_MAX) return at(off, rem, HBH_IMPL_OCT);
  if (rem <= HBH_AUTO_QUAD_MAX) return at(off, rem, HBH_IMPL_QUAD);
  return at(off, rem, HBH_IMPL_PAIR);
}

// HBH_IMPL_PAIR: a G2 side shared through an index map by at least 4 checks per point gets a line
// table (k_oct_prep); every other side is walked inside the verify kernel.  A resident side (res)
// brings its table along: nothing is built for it.
int launch_pair(hbh_engine* e, hipStream_t s, int impl, size_t n, const hbl::PairSideDesc& d1,
                const hbl::PairSideDesc& d2, const Resident& res, int flags, uint8_t* d_v, uint32_t* d_value,
                int slot) {
  hbl::PairSideDesc sd[2] = {d1, d2};
  DevBuf* tab[2] = {&e->ptab[slot][0], &e->ptab[slot][1]};
  DevBuf* inf[2] = {&e->pinf[slot][0], &e->pinf[slot][1]};
  const bool tab_ok[2] = {res.side[0] || (sd[0].idx && sd[0].nq * 4 <= n), res.side[1] || (sd[1].idx && sd[1].nq * 4 <= n)};
  for (int k = 0; k < 2; k++) {
    // WAVE2 walks every side: a table costs a serial 68-step walk (k_oct_prep, ~0.5 ms) before the
    // first check.  WAVE tables both sides of a call of >= HBH_WAVE_TT_MIN checks when both are
    // shared (decryption shares: H_uv and W per ciphertext): its TT program takes 138 Miller stages
    // where walking both sides takes 211 (round 6); one walked side gains nothing (TW: 210).  WAVEP
    // runs the same programs and follows the same rule.  Two resident sides cost no walk, so the wave
    // kernels take TT for them at any n (verify_kind).
    if (res.side[k] || !tab_ok[k] || impl == HBH_IMPL_WAVE2) continue;
    if ((impl == HBH_IMPL_WAVE || impl == HBH_IMPL_WAVEP) && !(tab_ok[0] && tab_ok[1] && n >= HBH_WAVE_TT_MIN)) continue;
    HBH_CHECK(tab[k]->ensure(hbl::pair_table_bytes(sd[k].nq)));
    HBH_CHECK(inf[k]->ensure(sd[k].nq));
    StageScope tm(e, s, HBH_STAGE_PREPARE);
    HBH_CHECK(hbl::oct_prep(s, (int)sd[k].nq, sd[k].q, tab[k]->p, (uint8_t*)inf[k]->p));
    sd[k].lines = tab[k]->p;
    sd[k].qinf = (const uint8_t*)inf[k]->p;
  }
  StageScope tm(e, s, HBH_STAGE_PAIRING);
  if (e->impl == HBH_IMPL_AUTO)
    HBH_CHECK(verify_auto(s, n, sd[0], sd[1], res, flags, d_v, d_value));
  else
    HBH_CHECK(verify_kind(impl, s, (int)n, sd[0], sd[1], res, flags, d_v, d_value));
  return HBH_OK;
}

// e(P1_i, Q1[i1_i]) == e(P2_i, Q2[i2_i]) for device-resident inputs, one descriptor per side; a null P
// means the G1 generator for every check.  flags as hbl::pair_verify.
int run_pairing_sides(hbh_engine* e, hipStream_t s, size_t n, const hbl::PairSideDesc& d1, const hbl::PairSideDesc& d2,
                      const Resident& res, int flags, uint8_t* d_v, uint32_t* d_value = nullptr, int slot = 0) {
  if (n == 0) return HBH_OK;
  if (n > (size_t)1 << 30 || d1.nq > (size_t)1 << 30 || d2.nq > (size_t)1 << 30) return fail(HBH_ERR_ARG, "batch too large");
  return launch_pair(e, s, resolve_impl(e, n), n, d1, d2, res, flags, d_v, d_value, slot);
}

// the same with both sides' G2 points given by the call (no resident set)
int run_pairing_dev(hbh_engine* e, hipStream_t s, size_t n, const void* d_p1, const void* d_q1, size_t nq1,
                    const uint32_t* d_i1, const void* d_p2, const void* d_q2, size_t nq2, const uint32_t* d_i2,
                    int flags, uint8_t* d_v, uint32_t* d_value = nullptr, int slot = 0) {
  return run_pairing_sides(e, s, n, {d_p1, d_q1, nullptr, nullptr, d_i1, nq1}, {d_p2, d_q2, nullptr, nullptr, d_i2, nq2},
                           Resident(), flags, d_v, d_value, slot);
}

// one side of a call from a resident set: its table, affine points and infinity bytes, nq = capacity
hbl::PairSideDesc set_side(const hbh_g2_set* gs, const void* d_p, const uint32_t* d_idx) {
  return {d_p, gs->q, gs->lines, gs->qinf, d_idx, gs->slots.capacity()};
}

// a set named by a _set call: attached, and to this engine
int check_g2_set(const hbh_engine* e, const hbh_g2_set* gs) {
  if (!gs->e) return fail(HBH_ERR_ARG, "G2 set detached: its engine was destroyed");
  if (gs->e != e) return fail(HBH_ERR_ARG, "G2 set belongs to another engine");
  return HBH_OK;
}

int check_idx(const uint32_t* idx, size_t n, size_t table) {
  if (!idx) return table == n ? HBH_OK : fail(HBH_ERR_ARG, "identity index map requires table size == n");
  for (size_t i = 0; i < n; i++)
    if (idx[i] >= table) return fail(HBH_ERR_ARG, "index out of range");
  return HBH_OK;
}

// Host-pointer pairing-eq: stage to device, run, copy verdicts back, synchronise.  p1 / p2 ==
// nullptr: the G1 generator (nothing is uploaded for it).
// A side with a resident set (set1 / set2) names slots in its index array and brings no Q table.
int run_pairing_eq_host(hbh_engine* e, size_t n, const uint8_t* p1, const uint8_t* q1, size_t nq1, const uint32_t* i1,
                        const uint8_t* p2, const uint8_t* q2, size_t nq2, const uint32_t* i2, uint8_t* v,
                        hbh_g2_set* set1 = nullptr, hbh_g2_set* set2 = nullptr) {
  hbh_g2_set* const set[2] = {set1, set2};
  const uint8_t* const q[2] = {q1, q2};
  const size_t nq[2] = {nq1, nq2};
  const uint32_t* const idx[2] = {i1, i2};
  for (int k = 0; k < 2; k++) {
    if (!set[k]) continue;
    const int rc = check_g2_set(e, set[k]);
    if (rc) return rc;
    if (q[k] || nq[k]) return fail(HBH_ERR_ARG, "a side with a G2 set takes no Q table");
  }
  if (n == 0) return HBH_OK;
  for (int k = 0; k < 2; k++)
    if (set[k] ? !idx[k] : !q[k]) return fail(HBH_ERR_ARG, "null pointer");
  if (!v) return fail(HBH_ERR_ARG, "null pointer");
  for (int k = 0; k < 2; k++) {
    if (set[k]) continue;
    const int rc = check_idx(idx[k], n, nq[k]);
    if (rc) return rc;
  }
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  for (int k = 0; k < 2; k++)  // under the engine lock: no add or release runs beside this
    for (size_t i = 0; set[k] && i < n; i++)
      if (!set[k]->slots.live(idx[k][i])) return fail(HBH_ERR_ARG, "G2 set slot is not live");
  hipStream_t s = call.s;
  if (p1) HBH_CHECK(upload(s, e->in_p1, p1, n * HBH_G1_BYTES));
  if (p2) HBH_CHECK(upload(s, e->in_p2, p2, n * HBH_G1_BYTES));
  if (!set1) HBH_CHECK(upload(s, e->in_q1, q1, nq1 * HBH_G2_BYTES));
  if (!set2) HBH_CHECK(upload(s, e->in_q2, q2, nq2 * HBH_G2_BYTES));
  HBH_CHECK(e->out_v.ensure(n));
  if (i1) HBH_CHECK(upload(s, e->in_i1, i1, n * 4));
  if (i2) HBH_CHECK(upload(s, e->in_i2, i2, n * 4));
  const void* d_p[2] = {p1 ? e->in_p1.p : nullptr, p2 ? e->in_p2.p : nullptr};
  const uint32_t* d_i[2] = {i1 ? (const uint32_t*)e->in_i1.p : nullptr, i2 ? (const uint32_t*)e->in_i2.p : nullptr};
  const void* d_q[2] = {e->in_q1.p, e->in_q2.p};
  hbl::PairSideDesc sd[2];
  Resident res;
  for (int k = 0; k < 2; k++) {
    res.side[k] = set[k] != nullptr;
    sd[k] = set[k] ? set_side(set[k], d_p[k], d_i[k]) : hbl::PairSideDesc{d_p[k], d_q[k], nullptr, nullptr, d_i[k], nq[k]};
  }
  const int rc = run_pairing_sides(e, s, n, sd[0], sd[1], res, 1, (uint8_t*)e->out_v.p);
  if (rc) return rc;
  HBH_CHECK(download(s, v, e->out_v, n));
  return call.finish();
}

}  // namespace

extern "C" {

const char* hbh_last_error(void) { return g_last_error.c_str(); }

// Not part of the public ABI: lets pool.cpp report a shard's failure on the calling thread.
extern "C" void hbh__set_error(const char* msg) { g_last_error = msg ? msg : ""; }

int hbh_device_count(int* out) {
  if (!out) return fail(HBH_ERR_ARG, "null pointer");
  int c = 0;
  hipError_t err = hipGetDeviceCount(&c);
  if (err != hipSuccess) {
    *out = 0;
    return fail(HBH_ERR_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(err));
  }
  *out = c;
  return HBH_OK;
}

int hbh_engine_create(int device, hbh_engine** out) {
  if (!out) return fail(HBH_ERR_ARG, "null pointer");
  *out = nullptr;
  int count = 0;
  HBH_CHECK(hipGetDeviceCount(&count));
  if (device < 0 || device >= count) return fail(HBH_ERR_ARG, "device ordinal out of range");
  HBH_CHECK(hipSetDevice(device));
  hbh_engine* e = new hbh_engine();
  e->device = device;
  if (const char* v = std::getenv("HBH_SPLIT_CHECK")) e->split_check = std::atoi(v) != 0;
  if (const char* v = std::getenv("HBH_SPLIT_TREE")) e->split_tree = std::atoi(v) != 0;
  if (const char* v = std::getenv("HBH_ACK_FD")) e->ack_fd = std::atoi(v) != 0;
  if (const char* v = std::getenv("HBH_SPLIT_MAX")) e->split_max = (size_t)std::max(0, std::atoi(v));
  hipError_t err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&e->done, hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventRecord(e->done, e->stream);
  for (int k = 0; k < 2 && err == hipSuccess; k++) {
    err = hipEventCreateWithFlags(&e->slot_done[k], hipEventDisableTiming);
    if (err == hipSuccess) err = hipEventRecord(e->slot_done[k], e->stream);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&e->wire_done[k], hipEventDisableTiming);
    if (err == hipSuccess) err = hipEventRecord(e->wire_done[k], e->stream);
  }
  if (err != hipSuccess) {
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return fail(HBH_ERR_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(err));
  }
  *out = e;
  return HBH_OK;
}

int hbh_engine_destroy(hbh_engine* e) {
  if (!e) return HBH_OK;
  (void)hipSetDevice(e->device);
  {
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipEventSynchronize(e->done);
    (void)hipStreamSynchronize(e->stream);
    for (hbh_commit_set* cs : e->sets) release_set_device(cs);  // detaches cs from e
    e->sets.clear();
    for (hipEvent_t ev : e->slot_done)  // _set_dev calls on caller streams read the sets' tables
      if (ev && !e->g2_sets.empty()) (void)hipEventSynchronize(ev);
    for (hbh_g2_set* gs : e->g2_sets) release_g2_set_device(gs);
    e->g2_sets.clear();
  }
  (void)hipEventSynchronize(e->done);
  for (hipEvent_t ev : e->slot_done)
    if (ev) (void)hipEventSynchronize(ev);
  for (hipEvent_t ev : e->wire_done)
    if (ev) (void)hipEventSynchronize(ev);
  (void)hipStreamSynchronize(e->stream);
  if (e->side) (void)hipStreamSynchronize(e->side);
  e->timer.clear();
  for (DevBuf* b : {&e->work, &e->status, &e->fbtab, &e->ipart, &e->in_p1, &e->in_q1, &e->in_i1, &e->in_p2, &e->in_q2, &e->in_i2, &e->out_v,
                    &e->in_a, &e->in_b, &e->in_c, &e->in_d, &e->out_x, &e->ptab[0][0], &e->ptab[0][1], &e->ptab[1][0],
                    &e->ptab[1][1], &e->pinf[0][0], &e->pinf[0][1], &e->pinf[1][0], &e->pinf[1][1], &e->fval, &e->split_in,
                    &e->split_out, &e->tree_cnt, &e->fd_e, &e->fd_meta, &e->fb16, &e->wire_w[0], &e->wire_w[1],
                    &e->wire_f[0], &e->wire_f[1], &e->hash_work, &e->hash_state})
    b->release();
  if (e->h_stage) (void)hipHostFree(e->h_stage);
  (void)hipEventDestroy(e->done);
  if (e->side) {
    (void)hipEventDestroy(e->fork);
    (void)hipEventDestroy(e->join);
    (void)hipStreamDestroy(e->side);
  }
  for (hipEvent_t ev : e->slot_done)
    if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : e->wire_done)
    if (ev) (void)hipEventDestroy(ev);
  (void)hipStreamDestroy(e->stream);
  delete e;
  return HBH_OK;
}

int hbh_verify_pairing_eq(hbh_engine* e, size_t n, const uint8_t* p1, const uint8_t* q1, size_t nq1,
                          const uint32_t* i1, const uint8_t* p2, const uint8_t* q2, size_t nq2, const uint32_t* i2,
                          uint8_t* v) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n && (!p1 || !p2)) return fail(HBH_ERR_ARG, "null pointer");
  return run_pairing_eq_host(e, n, p1, q1, nq1, i1, p2, q2, nq2, i2, v);
}

int hbh_verify_pairing_eq_dev(hbh_engine* e, void* stream, size_t n, const void* d_p1, const void* d_q1, size_t nq1,
                              const uint32_t* d_i1, const void* d_p2, const void* d_q2, size_t nq2,
                              const uint32_t* d_i2, uint8_t* d_v) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n && (!d_q1 || !d_q2 || !d_v)) return fail(HBH_ERR_ARG, "null pointer");
  if ((!d_i1 && nq1 != n) || (!d_i2 && nq2 != n)) return fail(HBH_ERR_ARG, "identity index map requires table size == n");
  if (n == 0) return HBH_OK;
  // table slot of its own: wait for the last general call and for this slot's previous user only
  EngineCall call(e, stream, false, EngineCall::PAIR_SLOT);
  if (call.rc) return call.rc;
  int rc = run_pairing_dev(e, call.s, n, d_p1, d_q1, nq1, d_i1, d_p2, d_q2, nq2, d_i2, 1, d_v, nullptr, call.slot);
  if (rc) return rc;
  return call.finish();
}

int hbh_verify_sig_shares(hbh_engine* e, size_t n, const uint8_t* pks, const uint8_t* sigs, const uint8_t* hashes,
                          size_t ndocs, const uint32_t* doc_idx, uint8_t* v) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n == 0) return HBH_OK;
  if (!pks || !sigs) return fail(HBH_ERR_ARG, "null pointer");
  return run_pairing_eq_host(e, n, pks, hashes, ndocs, doc_idx, nullptr, sigs, n, nullptr, v);
}

int hbh_verify_dec_shares(hbh_engine* e, size_t n, const uint8_t* shares, const uint8_t* pks, const uint8_t* huv,
                          const uint8_t* w, size_t ncts, const uint32_t* ct_idx, uint8_t* v) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n && (!shares || !pks)) return fail(HBH_ERR_ARG, "null pointer");
  return run_pairing_eq_host(e, n, shares, huv, ncts, ct_idx, pks, w, ncts, ct_idx, v);
}

int hbh_verify_ciphertexts(hbh_engine* e, size_t n, const uint8_t* u, const uint8_t* w, const uint8_t* huv,
                           uint8_t* v) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n == 0) return HBH_OK;
  if (!u) return fail(HBH_ERR_ARG, "null pointer");
  return run_pairing_eq_host(e, n, nullptr, w, n, nullptr, u, huv, n, nullptr, v);
}

int hbh_dbg_pairing(hbh_engine* e, size_t n, const uint8_t* p, const uint8_t* q, uint8_t* out) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n == 0) return HBH_OK;
  if (!p || !q || !out) return fail(HBH_ERR_ARG, "null pointer");
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  HBH_CHECK(upload(s, e->in_p1, p, n * HBH_G1_BYTES));
  HBH_CHECK(upload(s, e->in_q1, q, n * HBH_G2_BYTES));
  HBH_CHECK(e->out_v.ensure(n * 576));
  HBH_CHECK(e->in_p2.ensure(n * HBH_G1_BYTES));
  HBH_CHECK(hipMemsetAsync(e->in_p2.p, 0, n * HBH_G1_BYTES, s));  // second pair inactive (P2 = O)
  int rc = run_pairing_dev(e, s, n, e->in_p1.p, e->in_q1.p, n, nullptr, e->in_p2.p, e->in_q1.p, n, nullptr, 2, nullptr,
                           (uint32_t*)e->out_v.p);
  if (rc) return rc;
  HBH_CHECK(download(s, out, e->out_v, n * 576));
  return call.finish();
}

int hbh_engine_set_pairing_impl(hbh_engine* e, int impl) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (impl != HBH_IMPL_PAIR && impl != HBH_IMPL_AUTO && impl != HBH_IMPL_WAVE && impl != HBH_IMPL_QUAD &&
      impl != HBH_IMPL_OCT && impl != HBH_IMPL_WAVE2 && impl != HBH_IMPL_WAVEP)
    return fail(HBH_ERR_ARG, "unknown or retired pairing implementation");
  std::lock_guard<std::mutex> lk(e->mu);
  e->impl = impl;
  return HBH_OK;
}

int hbh_engine_set_ack_impl(hbh_engine* e, int impl) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (impl != HBH_ACK_AUTO && impl != HBH_ACK_QUAD && impl != HBH_ACK_LANE && impl != HBH_ACK_LANE_HORNER)
    return fail(HBH_ERR_ARG, "unknown Ack-check implementation");
  std::lock_guard<std::mutex> lk(e->mu);
  e->ack_impl = impl;
  return HBH_OK;
}

int hbh_engine_set_decode_impl(hbh_engine* e, int impl) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (impl != HBH_DEC_AUTO && impl != HBH_DEC_LANE && impl != HBH_DEC_SPLIT)
    return fail(HBH_ERR_ARG, "unknown point-decoding implementation");
  std::lock_guard<std::mutex> lk(e->mu);
  e->dec_impl = impl;
  return HBH_OK;
}

int hbh_engine_set_group_sum_impl(hbh_engine* e, int impl) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (impl != HBH_GSUM_AUTO && impl != HBH_GSUM_CHAIN && impl != HBH_GSUM_BUCKET)
    return fail(HBH_ERR_ARG, "unknown group-sum implementation");
  std::lock_guard<std::mutex> lk(e->mu);
  e->gsum_impl = impl;
  return HBH_OK;
}

int hbh_engine_set_group_scalar_form(hbh_engine* e, int form) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (form != HBH_GSCALAR_INT128 && form != HBH_GSCALAR_DIGITS) return fail(HBH_ERR_ARG, "unknown group scalar form");
  std::lock_guard<std::mutex> lk(e->mu);
  e->gscalar_form = form;
  return HBH_OK;
}

int hbh_engine_set_hash_impl(hbh_engine* e, int impl) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (impl != HBH_HASH_AUTO && impl != HBH_HASH_HOST && impl != HBH_HASH_DEVICE)
    return fail(HBH_ERR_ARG, "unknown hash-to-G2 implementation");
  std::lock_guard<std::mutex> lk(e->mu);
  e->hash_impl = impl;
  return HBH_OK;
}

int hbh_engine_set_hash_form(hbh_engine* e, int form) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (form != HBH_HFORM_AUTO && form != HBH_HFORM_LANE && form != HBH_HFORM_QUAD)
    return fail(HBH_ERR_ARG, "unknown hash-to-G2 device form");
  std::lock_guard<std::mutex> lk(e->mu);
  e->hash_form = form;
  return HBH_OK;
}

int hbh_dbg_set_hash_rounds(hbh_engine* e, int rounds) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (rounds < 0 || rounds > 1024) return fail(HBH_ERR_ARG, "hash rounds out of range");
  std::lock_guard<std::mutex> lk(e->mu);
  e->hash_rounds = rounds ? rounds : HBH_HASH_ROUNDS;
  return HBH_OK;
}

int hbh_engine_set_profiling(hbh_engine* e, int on) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  std::lock_guard<std::mutex> lk(e->mu);
  HBH_CHECK(hipSetDevice(e->device));
  HBH_CHECK(hipStreamSynchronize(e->stream));
  e->timer.clear();
  e->profiling = on != 0;
  return HBH_OK;
}

int hbh_engine_stage_time(hbh_engine* e, int stage, double* total_ms, int* launches) {
  if (!e || !total_ms || !launches || stage < 0 || stage >= HBH_NUM_STAGES || stage == 3)  // 3: not assigned
    return fail(HBH_ERR_ARG, "bad argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HBH_CHECK(hipSetDevice(e->device));
  double sum = 0;
  for (auto& p : e->timer.ev[stage]) {
    HBH_CHECK(hipEventSynchronize(p.second));
    float ms = 0;
    HBH_CHECK(hipEventElapsedTime(&ms, p.first, p.second));
    sum += ms;
  }
  *total_ms = sum;
  *launches = (int)e->timer.ev[stage].size();
  return HBH_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- hashing to G2
// host_hash.cpp, not part of the public ABI: seeds[i] = sha3_256 of message i (u == nullptr) or of
// hash_g1_g2's message for (u_i, message i); the curve half of hash_g2 from one seed.
extern "C" void hbh__hash_seeds(size_t n, const uint8_t* u, const uint8_t* data, const size_t* offsets, uint8_t* seeds);
extern "C" void hbh__hash_g2_seeds(size_t n, const uint32_t* which, const uint8_t* seeds, uint8_t* out);
// the same for the Q form: out[which[k]] = Q_bp of that seed (hbh_hash_g1_g2_bp's bytes)
extern "C" void hbh__hash_g2_bp_seeds(size_t n, const uint32_t* which, const uint8_t* seeds, uint8_t* out);

namespace {

int check_msgs(size_t n, const uint8_t* data, const size_t* offsets) {
  if (!offsets || (!data && offsets[n] != 0)) return fail(HBH_ERR_ARG, "null pointer");
  for (size_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i]) return fail(HBH_ERR_ARG, "offsets not ascending");
  if (n > (size_t)1 << 26) return fail(HBH_ERR_ARG, "batch too large");
  return HBH_OK;
}

bool hash_on_device(const hbh_engine* e, size_t n) {
  if (e->hash_impl != HBH_HASH_AUTO) return e->hash_impl == HBH_HASH_DEVICE;
  return HBH_AUTO_HASH_DEVICE_MIN != 0 && n >= HBH_AUTO_HASH_DEVICE_MIN;
}

// which device form a run of n messages takes (hbh_engine_set_hash_form); same bytes from either
bool hash_quad(const hbh_engine* e, size_t n) {
  if (e->hash_form != HBH_HFORM_AUTO) return e->hash_form == HBH_HFORM_QUAD;
  return HBH_AUTO_HASH_QUAD_MAX != 0 && n <= HBH_AUTO_HASH_QUAD_MAX;
}

// the kernels of the device form on s: d_seeds -> d_out, one state byte per message in e->hash_state
int launch_hash(hbh_engine* e, hipStream_t s, size_t n, const uint8_t* d_seeds, void* d_out,
                hbl::HashForm form = hbl::HASH_FORM_FULL) {
  HBH_CHECK(e->hash_work.ensure(hbl::hash_work_bytes(n, e->hash_rounds)));
  HBH_CHECK(e->hash_state.ensure(n));
  StageScope tm(e, s, HBH_STAGE_HASH);
  const auto run = hash_quad(e, n) ? hbl::hash_g2_quad : hbl::hash_g2;
  HBH_CHECK(run(s, (int)n, e->hash_rounds, d_seeds, e->hash_work.p, (uint8_t*)e->hash_state.p, d_out, form));
  return HBH_OK;
}

// indices of the messages the device left unresolved (more candidates than rounds)
std::vector<uint32_t> hash_leftovers(const std::vector<uint8_t>& state) {
  std::vector<uint32_t> left;
  for (size_t i = 0; i < state.size(); i++)
    if (state[i] != hbl::HASH_DONE) left.push_back((uint32_t)i);
  return left;
}

// the device form for host buffers: seeds up, the points (FULL: hash_g2's, BP: Q_bp) down, the leftovers of
// the sampler rounds hashed on the host stage
int hash_seeds_device(hbh_engine* e, size_t n, const std::vector<uint8_t>& seeds, hbl::HashForm form, uint8_t* out) {
  std::vector<uint8_t> state(n);
  {
    EngineCall call(e, nullptr, true);
    if (call.rc) return call.rc;
    hipStream_t s = call.s;
    HBH_CHECK(upload(s, e->in_a, seeds.data(), n * 32));
    HBH_CHECK(e->out_x.ensure(n * HBH_G2_BYTES));
    int rc = launch_hash(e, s, n, (const uint8_t*)e->in_a.p, e->out_x.p, form);
    if (rc) return rc;
    HBH_CHECK(download(s, out, e->out_x, n * HBH_G2_BYTES));
    HBH_CHECK(download(s, state.data(), e->hash_state, n));
    rc = call.finish();
    if (rc) return rc;
  }
  const std::vector<uint32_t> left = hash_leftovers(state);
  if (!left.empty())
    (form == hbl::HASH_FORM_BP ? hbh__hash_g2_bp_seeds : hbh__hash_g2_seeds)(left.size(), left.data(), seeds.data(), out);
  return HBH_OK;
}

// hbh_engine_hash_g2 / hbh_engine_hash_g1_g2 (u != nullptr) / hbh_engine_hash_g1_g2_bp (u != nullptr, BP)
int run_hash_host(hbh_engine* e, size_t n, const uint8_t* u, const uint8_t* data, const size_t* offsets, uint8_t* out,
                  hbl::HashForm form = hbl::HASH_FORM_FULL) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n == 0) return HBH_OK;
  if (!out) return fail(HBH_ERR_ARG, "null pointer");
  int rc = check_msgs(n, data, offsets);
  if (rc) return rc;
  bool device;
  {
    std::lock_guard<std::mutex> lk(e->mu);
    device = hash_on_device(e, n);
  }
  if (!device) {
    if (form == hbl::HASH_FORM_BP)
      rc = hbh_hash_g1_g2_bp(n, u, data, offsets, out, 0);
    else
      rc = u ? hbh_hash_g1_g2(n, u, data, offsets, out, 0) : hbh_hash_g2(n, data, offsets, out, 0);
    return rc ? fail(rc, hbh_host_last_error()) : HBH_OK;
  }
  std::vector<uint8_t> seeds(n * 32);
  hbh__hash_seeds(n, u, data, offsets, seeds.data());
  return hash_seeds_device(e, n, seeds, form, out);
}

}  // namespace

extern "C" {

int hbh_engine_hash_g2(hbh_engine* e, size_t n, const uint8_t* data, const size_t* offsets, uint8_t* out) {
  return run_hash_host(e, n, nullptr, data, offsets, out);
}

int hbh_engine_hash_g1_g2(hbh_engine* e, size_t n, const uint8_t* u, const uint8_t* data, const size_t* offsets,
                          uint8_t* out) {
  if (n && !u) return fail(HBH_ERR_ARG, "null pointer");
  return run_hash_host(e, n, u, data, offsets, out);
}

int hbh_engine_hash_g1_g2_bp(hbh_engine* e, size_t n, const uint8_t* u, const uint8_t* data, const size_t* offsets,
                             uint8_t* out) {
  if (n && !u) return fail(HBH_ERR_ARG, "null pointer");
  return run_hash_host(e, n, u, data, offsets, out, hbl::HASH_FORM_BP);
}

int hbh_hash_g2_dev(hbh_engine* e, void* stream, size_t n, const uint8_t* d_seeds, void* d_out) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n == 0) return HBH_OK;
  if (!d_seeds || !d_out) return fail(HBH_ERR_ARG, "null pointer");
  if (n > (size_t)1 << 26) return fail(HBH_ERR_ARG, "batch too large");
  EngineCall call(e, stream, false);
  if (call.rc) return call.rc;
  const int rc = launch_hash(e, call.s, n, d_seeds, d_out);
  if (rc) return rc;
  return call.finish();
}

int hbh_verify_signatures(hbh_engine* e, size_t n, const uint8_t* pks, const uint8_t* sigs, const uint8_t* data,
                          const size_t* offsets, uint8_t* v) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n == 0) return HBH_OK;
  if (!pks || !sigs || !v) return fail(HBH_ERR_ARG, "null pointer");
  int rc = check_msgs(n, data, offsets);
  if (rc) return rc;
  bool device;
  {
    std::lock_guard<std::mutex> lk(e->mu);
    device = hash_on_device(e, n);
  }
  if (!device) {
    std::vector<uint8_t> h(n * HBH_G2_BYTES);
    rc = hbh_hash_g2(n, data, offsets, h.data(), 0);
    if (rc) return fail(rc, hbh_host_last_error());
    return run_pairing_eq_host(e, n, pks, h.data(), n, nullptr, nullptr, sigs, n, nullptr, v);
  }
  std::vector<uint8_t> seeds(n * 32), state(n), fixed;
  hbh__hash_seeds(n, nullptr, data, offsets, seeds.data());
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  // the hashes are written straight into the Q1 staging buffer of the pairing path and stay in HBM
  HBH_CHECK(upload(s, e->in_a, seeds.data(), n * 32));
  HBH_CHECK(e->in_q1.ensure(n * HBH_G2_BYTES));
  rc = launch_hash(e, s, n, (const uint8_t*)e->in_a.p, e->in_q1.p);
  if (rc) return rc;
  HBH_CHECK(upload(s, e->in_p1, pks, n * HBH_G1_BYTES));
  HBH_CHECK(upload(s, e->in_q2, sigs, n * HBH_G2_BYTES));
  HBH_CHECK(e->out_v.ensure(n));
  HBH_CHECK(download(s, state.data(), e->hash_state, n));
  HBH_CHECK(hipStreamSynchronize(s));
  const std::vector<uint32_t> left = hash_leftovers(state);
  if (!left.empty()) {  // host-hashed, then patched into the table
    fixed.resize(n * HBH_G2_BYTES);
    hbh__hash_g2_seeds(left.size(), left.data(), seeds.data(), fixed.data());
    for (uint32_t i : left)
      HBH_CHECK(h2d(s, (uint8_t*)e->in_q1.p + (size_t)i * HBH_G2_BYTES, fixed.data() + (size_t)i * HBH_G2_BYTES,
                    HBH_G2_BYTES));
  }
  rc = run_pairing_sides(e, s, n, {e->in_p1.p, e->in_q1.p, nullptr, nullptr, nullptr, n},
                         {nullptr, e->in_q2.p, nullptr, nullptr, nullptr, n}, Resident(), 1, (uint8_t*)e->out_v.p);
  if (rc) return rc;
  HBH_CHECK(download(s, v, e->out_v, n));
  return call.finish();
}

int hbh_verify_ciphertexts_uv(hbh_engine* e, size_t n, const uint8_t* u, const uint8_t* data, const size_t* offsets,
                              const uint8_t* w, uint8_t* v) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n == 0) return HBH_OK;
  if (!u || !w || !v) return fail(HBH_ERR_ARG, "null pointer");
  int rc = check_msgs(n, data, offsets);
  if (rc) return rc;
  bool device;
  std::vector<uint8_t> g1k(n * HBH_G1_BYTES);  // P1 = G1K for every check
  {
    std::lock_guard<std::mutex> lk(e->mu);
    device = hash_on_device(e, n);
    if (e->g1k.empty()) {
      e->g1k.resize(HBH_G1_BYTES);
      rc = hbh_hash_bp_g1(e->g1k.data());
      if (rc) {
        e->g1k.clear();
        return fail(rc, hbh_host_last_error());
      }
    }
    for (size_t i = 0; i < n; i++) std::memcpy(g1k.data() + i * HBH_G1_BYTES, e->g1k.data(), HBH_G1_BYTES);
  }
  // e(G1K, W) == e(U, Q_bp): sides as Engine.verify_ciphertexts_bp's (P1 = G1K, Q1 = W, P2 = U, Q2 = Q)
  if (!device) {
    std::vector<uint8_t> q(n * HBH_G2_BYTES);
    rc = hbh_hash_g1_g2_bp(n, u, data, offsets, q.data(), 0);
    if (rc) return fail(rc, hbh_host_last_error());
    return run_pairing_eq_host(e, n, g1k.data(), w, n, nullptr, u, q.data(), n, nullptr, v);
  }
  std::vector<uint8_t> seeds(n * 32), state(n), fixed;
  hbh__hash_seeds(n, u, data, offsets, seeds.data());
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  // the Q_bp are written straight into the Q2 staging buffer of the pairing path and stay in HBM
  HBH_CHECK(upload(s, e->in_a, seeds.data(), n * 32));
  HBH_CHECK(e->in_q2.ensure(n * HBH_G2_BYTES));
  rc = launch_hash(e, s, n, (const uint8_t*)e->in_a.p, e->in_q2.p, hbl::HASH_FORM_BP);
  if (rc) return rc;
  HBH_CHECK(upload(s, e->in_p1, g1k.data(), n * HBH_G1_BYTES));
  HBH_CHECK(upload(s, e->in_q1, w, n * HBH_G2_BYTES));
  HBH_CHECK(upload(s, e->in_p2, u, n * HBH_G1_BYTES));
  HBH_CHECK(e->out_v.ensure(n));
  HBH_CHECK(download(s, state.data(), e->hash_state, n));
  HBH_CHECK(hipStreamSynchronize(s));
  const std::vector<uint32_t> left = hash_leftovers(state);
  if (!left.empty()) {  // host-hashed, then patched into the table
    fixed.resize(n * HBH_G2_BYTES);
    hbh__hash_g2_bp_seeds(left.size(), left.data(), seeds.data(), fixed.data());
    for (uint32_t i : left)
      HBH_CHECK(h2d(s, (uint8_t*)e->in_q2.p + (size_t)i * HBH_G2_BYTES, fixed.data() + (size_t)i * HBH_G2_BYTES,
                    HBH_G2_BYTES));
  }
  rc = run_pairing_sides(e, s, n, {e->in_p1.p, e->in_q1.p, nullptr, nullptr, nullptr, n},
                         {e->in_p2.p, e->in_q2.p, nullptr, nullptr, nullptr, n}, Resident(), 1, (uint8_t*)e->out_v.p);
  if (rc) return rc;
  HBH_CHECK(download(s, v, e->out_v, n));
  return call.finish();
}

int hbh_engine_encrypt(hbh_engine* e, size_t n, const uint8_t* pks, int pk_per_item, const uint8_t* data,
                       const size_t* offsets, const uint8_t* nonces, uint8_t* u_out, uint8_t* v_out, uint8_t* w_out) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n == 0) return HBH_OK;
  if (!pks || !nonces || !u_out || !w_out) return fail(HBH_ERR_ARG, "null pointer");
  int rc = check_msgs(n, data, offsets);
  if (rc) return rc;
  if (offsets[n] && !v_out) return fail(HBH_ERR_ARG, "null pointer");
  bool device;
  {
    std::lock_guard<std::mutex> lk(e->mu);
    device = hash_on_device(e, n);
  }
  if (!device) {
    rc = hbh_encrypt(n, pks, pk_per_item, data, offsets, nonces, u_out, v_out, w_out, 0);
    return rc ? fail(rc, hbh_host_last_error()) : HBH_OK;
  }
  // U, V and W on the host workers; between them only the seeds sha3(hash_g1_g2's message of the public
  // (U, V)) go to the device and the Q_bp come back.  Nonces, pk r and plaintexts stay in host memory.
  rc = hbh_encrypt_uv(n, pks, pk_per_item, data, offsets, nonces, u_out, v_out, 0);
  if (rc) return fail(rc, hbh_host_last_error());
  std::vector<uint8_t> seeds(n * 32), q(n * HBH_G2_BYTES);
  hbh__hash_seeds(n, u_out, v_out, offsets, seeds.data());
  rc = hash_seeds_device(e, n, seeds, hbl::HASH_FORM_BP, q.data());
  if (rc) return rc;
  rc = hbh_encrypt_w(n, q.data(), nonces, w_out, 0);
  return rc ? fail(rc, hbh_host_last_error()) : HBH_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- curve entry points
namespace {
int check_t(int t) { return (t < 0 || t > 4096) ? fail(HBH_ERR_ARG, "threshold out of range") : HBH_OK; }

template <class Launch>
int run_mul(hbh_engine* e, size_t n, const uint8_t* pts, size_t pt_bytes, const uint8_t* scalars, uint8_t* out,
            Launch launch) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n == 0) return HBH_OK;
  if (!pts || !scalars || !out) return fail(HBH_ERR_ARG, "null pointer");
  if (n > (size_t)1 << 28) return fail(HBH_ERR_ARG, "batch too large");
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  HBH_CHECK(upload(s, e->in_a, pts, n * pt_bytes));
  HBH_CHECK(upload(s, e->in_b, scalars, n * HBH_FR_BYTES));
  HBH_CHECK(e->out_x.ensure(n * pt_bytes));
  {
    StageScope tm(e, s, HBH_STAGE_CURVE);
    HBH_CHECK(launch(s, (int)n, e->in_a.p, (const uint32_t*)e->in_b.p, e->out_x.p));
  }
  HBH_CHECK(download(s, out, e->out_x, n * pt_bytes));
  return call.finish();
}

// The g1 comb table, built on the engine stream the first time a call needs it.
int ensure_fbtab(hbh_engine* e, hipStream_t s) {
  if (e->fbtab_ready) return HBH_OK;
  HBH_CHECK(e->fbtab.ensure(hbl::fb_table_bytes()));
  HBH_CHECK(hbl::fb_table(s, e->fbtab.p));
  e->fbtab_ready = true;
  return HBH_OK;
}

int ensure_fb16(hbh_engine* e, hipStream_t s) {
  if (e->fb16_ready) return HBH_OK;
  HBH_CHECK(e->fb16.ensure(hbl::fb16_table_bytes()));
  DevBuf scratch;  // freed before return, also on failure
  hipError_t err = scratch.ensure(hbl::fb16_scratch_bytes());
  if (err == hipSuccess) err = hbl::fb16_table(s, e->fb16.p, scratch.p);
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  scratch.release();
  HBH_CHECK(err);
  e->fb16_ready = true;
  return HBH_OK;
}

// G2 combines: few combines (latency-bound: the chip is idle but for the serial chains) take the
// lane-pair form (digits + k_interp_pair); many take k_interp_endo (throughput form).  With the x
// values on the host and at most HOST_DIGITS_MAX combines, the digits are computed on the host and
// uploaded (status too) instead of running k_interp_digits.
#ifndef HBH_INTERP_PAIR_MAX
#define HBH_INTERP_PAIR_MAX 384  // measured crossover with k_interp_endo<Fp2>: 100 combines 5.25 -> 2.46 ms, 1,024: 11.9 vs 15.8 ms
#endif
constexpr size_t INTERP_PAIR_MAX = HBH_INTERP_PAIR_MAX;
constexpr size_t HOST_DIGITS_MAX = 2;
// The digits of a combine call in e->in_d (four base-|x| digits per sample, g1: two base-x^2 digits):
// from the host when the x values are there and the call is small, else by k_interp_digits.
int stage_digits(hbh_engine* e, hipStream_t s, size_t ncomb, size_t m, const uint32_t* d_xs, int* d_status,
                 const uint32_t* h_xs, bool g1) {
  HBH_CHECK(e->in_d.ensure(ncomb * m * 4 * sizeof(uint64_t)));
  if (h_xs && ncomb <= HOST_DIGITS_MAX) {
    e->h_digits.resize(ncomb * m * 4);
    e->h_status.resize(ncomb);
    host_interp_digits(h_xs, ncomb, m, e->h_digits.data(), e->h_status.data(), g1);
    HBH_CHECK(h2d(s, e->in_d.p, e->h_digits.data(), ncomb * m * 32));
    HBH_CHECK(h2d(s, d_status, e->h_status.data(), ncomb * sizeof(int)));
  } else {
    HBH_CHECK(hbl::interp_digits(s, (int)ncomb, (int)m, d_xs, (uint64_t*)e->in_d.p, d_status, g1));
  }
  return HBH_OK;
}

int launch_combine_g2(hbh_engine* e, hipStream_t s, size_t ncomb, size_t m, const uint32_t* d_xs, const void* d_pts,
                      void* d_out, int* d_status, const uint32_t* h_xs = nullptr) {
  if (ncomb <= INTERP_PAIR_MAX && hbl::interp_g2_pair_fits((int)m)) {
    const int rc = stage_digits(e, s, ncomb, m, d_xs, d_status, h_xs, false);
    if (rc) return rc;
    HBH_CHECK(e->ipart.ensure(hbl::interp_g2_pair_part_bytes((int)ncomb)));
    HBH_CHECK(hbl::interp_g2_pair(s, (int)ncomb, (int)m, (const uint64_t*)e->in_d.p, d_pts, e->ipart.p, d_out));
    return HBH_OK;
  }
  HBH_CHECK(hbl::combine_g2(s, (int)ncomb, (int)m, d_xs, d_pts, d_out, d_status));
  return HBH_OK;
}

// G1 combines: few combines take the lane-quad latency form (digits + k_interp_g1q + join), many
// k_interp_endo<Fp> (throughput form).
#ifndef HBH_INTERP_G1Q_MAX
#define HBH_INTERP_G1Q_MAX 256  // quad form: 1 combine 0.91 ms, 100 1.74 ms (k_interp_endo<Fp>: 3.2 ms), 256 3.0 ms; 1,024 endo 4.1 ms
#endif
int launch_combine_g1(hbh_engine* e, hipStream_t s, size_t ncomb, size_t m, const uint32_t* d_xs, const void* d_pts,
                      void* d_out, int* d_status, const uint32_t* h_xs = nullptr) {
  if (ncomb <= HBH_INTERP_G1Q_MAX && m <= 4096) {
    const int rc = stage_digits(e, s, ncomb, m, d_xs, d_status, h_xs, true);
    if (rc) return rc;
    HBH_CHECK(e->ipart.ensure(hbl::interp_g1_quad_part_bytes((int)ncomb)));
    HBH_CHECK(hbl::interp_g1_quad(s, (int)ncomb, (int)m, (const uint64_t*)e->in_d.p, d_pts, e->ipart.p, d_out));
    return HBH_OK;
  }
  HBH_CHECK(hbl::combine_g1(s, (int)ncomb, (int)m, d_xs, d_pts, d_out, d_status));
  return HBH_OK;
}
int launch_combine(hbh_engine* e, hipStream_t s, bool g2, size_t ncomb, size_t m, const uint32_t* d_xs,
                   const void* d_pts, void* d_out, int* d_status, const uint32_t* h_xs = nullptr) {
  return g2 ? launch_combine_g2(e, s, ncomb, m, d_xs, d_pts, d_out, d_status, h_xs)
            : launch_combine_g1(e, s, ncomb, m, d_xs, d_pts, d_out, d_status, h_xs);
}

int run_interp(hbh_engine* e, size_t ncomb, int t, const uint32_t* idx, const uint8_t* pts, uint8_t* out, int* status,
               bool g2) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  int rc = check_t(t);
  if (rc) return rc;
  if (ncomb == 0) return HBH_OK;
  if (!idx || !pts || !out || !status) return fail(HBH_ERR_ARG, "null pointer");
  const size_t m = (size_t)t + 1, pb = g2 ? HBH_G2_BYTES : HBH_G1_BYTES;
  if (ncomb * m > (size_t)1 << 26) return fail(HBH_ERR_ARG, "batch too large");
  // x_k = idx_k + 1 as a small Fr integer (threshold_crypto into_fr_plus_1)
  std::vector<uint32_t> xs(ncomb * m);
  for (size_t k = 0; k < ncomb * m; k++) {
    if (idx[k] == 0xffffffffu) return fail(HBH_ERR_ARG, "node index out of range");
    xs[k] = idx[k] + 1;
  }
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  HBH_CHECK(upload(s, e->in_a, xs.data(), ncomb * m * 4));
  HBH_CHECK(upload(s, e->in_b, pts, ncomb * m * pb));
  HBH_CHECK(e->out_x.ensure(ncomb * pb));
  HBH_CHECK(e->status.ensure(ncomb * sizeof(int)));
  HBH_CHECK(hipMemsetAsync(e->status.p, 0, ncomb * sizeof(int), s));
  {
    StageScope tm(e, s, HBH_STAGE_CURVE);
    rc = launch_combine(e, s, g2, ncomb, m, (const uint32_t*)e->in_a.p, e->in_b.p, e->out_x.p, (int*)e->status.p,
                        xs.data());
    if (rc) return rc;
  }
  HBH_CHECK(download(s, out, e->out_x, ncomb * pb));
  HBH_CHECK(download(s, status, e->status, ncomb * sizeof(int)));
  return call.finish();
}

// ThresholdSign::combine_and_verify_sig's master check split off the interpolation (few combines, the
// latency case).  e(g1, sigma) == e(mpk, H) with sigma = sum_k lambda_k sigma_k is, by bilinearity,
//   prod_k e(lambda_k g1, sigma_k) * e(-mpk, H) == 1,
// which needs no sigma: its m + 1 Miller loops (two pairs per wave, k_wave's Miller-only mode) run on a
// second stream WHILE the engine stream interpolates sigma (one pair per wave, homogeneous walk: mode
// W1J of tools/gen_wave_prog.py); in the same launch the partial values are multiplied up a binary tree
// (the later of two sibling waves multiplies: log2(m + 1) products on the critical path instead of m)
// and the wave holding a combine's product runs the single final exponentiation (wave_miller_tree;
// HBH_SPLIT_TREE=0: a second launch multiplies the m + 1 values in order, wave_prod_fe).  The verdict is the same
// boolean for every input (an exact identity, no randomisation); lambda_k g1 comes from the device comb
// table summed in a 5-level tree on lane quads (k_g1_gen_quad) on the side stream, left in Jacobian
// form: the Miller kernel scales each line by Z^3 instead of inverting Z (WAVE_JAC_P).  A repeated index gives zero
// lambdas (status DuplicateEntry), as in the interpolation.
#ifndef HBH_SPLIT_PAIRS
#define HBH_SPLIT_PAIRS 1
#endif
}  // namespace
extern "C" int hbh__host_g1_neg(const uint8_t* pk, uint8_t* neg_out);
namespace {

int combine_verify_split(hbh_engine* e, size_t ncomb, size_t m, const std::vector<uint32_t>& xs,
                         const uint8_t* shares, const uint8_t* master_pk, const uint8_t* hashes, uint8_t* out,
                         int* status, uint8_t* verdicts) {
  // SPLIT_PAIRS pairs per wave: 1 = the homogeneous-walk program (two stages per Miller step),
  // 2 = the two-sided Jacobian program (WWJ, three stages per step, half the waves)
  constexpr int pairs = HBH_SPLIT_PAIRS;
  const size_t np = m + 1, nw = (np + pairs - 1) / pairs, nchk = ncomb * nw, nq = ncomb * np;
  constexpr size_t JB = 3 * 48;  // Jacobian P: X || Y || Z canonical
  uint8_t negpk[HBH_G1_BYTES];
  if (hbh__host_g1_neg(master_pk, negpk)) return fail(HBH_ERR_ARG, "master key coordinate >= p");  // checked by the caller too
  bool pk_inf = true;
  for (int b = 0; b < HBH_G1_BYTES; b++) pk_inf = pk_inf && negpk[b] == 0;
  // one upload: Q table (shares, then one H per combine) | GLS digits | lambdas | P sides | Q indices
  const size_t o_q = 0, o_dg = o_q + nq * HBH_G2_BYTES, o_lam = o_dg + ncomb * m * 32, o_p0 = o_lam + ncomb * m * 32,
               o_p1 = o_p0 + nchk * JB, o_i0 = o_p1 + nchk * JB, o_i1 = o_i0 + nchk * 4, in_bytes = o_i1 + nchk * 4;
  // one download: signatures | verdicts
  const size_t o_v = ncomb * HBH_G2_BYTES, out_bytes = o_v + ncomb;
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  if (!e->side) {
    HBH_CHECK(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
    HBH_CHECK(hipEventCreateWithFlags(&e->fork, hipEventDisableTiming));
    HBH_CHECK(hipEventCreateWithFlags(&e->join, hipEventDisableTiming));
  }
  const size_t stage_bytes = std::max(in_bytes, out_bytes);
  if (stage_bytes > e->h_stage_cap) {
    if (e->h_stage) HBH_CHECK(hipHostFree(e->h_stage));
    e->h_stage = nullptr;
    e->h_stage_cap = 0;
    HBH_CHECK(hipHostMalloc((void**)&e->h_stage, stage_bytes + stage_bytes / 4 + 4096, hipHostMallocDefault));
    e->h_stage_cap = stage_bytes + stage_bytes / 4 + 4096;
  }
  uint8_t* hs = e->h_stage;
  std::memcpy(hs + o_q, shares, ncomb * m * HBH_G2_BYTES);
  std::memcpy(hs + o_q + ncomb * m * HBH_G2_BYTES, hashes, ncomb * HBH_G2_BYTES);
  std::vector<int> lst(ncomb);
  host_lagrange(xs.data(), ncomb, m, (uint64_t*)(hs + o_lam), lst.data());
  host_gls_digits((const uint64_t*)(hs + o_lam), ncomb * m, (uint64_t*)(hs + o_dg));
  std::memset(hs + o_p0, 0, 2 * nchk * JB);
  uint32_t* i0 = (uint32_t*)(hs + o_i0);
  uint32_t* i1 = (uint32_t*)(hs + o_i1);
  for (size_t c = 0; c < ncomb; c++)
    for (size_t w = 0; w < nw; w++)
      for (int sd = 0; sd < pairs; sd++) {
        const size_t k = pairs * w + sd, j = c * nw + w;
        uint32_t* qi = sd ? &i1[j] : &i0[j];
        if (k < m) {
          *qi = (uint32_t)(c * m + k);  // (lambda_k g1, sigma_k): P written by k_g1_gen_quad
        } else {
          if (k == m) {  // (-mpk, H_c) with Z = 1 (Z = 0: mpk at infinity, an inactive pair)
            uint8_t* d = hs + (sd ? o_p1 : o_p0) + j * JB;
            std::memcpy(d, negpk, HBH_G1_BYTES);
            d[96] = pk_inf ? 0 : 1;
          }
          *qi = (uint32_t)(ncomb * m + c);  // then an inactive pad (P = O)
        }
      }
  hipStream_t s = call.s, s2 = e->side;
  HBH_CHECK(e->split_in.ensure(in_bytes));
  HBH_CHECK(e->split_out.ensure(out_bytes));
  HBH_CHECK(e->fval.ensure(nchk * 144 * 4));
  HBH_CHECK(e->ipart.ensure(hbl::interp_g2_pair_part_bytes((int)ncomb)));
  uint8_t* din = (uint8_t*)e->split_in.p;
  uint8_t* dout = (uint8_t*)e->split_out.p;
  HBH_CHECK(h2d(s, din, hs, in_bytes));
  HBH_CHECK(hipEventRecord(e->fork, s));
  HBH_CHECK(hipStreamWaitEvent(s2, e->fork, 0));
  // From here on both streams hold queued work: every exit joins the side stream into s before the
  // call closes on s, so e->done covers the side stream's kernels even when a launch fails.
  auto launch = [&]() -> int {
    // side stream: lambda_k g1 (Jacobian, over the zero P entries), the m + 1 Miller loops, the product
    // and the final exponentiation
    int rc = ensure_fbtab(e, s2);
    if (rc) return rc;
    HBH_CHECK(hbl::g1_gen_tree(s2, (int)(ncomb * m), (int)m, (int)nw, pairs, e->fbtab.p,
                               (const uint32_t*)(din + o_lam), din + o_p0, din + o_p1));
    hbl::PairSideDesc sd0 = {din + o_p0, din + o_q, nullptr, nullptr, (const uint32_t*)(din + o_i0), nq};
    hbl::PairSideDesc sd1 = {din + o_p1, din + o_q, nullptr, nullptr, (const uint32_t*)(din + o_i1), nq};
    StageScope tp(e, s2, HBH_STAGE_PAIRING);
    const int wflags = hbl::WAVE_MILLER_ONLY | hbl::WAVE_JAC_P | (pairs == 1 ? hbl::WAVE_ONE_SIDE : 0);
    if (e->split_tree) {  // product up a tree and the final exponentiation inside the Miller launch
      HBH_CHECK(e->tree_cnt.ensure(hbl::wave_tree_counter_bytes((int)ncomb, (int)nw)));
      HBH_CHECK(hbl::wave_miller_tree(s2, (int)ncomb, (int)nw, sd0, sd1, wflags, (uint32_t*)e->fval.p,
                                      (uint32_t*)e->tree_cnt.p, dout + o_v));
    } else {
      HBH_CHECK(hbl::wave_verify(s2, (int)nchk, sd0, sd1, wflags, nullptr, (uint32_t*)e->fval.p));
      HBH_CHECK(hbl::wave_prod_fe(s2, (int)ncomb, (int)nw, (const uint32_t*)e->fval.p, dout + o_v));
    }
    tp.stop();
    // engine stream, concurrently: the interpolation (lane-quad latency form, host digits)
    StageScope tm(e, s, HBH_STAGE_CURVE);
    HBH_CHECK(hbl::interp_g2_pair(s, (int)ncomb, (int)m, (const uint64_t*)(din + o_dg), din + o_q, e->ipart.p, dout));
    return HBH_OK;
  };
  const int lrc = launch();
  const hipError_t jerr = hipEventRecord(e->join, s2);
  const hipError_t werr = jerr == hipSuccess ? hipStreamWaitEvent(s, e->join, 0) : jerr;
  if (werr != hipSuccess) {  // cannot order s after s2: drain both before the workspaces are reused
    (void)hipStreamSynchronize(s2);
    (void)hipStreamSynchronize(s);
  }
  if (lrc) return lrc;
  if (werr != hipSuccess) return fail(HBH_ERR_DEVICE, std::string("split check join: ") + hipGetErrorString(werr));
  HBH_CHECK(download(s, hs, e->split_out, out_bytes));
  const int frc = call.finish();
  if (frc) return frc;
  std::memcpy(out, hs, ncomb * HBH_G2_BYTES);
  std::memcpy(verdicts, hs + o_v, ncomb);
  for (size_t c = 0; c < ncomb; c++) status[c] = lst[c];
  return HBH_OK;
}
}  // namespace

extern "C" {

int hbh_g1_mul(hbh_engine* e, size_t n, const uint8_t* pts, const uint8_t* scalars, uint8_t* out) {
  return run_mul(e, n, pts, HBH_G1_BYTES, scalars, out, hbl::g1_mul);
}
int hbh_g2_mul(hbh_engine* e, size_t n, const uint8_t* pts, const uint8_t* scalars, uint8_t* out) {
  return run_mul(e, n, pts, HBH_G2_BYTES, scalars, out, hbl::g2_mul);
}
int hbh_interpolate_g2(hbh_engine* e, size_t ncomb, int t, const uint32_t* idx, const uint8_t* pts, uint8_t* out,
                       int* status) {
  return run_interp(e, ncomb, t, idx, pts, out, status, true);
}
int hbh_interpolate_g1(hbh_engine* e, size_t ncomb, int t, const uint32_t* idx, const uint8_t* pts, uint8_t* out,
                       int* status) {
  return run_interp(e, ncomb, t, idx, pts, out, status, false);
}

// ThresholdSign::combine_and_verify_sig (src/threshold_sign.rs:249-270) as one device pass: the
// interpolated signature stays in HBM and feeds the master check e(pk, H_c) == e(g1, sig_c) on the
// same stream -- no host round trip between combine and verify.
int hbh_combine_verify_g2(hbh_engine* e, size_t ncomb, int t, const uint32_t* idx, const uint8_t* shares,
                          const uint8_t* master_pk, const uint8_t* hashes, uint8_t* out, int* status,
                          uint8_t* verdicts) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  int rc = check_t(t);
  if (rc) return rc;
  if (ncomb == 0) return HBH_OK;
  if (!idx || !shares || !master_pk || !hashes || !out || !status || !verdicts) return fail(HBH_ERR_ARG, "null pointer");
  const size_t m = (size_t)t + 1;
  if (ncomb * m > (size_t)1 << 26) return fail(HBH_ERR_ARG, "batch too large");
  std::vector<uint32_t> xs(ncomb * m);
  for (size_t k = 0; k < ncomb * m; k++) {
    if (idx[k] == 0xffffffffu) return fail(HBH_ERR_ARG, "node index out of range");
    xs[k] = idx[k] + 1;
  }
  {
    // one contract for both forms of the check: a master key coordinate >= p is an argument error
    // (the split form rejected it, interpolate-then-verify returned verdicts)
    uint8_t negpk[HBH_G1_BYTES];
    if (hbh__host_g1_neg(master_pk, negpk)) return fail(HBH_ERR_ARG, "master key coordinate >= p");
  }
  if (e->split_check && (e->split_max ? ncomb <= e->split_max : ncomb * (m + 1) <= split_waves_max(t)) &&
      ncomb <= INTERP_PAIR_MAX && hbl::interp_g2_pair_fits((int)m))
    return combine_verify_split(e, ncomb, m, xs, shares, master_pk, hashes, out, status, verdicts);
  // P1 = master pk (one record per combine), P2 = the G1 generator (a flag, nothing uploaded)
  std::vector<uint8_t> p12(ncomb * HBH_G1_BYTES);
  for (size_t c = 0; c < ncomb; c++) std::memcpy(p12.data() + c * HBH_G1_BYTES, master_pk, HBH_G1_BYTES);
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  HBH_CHECK(upload(s, e->in_a, xs.data(), ncomb * m * 4));
  HBH_CHECK(upload(s, e->in_b, shares, ncomb * m * HBH_G2_BYTES));
  HBH_CHECK(upload(s, e->in_q1, hashes, ncomb * HBH_G2_BYTES));
  HBH_CHECK(upload(s, e->in_p1, p12.data(), p12.size()));
  HBH_CHECK(e->out_x.ensure(ncomb * HBH_G2_BYTES));
  HBH_CHECK(e->status.ensure(ncomb * sizeof(int)));
  HBH_CHECK(e->out_v.ensure(ncomb));
  HBH_CHECK(hipMemsetAsync(e->status.p, 0, ncomb * sizeof(int), s));
  {
    StageScope tm(e, s, HBH_STAGE_CURVE);
    rc = launch_combine_g2(e, s, ncomb, m, (const uint32_t*)e->in_a.p, e->in_b.p, e->out_x.p, (int*)e->status.p,
                           xs.data());
    if (rc) return rc;
  }
  rc = run_pairing_dev(e, s, ncomb, e->in_p1.p, e->in_q1.p, ncomb, nullptr, nullptr, e->out_x.p, ncomb, nullptr, 1,
                       (uint8_t*)e->out_v.p);
  if (rc) return rc;
  HBH_CHECK(download(s, out, e->out_x, ncomb * HBH_G2_BYTES));
  HBH_CHECK(download(s, status, e->status, ncomb * sizeof(int)));
  HBH_CHECK(download(s, verdicts, e->out_v, ncomb));
  return call.finish();
}

int hbh_bivar_row(hbh_engine* e, size_t nrow, int t, size_t nparts, const uint8_t* commits, const uint32_t* part_idx,
                  const uint32_t* xs, uint8_t* out) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  int rc = check_t(t);
  if (rc) return rc;
  if (nrow == 0) return HBH_OK;
  if (!commits || !part_idx || !xs || !out) return fail(HBH_ERR_ARG, "null pointer");
  const size_t ncoef = (size_t)(t + 1) * (t + 2) / 2;
  for (size_t r = 0; r < nrow; r++)
    if (part_idx[r] >= nparts) return fail(HBH_ERR_ARG, "part index out of range");
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  const size_t nout = nrow * (t + 1);
  HBH_CHECK(upload(s, e->in_a, commits, nparts * ncoef * HBH_G1_BYTES));
  HBH_CHECK(upload(s, e->in_b, part_idx, nrow * 4));
  HBH_CHECK(upload(s, e->in_c, xs, nrow * 4));
  HBH_CHECK(e->out_x.ensure(nout * HBH_G1_BYTES));
  {
    StageScope tm(e, s, HBH_STAGE_CURVE);
    HBH_CHECK(hbl::bivar_row(s, (int)nrow, t, e->in_a.p, (const uint32_t*)e->in_b.p, (const uint32_t*)e->in_c.p,
                             e->out_x.p));
  }
  HBH_CHECK(download(s, out, e->out_x, nout * HBH_G1_BYTES));
  return call.finish();
}

}  // extern "C"

namespace {
// The decoder of one call: a forced form for every n; AUTO takes the latency form (k_wire_split.hip)
// up to the group's threshold and the throughput form (k_wire.hip) above it.
hipError_t launch_decompress(const hbh_engine* e, hipStream_t s, size_t n, bool g2, const uint32_t* xw,
                             const uint8_t* fl, void* out, uint8_t* ok) {
  const size_t split_max = g2 ? HBH_AUTO_DEC_G2_SPLIT_MAX : HBH_AUTO_DEC_G1_SPLIT_MAX;
  const bool split = e->dec_impl == HBH_DEC_SPLIT || (e->dec_impl == HBH_DEC_AUTO && n <= split_max);
  if (g2)
    return split ? hbl::g2_decompress_split(s, (int)n, xw, fl, out, ok)
                 : hbl::g2_decompress(s, (int)n, xw, fl, out, ok);
  return split ? hbl::g1_decompress_split(s, (int)n, xw, fl, out, ok) : hbl::g1_decompress(s, (int)n, xw, fl, out, ok);
}

int run_decompress(hbh_engine* e, size_t n, const uint8_t* in, uint8_t* out, uint8_t* ok, bool g2) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n == 0) return HBH_OK;
  if (!in || !out || !ok) return fail(HBH_ERR_ARG, "null pointer");
  if (n > (size_t)1 << 28) return fail(HBH_ERR_ARG, "batch too large");
  const int nfe = g2 ? 2 : 1;
  const size_t pb = g2 ? HBH_G2_BYTES : HBH_G1_BYTES;
  std::vector<uint32_t> xw(n * 12 * nfe);
  std::vector<uint8_t> fl(n);
  for (size_t i = 0; i < n; i++) parse_compressed(in + i * 48 * nfe, nfe, xw.data() + i * 12 * nfe, fl[i]);
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  HBH_CHECK(upload(s, e->in_a, xw.data(), xw.size() * 4));
  HBH_CHECK(upload(s, e->in_b, fl.data(), n));
  HBH_CHECK(e->out_x.ensure(n * pb));
  HBH_CHECK(e->out_v.ensure(n));
  {
    StageScope tm(e, s, HBH_STAGE_CURVE);
    HBH_CHECK(launch_decompress(e, s, n, g2, (const uint32_t*)e->in_a.p, (const uint8_t*)e->in_b.p, e->out_x.p,
                                (uint8_t*)e->out_v.p));
  }
  HBH_CHECK(download(s, out, e->out_x, n * pb));
  HBH_CHECK(download(s, ok, e->out_v, n));
  return call.finish();
}
}  // namespace

extern "C" {

int hbh_g1_decompress(hbh_engine* e, size_t n, const uint8_t* in, uint8_t* out, uint8_t* ok) {
  return run_decompress(e, n, in, out, ok, false);
}
int hbh_g2_decompress(hbh_engine* e, size_t n, const uint8_t* in, uint8_t* out, uint8_t* ok) {
  return run_decompress(e, n, in, out, ok, true);
}

int hbh_commitment_eval(hbh_engine* e, size_t n, int t, size_t ncommits, const uint8_t* commits,
                        const uint32_t* commit_idx, const uint32_t* xs, uint8_t* out) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  int rc = check_t(t);
  if (rc) return rc;
  if (n == 0) return HBH_OK;
  if (!commits || !commit_idx || !xs || !out) return fail(HBH_ERR_ARG, "null pointer");
  if (n > (size_t)1 << 28) return fail(HBH_ERR_ARG, "batch too large");
  for (size_t r = 0; r < n; r++)
    if (commit_idx[r] >= ncommits) return fail(HBH_ERR_ARG, "commitment index out of range");
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  HBH_CHECK(upload(s, e->in_a, commits, ncommits * (size_t)(t + 1) * HBH_G1_BYTES));
  HBH_CHECK(upload(s, e->in_b, commit_idx, n * 4));
  HBH_CHECK(upload(s, e->in_c, xs, n * 4));
  HBH_CHECK(e->out_x.ensure(n * HBH_G1_BYTES));
  {
    StageScope tm(e, s, HBH_STAGE_CURVE);
    HBH_CHECK(hbl::commit_eval(s, (int)n, t, e->in_a.p, (const uint32_t*)e->in_b.p, (const uint32_t*)e->in_c.p,
                               e->out_x.p));
  }
  HBH_CHECK(download(s, out, e->out_x, n * HBH_G1_BYTES));
  return call.finish();
}

int hbh_bivar_ack_check(hbh_engine* e, size_t nack, int t, size_t nparts, const uint8_t* commits,
                        const uint32_t* part_idx, const uint32_t* xs, const uint32_t* ys, const uint8_t* vals,
                        uint8_t* verdicts) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  int rc = check_t(t);
  if (rc) return rc;
  if (nack == 0) return HBH_OK;
  if (!commits || !part_idx || !xs || !ys || !vals || !verdicts) return fail(HBH_ERR_ARG, "null pointer");
  const size_t ncoef = (size_t)(t + 1) * (t + 2) / 2;
  // one row(x) per distinct (part, x): evaluate(x, y) = sum_j row(x)_j y^j
  std::vector<uint32_t> row_part, row_x, row_of;
  if (!dedup_rows(nack, nparts, part_idx, xs, row_part, row_x, row_of))
    return fail(HBH_ERR_ARG, "part index out of range");
  const size_t nrow = row_part.size();
  std::vector<uint32_t> order;
  order_by_y(nack, ys, order);
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  HBH_CHECK(upload(s, e->in_a, commits, nparts * ncoef * HBH_G1_BYTES));
  HBH_CHECK(e->in_b.ensure(nrow * 8 + nack * 12));
  HBH_CHECK(upload(s, e->in_c, vals, nack * HBH_FR_BYTES));
  HBH_CHECK(e->work.ensure(hbl::bivar_rows_quad_bytes((int)nrow, t)));
  HBH_CHECK(e->out_v.ensure(nack));
  uint32_t* d_rp = (uint32_t*)e->in_b.p;
  uint32_t* d_rx = d_rp + nrow;
  uint32_t* d_ro = d_rx + nrow;
  uint32_t* d_y = d_ro + nack;
  uint32_t* d_ord = d_y + nack;
  HBH_CHECK(h2d(s, d_rp, row_part.data(), nrow * 4));
  HBH_CHECK(h2d(s, d_rx, row_x.data(), nrow * 4));
  HBH_CHECK(h2d(s, d_ro, row_of.data(), nack * 4));
  HBH_CHECK(h2d(s, d_y, ys, nack * 4));
  HBH_CHECK(h2d(s, d_ord, order.data(), nack * 4));
  {
    StageScope tm(e, s, HBH_STAGE_CURVE);
    HBH_CHECK(hbl::bivar_row_quad(s, (int)nrow, t, e->in_a.p, d_rp, d_rx, e->work.p));
    rc = ensure_fbtab(e, s);
    if (rc) return rc;
    HBH_CHECK(hbl::bivar_check_quad(s, (int)nack, t, e->work.p, d_ro, d_y, (const uint32_t*)e->in_c.p, e->fbtab.p,
                                    (uint8_t*)e->out_v.p, d_ord));
  }
  HBH_CHECK(download(s, verdicts, e->out_v, nack));
  return call.finish();
}

}  // extern "C"

// ---------------------------------------------------------------- device-resident variants
// Inputs and outputs in device memory, asynchronous on `stream` (NULL = engine stream), ordered
// after the engine's previous call like hbh_verify_pairing_eq_dev.
namespace {
int run_interp_dev(hbh_engine* e, void* stream, size_t ncomb, int t, const uint32_t* d_idx, const void* d_pts,
                   void* d_out, int* d_status, bool g2) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  int rc = check_t(t);
  if (rc) return rc;
  if (ncomb == 0) return HBH_OK;
  if (!d_idx || !d_pts || !d_out || !d_status) return fail(HBH_ERR_ARG, "null pointer");
  const size_t m = (size_t)t + 1;
  if (ncomb * m > (size_t)1 << 26) return fail(HBH_ERR_ARG, "batch too large");
  EngineCall call(e, stream, false);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  HBH_CHECK(e->in_a.ensure(ncomb * m * 4));
  HBH_CHECK(hipMemsetAsync(d_status, 0, ncomb * sizeof(int), s));
  HBH_CHECK(hbl::index_plus_one(s, (int)(ncomb * m), (int)m, d_idx, (uint32_t*)e->in_a.p, d_status));
  {
    StageScope tm(e, s, HBH_STAGE_CURVE);
    rc = launch_combine(e, s, g2, ncomb, m, (const uint32_t*)e->in_a.p, d_pts, d_out, d_status);
    if (rc) return rc;
  }
  return call.finish();
}

int run_decompress_dev(hbh_engine* e, void* stream, size_t n, const uint8_t* d_in, void* d_out, uint8_t* d_ok,
                       bool g2) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n == 0) return HBH_OK;
  if (!d_in || !d_out || !d_ok) return fail(HBH_ERR_ARG, "null pointer");
  if (n > (size_t)1 << 28) return fail(HBH_ERR_ARG, "batch too large");
  const int nfe = g2 ? 2 : 1;
  // a staging slot of its own: wait for the last general call and this slot's previous user only
  EngineCall call(e, stream, false, EngineCall::WIRE_SLOT);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  HBH_CHECK(e->wire_w[call.slot].ensure(n * 12 * nfe * 4));
  HBH_CHECK(e->wire_f[call.slot].ensure(n));
  uint32_t* xw = (uint32_t*)e->wire_w[call.slot].p;
  uint8_t* fl = (uint8_t*)e->wire_f[call.slot].p;
  {
    StageScope tm(e, s, HBH_STAGE_CURVE);
    HBH_CHECK(hbl::wire_parse(s, (int)n, nfe, d_in, xw, fl));
    HBH_CHECK(launch_decompress(e, s, n, g2, xw, fl, d_out, d_ok));
  }
  return call.finish();
}
}  // namespace

extern "C" {

int hbh_interpolate_g1_dev(hbh_engine* e, void* stream, size_t ncomb, int t, const uint32_t* d_idx, const void* d_pts,
                           void* d_out, int* d_status) {
  return run_interp_dev(e, stream, ncomb, t, d_idx, d_pts, d_out, d_status, false);
}
int hbh_interpolate_g2_dev(hbh_engine* e, void* stream, size_t ncomb, int t, const uint32_t* d_idx, const void* d_pts,
                           void* d_out, int* d_status) {
  return run_interp_dev(e, stream, ncomb, t, d_idx, d_pts, d_out, d_status, true);
}
int hbh_g1_decompress_dev(hbh_engine* e, void* stream, size_t n, const uint8_t* d_in, void* d_out, uint8_t* d_ok) {
  return run_decompress_dev(e, stream, n, d_in, d_out, d_ok, false);
}
int hbh_g2_decompress_dev(hbh_engine* e, void* stream, size_t n, const uint8_t* d_in, void* d_out, uint8_t* d_ok) {
  return run_decompress_dev(e, stream, n, d_in, d_out, d_ok, true);
}

int hbh_bivar_ack_check_dev(hbh_engine* e, void* stream, size_t nack, int t, const void* d_commits, size_t nrow,
                            const uint32_t* d_row_part, const uint32_t* d_row_x, const uint32_t* d_row_of,
                            const uint32_t* d_ys, const void* d_vals, uint8_t* d_verdicts) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  int rc = check_t(t);
  if (rc) return rc;
  if (nack == 0) return HBH_OK;
  if (!d_commits || !d_row_part || !d_row_x || !d_row_of || !d_ys || !d_vals || !d_verdicts || nrow == 0)
    return fail(HBH_ERR_ARG, "null pointer");
  EngineCall call(e, stream, false);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  HBH_CHECK(e->work.ensure(hbl::bivar_rows_quad_bytes((int)nrow, t)));
  {
    StageScope tm(e, s, HBH_STAGE_CURVE);
    HBH_CHECK(hbl::bivar_row_quad(s, (int)nrow, t, d_commits, d_row_part, d_row_x, e->work.p));
    rc = ensure_fbtab(e, s);
    if (rc) return rc;
    HBH_CHECK(hbl::bivar_check_quad(s, (int)nack, t, e->work.p, d_row_of, d_ys, (const uint32_t*)d_vals, e->fbtab.p,
                                    d_verdicts, nullptr));
  }
  return call.finish();
}

}  // extern "C"

extern "C" {

// out[i] = g1 * k_i from the comb table: Poly::commitment / BivarPoly::commitment and public-key
// derivation (src/sync_key_gen.rs:346-357, 508; network_info.rs:59-62).
int hbh_g1_mul_gen(hbh_engine* e, size_t n, const uint8_t* scalars, uint8_t* out) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n == 0) return HBH_OK;
  if (!scalars || !out) return fail(HBH_ERR_ARG, "null pointer");
  if (n > (size_t)1 << 28) return fail(HBH_ERR_ARG, "batch too large");
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  int rc = ensure_fbtab(e, s);
  if (rc) return rc;
  HBH_CHECK(upload(s, e->in_a, scalars, n * 32));
  HBH_CHECK(e->out_x.ensure(n * HBH_G1_BYTES));
  {
    StageScope tm(e, s, HBH_STAGE_CURVE);
    HBH_CHECK(hbl::g1_mul_gen(s, (int)n, e->fbtab.p, (const uint32_t*)e->in_a.p, e->out_x.p));
  }
  HBH_CHECK(download(s, out, e->out_x, n * HBH_G1_BYTES));
  return call.finish();
}

}  // extern "C"

// ---------------------------------------------------------------- device-resident commitment sets
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

// Frees a set's device memory and detaches it from its engine (cs->e = nullptr): every later call on
// the set fails with HBH_ERR_ARG, and hbh_commit_set_destroy only deletes the host object.  Caller
// holds the engine lock with the engine's streams drained.
void release_set_device(hbh_commit_set* cs) {
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
  std::vector<uint32_t> order;
  hbh_engine* e = cs->e;
  const int t = cs->t;
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  // lane quads (four lanes per ack, one wave per SIMD) for latency; one lane per ack on affine
  // rows (two waves per SIMD, mixed additions) for throughput
  const bool lane = e->ack_impl == HBH_ACK_LANE || e->ack_impl == HBH_ACK_LANE_HORNER ||
                    (e->ack_impl == HBH_ACK_AUTO && nack >= HBH_ACK_LANE_MIN);
  std::vector<uint32_t> slot;
  rc = set_rows(cs, s, lane, nack, part_idx, xs, slot);
  if (rc) return rc;
  FdPlan fd;
  if (lane && e->ack_fd && e->ack_impl != HBH_ACK_LANE_HORNER) {
    plan_fd(nack, slot, ys, t, fd);
    // the Horner kernel's acks in order of y
    std::vector<uint32_t> oy(fd.other.size());
    for (size_t k = 0; k < fd.other.size(); k++) oy[k] = ys[fd.other[k]];
    order_by_y(fd.other.size(), oy.data(), order);
    for (auto& o : order) o = fd.other[o];
  } else {
    order_by_y(nack, ys, order);
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
  if (!fd.slot.empty() && ensure_fb16(e, s) != HBH_OK) {
    // the 16-bit comb (96 MiB + ~192 MiB of build scratch) could not be built: the Horner kernel
    // checks every ack (same verdicts), and this engine stops planning FD runs
    e->fb16.release();
    e->ack_fd = false;
    static std::once_flag warned;
    std::call_once(warned, [] { fprintf(stderr, "hbbft_hip: no memory for the FD ack comb; Horner ack checks\n"); });
    fd = FdPlan();
    order_by_y(nack, ys, order);
  }
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
  if (lane && nfd) {
    HBH_CHECK(hbl::bivar_fd(s, (int)nfd, t, cs->rows[1].p, d_fd, d_fd + nfd, d_fd + 2 * nfd, d_fd + 3 * nfd,
                            e->fd_e.p));
    HBH_CHECK(hbl::bivar_fd_check(s, (int)fd.fd_acks.size(), e->fd_e.p, d_fd + 4 * nfd, (const uint32_t*)e->in_c.p,
                                  e->fb16.p, d_fd + 4 * nfd + nack, (uint8_t*)e->out_v.p));
    HBH_CHECK(hbl::bivar_check(s, (int)order.size(), t, cs->rows[1].p, d_ro, d_y, (const uint32_t*)e->in_c.p,
                               e->fbtab.p, (uint8_t*)e->out_v.p, d_ord));
  } else if (lane)
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

// ---------------------------------------------------------------- device-resident G2 sets
// The G2 point every share of an instance is checked against -- H of a ThresholdSign document
// (src/threshold_sign.rs:223), H_uv and W of a ThresholdDecrypt ciphertext (src/threshold_decrypt.rs:227)
// -- lives as long as the instance and is read by every drain that verifies its shares: a set keeps
// such points prepared in HBM (line table, affine point, infinity byte per slot), so a drain names
// slots and its verify kernel starts without the serial table walk (k_oct_prep).

// Frees a set's device memory and detaches it from its engine, as release_set_device.
void release_g2_set_device(hbh_g2_set* gs) {
  if (gs->mem) (void)hipFree(gs->mem);
  gs->mem = gs->lines = gs->q = nullptr;
  gs->qinf = nullptr;
  gs->slots.reset(0);
  gs->e = nullptr;
}

namespace {
// every coordinate of n ABI G2 points below p
bool g2_coords_canonical(size_t n, const uint8_t* pts) {
  for (size_t c = 0; c < 4 * n; c++) {
    const uint8_t* b = pts + c * 48;
    bool below = false;
    for (int w = 11; w >= 0; w--) {
      uint32_t x;
      std::memcpy(&x, b + 4 * w, 4);  // little-endian host
      const uint32_t pw = hb::PM2_W[w] + (w == 0 ? 2u : 0u);  // p = (p - 2) + 2, no carry out of word 0
      if (x != pw) {
        below = x < pw;
        break;
      }
    }
    if (!below) return false;
  }
  return true;
}

int g2_set_call_check(const hbh_g2_set* gs) {
  if (!gs) return fail(HBH_ERR_ARG, "null G2 set");
  if (!gs->e) return fail(HBH_ERR_ARG, "G2 set detached: its engine was destroyed");
  return HBH_OK;
}
}  // namespace

extern "C" {

int hbh_g2_set_create(hbh_engine* e, size_t capacity, hbh_g2_set** out) {
  if (!e || !out) return fail(HBH_ERR_ARG, "null pointer");
  *out = nullptr;
  if (capacity == 0 || capacity > ((size_t)1 << 20)) return fail(HBH_ERR_ARG, "G2 set capacity out of range");
  std::lock_guard<std::mutex> lk(e->mu);
  HBH_CHECK(hipSetDevice(e->device));
  const size_t tb = hbl::pair_table_bytes(1);
  void* mem = nullptr;
  if (hipMalloc(&mem, capacity * (tb + HBH_G2_BYTES + 1)) != hipSuccess)
    return fail(HBH_ERR_NOMEM, "no device memory for the G2 set");
  // a slot never added reads as a point at infinity (an inactive pair), whatever a _dev caller names
  hipError_t err = hipMemsetAsync((uint8_t*)mem + capacity * tb, 0, capacity * HBH_G2_BYTES, e->stream);
  if (err == hipSuccess) err = hipMemsetAsync((uint8_t*)mem + capacity * (tb + HBH_G2_BYTES), 1, capacity, e->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  if (err != hipSuccess) {
    (void)hipFree(mem);
    return fail(HBH_ERR_DEVICE, std::string("hipMemset: ") + hipGetErrorString(err));
  }
  hbh_g2_set* gs = new hbh_g2_set();
  gs->e = e;
  gs->slots.reset(capacity);
  gs->mem = gs->lines = mem;
  gs->q = (uint8_t*)mem + capacity * tb;
  gs->qinf = (uint8_t*)mem + capacity * (tb + HBH_G2_BYTES);
  e->g2_sets.insert(gs);
  *out = gs;
  return HBH_OK;
}

int hbh_g2_set_destroy(hbh_g2_set* gs) {
  if (!gs) return HBH_OK;
  if (hbh_engine* e = gs->e) {  // else: detached by hbh_engine_destroy, device memory already freed
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    (void)hipEventSynchronize(e->done);
    for (hipEvent_t ev : e->slot_done) (void)hipEventSynchronize(ev);  // _set_dev calls on caller streams
    (void)hipStreamSynchronize(e->stream);
    e->g2_sets.erase(gs);
    release_g2_set_device(gs);
  }
  delete gs;
  return HBH_OK;
}

int hbh_g2_set_add(hbh_g2_set* gs, size_t n, const uint8_t* pts, uint32_t* slots) {
  int rc = g2_set_call_check(gs);
  if (rc) return rc;
  if (n == 0) return HBH_OK;
  if (!pts || !slots) return fail(HBH_ERR_ARG, "null pointer");
  if (!g2_coords_canonical(n, pts)) {
    // the point at infinity is all zero, hence canonical; anything else >= p is refused
    return fail(HBH_ERR_ARG, "coordinate >= p");
  }
  hbh_engine* e = gs->e;
  // GENERAL: waits for done and both table slots, so no reader of a reused slot is still in flight
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  if (!gs->slots.take(n, slots)) return fail(HBH_ERR_ARG, "G2 set full");
  auto prepare = [&]() -> int {
    hipStream_t s = call.s;
    HBH_CHECK(upload(s, e->in_q1, pts, n * HBH_G2_BYTES));
    HBH_CHECK(upload(s, e->in_i1, slots, n * 4));
    {
      StageScope tm(e, s, HBH_STAGE_PREPARE);
      HBH_CHECK(hbl::oct_prep(s, (int)n, e->in_q1.p, gs->lines, gs->qinf, (const uint32_t*)e->in_i1.p,
                              gs->slots.capacity(), gs->q));
    }
    return call.finish();
  };
  rc = prepare();
  if (rc) (void)gs->slots.release(n, slots);  // never filled: free again
  return rc;
}

int hbh_g2_set_release(hbh_g2_set* gs, size_t n, const uint32_t* slots) {
  int rc = g2_set_call_check(gs);
  if (rc) return rc;
  if (n == 0) return HBH_OK;
  if (!slots) return fail(HBH_ERR_ARG, "null pointer");
  std::lock_guard<std::mutex> lk(gs->e->mu);
  if (!gs->slots.release(n, slots)) return fail(HBH_ERR_ARG, "G2 set slot is not live");
  return HBH_OK;
}

int hbh_g2_set_size(const hbh_g2_set* gs, size_t* live, size_t* capacity) {
  if (!gs) return fail(HBH_ERR_ARG, "null G2 set");
  if (live) *live = gs->slots.live_count();
  if (capacity) *capacity = gs->slots.capacity();
  return HBH_OK;
}

int hbh_verify_pairing_eq_set(hbh_engine* e, size_t n, const uint8_t* p1, hbh_g2_set* set1, const uint8_t* q1,
                              size_t nq1, const uint32_t* i1, const uint8_t* p2, hbh_g2_set* set2, const uint8_t* q2,
                              size_t nq2, const uint32_t* i2, uint8_t* v) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n && (!p1 || !p2)) return fail(HBH_ERR_ARG, "null pointer");
  return run_pairing_eq_host(e, n, p1, q1, nq1, i1, p2, q2, nq2, i2, v, set1, set2);
}

int hbh_verify_sig_shares_set(hbh_engine* e, size_t n, const uint8_t* pks, const uint8_t* sigs, hbh_g2_set* docs,
                              const uint32_t* doc_slot, uint8_t* v) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (!docs) return fail(HBH_ERR_ARG, "null G2 set");
  if (n && (!pks || !sigs)) return fail(HBH_ERR_ARG, "null pointer");
  return run_pairing_eq_host(e, n, pks, nullptr, 0, doc_slot, nullptr, sigs, n, nullptr, v, docs, nullptr);
}

int hbh_verify_dec_shares_set(hbh_engine* e, size_t n, const uint8_t* shares, const uint8_t* pks, hbh_g2_set* cts,
                              const uint32_t* huv_slot, const uint32_t* w_slot, uint8_t* v) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (!cts) return fail(HBH_ERR_ARG, "null G2 set");
  if (n && (!shares || !pks)) return fail(HBH_ERR_ARG, "null pointer");
  return run_pairing_eq_host(e, n, shares, nullptr, 0, huv_slot, pks, nullptr, 0, w_slot, v, cts, cts);
}

int hbh_verify_pairing_eq_set_dev(hbh_engine* e, void* stream, size_t n, const void* d_p1, hbh_g2_set* set1,
                                  const void* d_q1, size_t nq1, const uint32_t* d_i1, const void* d_p2,
                                  hbh_g2_set* set2, const void* d_q2, size_t nq2, const uint32_t* d_i2, uint8_t* d_v) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  hbh_g2_set* const set[2] = {set1, set2};
  const void* const d_q[2] = {d_q1, d_q2};
  const void* const d_p[2] = {d_p1, d_p2};
  const uint32_t* const d_i[2] = {d_i1, d_i2};
  const size_t nq[2] = {nq1, nq2};
  for (int k = 0; k < 2; k++) {
    if (!set[k]) continue;
    const int rc = check_g2_set(e, set[k]);
    if (rc) return rc;
    if (d_q[k] || nq[k]) return fail(HBH_ERR_ARG, "a side with a G2 set takes no Q table");
  }
  if (n == 0) return HBH_OK;
  if (!d_v) return fail(HBH_ERR_ARG, "null pointer");
  for (int k = 0; k < 2; k++) {
    if (set[k] ? !d_i[k] : !d_q[k]) return fail(HBH_ERR_ARG, "null pointer");
    if (!set[k] && !d_i[k] && nq[k] != n) return fail(HBH_ERR_ARG, "identity index map requires table size == n");
  }
  // the scope of hbh_verify_pairing_eq_dev: a side given by the call may still build a table
  EngineCall call(e, stream, false, EngineCall::PAIR_SLOT);
  if (call.rc) return call.rc;
  hbl::PairSideDesc sd[2];
  Resident res;
  for (int k = 0; k < 2; k++) {
    res.side[k] = set[k] != nullptr;
    sd[k] = set[k] ? set_side(set[k], d_p[k], d_i[k]) : hbl::PairSideDesc{d_p[k], d_q[k], nullptr, nullptr, d_i[k], nq[k]};
  }
  const int rc = run_pairing_sides(e, call.s, n, sd[0], sd[1], res, 1, d_v, nullptr, call.slot);
  if (rc) return rc;
  return call.finish();
}

}  // extern "C"

// ---------------------------------------------------------------- grouped random-combination share checks
// Opt-in forms of hbh_verify_sig_shares / hbh_verify_dec_shares (include/hbbft_hip.h): the items that
// share a table entry are settled by ONE pairing check on their random linear combination
// (group_plan.hpp plans the groups, k_rlc.hip sums them, k_rlc_digits.hip under the digit forms of the
// scalars); the items of a group whose check fails, and
// the items alone in their group, take the per-share check, so every reported 0 is exact.
#include <sys/random.h>

#include "group_digits.hpp"
#include "group_plan.hpp"

namespace {

constexpr size_t RLC_BYTES = 16;  // one scalar: 128 bits, a little-endian integer or the form's LE digits
static_assert(HBH_GFORM_INT128 == gd::FORM_INT128 && HBH_GFORM_X4 == gd::FORM_X4 && HBH_GFORM_X2 == gd::FORM_X2,
              "the ABI's forms are group_digits.hpp's");

bool rlc_is_zero(const uint8_t* r) {
  uint8_t o = 0;
  for (size_t k = 0; k < RLC_BYTES; k++) o |= r[k];
  return o == 0;
}

int os_random(uint8_t* out, size_t bytes) {
  while (bytes) {
    const ssize_t got = getrandom(out, bytes < 256 ? bytes : 256, 0);  // <= 256 B is never cut short
    if (got <= 0) return fail(HBH_ERR_DEVICE, "getrandom failed");
    out += got;
    bytes -= (size_t)got;
  }
  return HBH_OK;
}

// The n scalars of a call: the caller's (none may be zero), or n x 128 bits from the OS with a zero
// draw replaced.  The same in every form: the all-zero bytes are the zero integer and the all-zero tuple.
int rlc_scalars(size_t n, const uint8_t* given, std::vector<uint8_t>& r) {
  r.resize(n * RLC_BYTES);
  if (given) {
    std::memcpy(r.data(), given, r.size());
    for (size_t i = 0; i < n; i++)
      if (rlc_is_zero(&r[i * RLC_BYTES])) return fail(HBH_ERR_ARG, "zero scalar");
    return HBH_OK;
  }
  int rc = os_random(r.data(), r.size());
  for (size_t i = 0; i < n && !rc; i++)
    while (!rc && rlc_is_zero(&r[i * RLC_BYTES])) rc = os_random(&r[i * RLC_BYTES], RLC_BYTES);
  return rc;
}

// A plan's arrays and the scalars in device memory (e->in_b, e->in_a).  `packed` is the host image of
// the plan arrays: the caller keeps it until the stream has synchronised.
struct GroupDev {
  const uint32_t *perm, *tile_off, *tile_len, *ctile, *centry, *scalars;
  int ntile, ncomb, max_len;  // max_len: the longest tile
};
int upload_plan(hbh_engine* e, hipStream_t s, const GroupPlan& P, const std::vector<uint8_t>& scalars,
                std::vector<uint32_t>& packed, GroupDev& d) {
  const size_t n = P.perm.size(), nt = P.tile_off.size(), nc = P.comb.size();
  if (n > (size_t)1 << 30) return fail(HBH_ERR_ARG, "batch too large");
  packed.clear();
  packed.insert(packed.end(), P.perm.begin(), P.perm.end());
  packed.insert(packed.end(), P.tile_off.begin(), P.tile_off.end());
  packed.insert(packed.end(), P.tile_len.begin(), P.tile_len.end());
  packed.insert(packed.end(), P.ctile.begin(), P.ctile.end());
  for (uint32_t g : P.comb) packed.push_back(P.entry[g]);
  HBH_CHECK(upload(s, e->in_b, packed.data(), packed.size() * 4));
  HBH_CHECK(upload(s, e->in_a, scalars.data(), scalars.size()));
  d.perm = (const uint32_t*)e->in_b.p;
  d.tile_off = d.perm + n;
  d.tile_len = d.tile_off + nt;
  d.ctile = d.tile_len + nt;
  d.centry = d.ctile + nc + 1;
  d.scalars = (const uint32_t*)e->in_a.p;
  d.ntile = (int)nt;
  d.ncomb = (int)nc;
  d.max_len = 1;
  for (uint32_t len : P.tile_len) d.max_len = std::max(d.max_len, (int)len);
  return HBH_OK;
}

// out[c] = sum of r_i P_i over combined group c, for the n points d_pts (G1 or G2 ABI words); tile sums
// in `region` (0 / 1) of e->work, which the caller sized for two G2 regions.  form: HBH_GFORM_* of the
// scalars; the digit forms always run k_rlc_digits.hip, hbh_engine_set_group_sum_impl governs INT128 only.
int launch_group_sums(hbh_engine* e, hipStream_t s, bool g2, size_t n, const void* d_pts, const GroupDev& d, int region,
                      void* d_out, int form) {
  void* tiles = (uint8_t*)e->work.p + (size_t)region * d.ntile * hbl::group_tile_bytes(true);
  if (form != HBH_GFORM_INT128) {
    HBH_CHECK((g2 ? hbl::group_digits_g2 : hbl::group_digits_g1)(s, form, d.ntile, (int)n, d.max_len, d_pts, d.scalars,
                                                                 d.perm, d.tile_off, d.tile_len, tiles));
    HBH_CHECK((g2 ? hbl::group_join_g2 : hbl::group_join_g1)(s, d.ncomb, d.ctile, tiles, d_out));
    return HBH_OK;
  }
  // the form of this sum: forced, or AUTO by the items of the call (a threshold of 0: never BUCKET)
  const size_t bucket_min = g2 ? HBH_AUTO_GSUM_G2_BUCKET_MIN : HBH_AUTO_GSUM_G1_BUCKET_MIN;
  const bool bucket =
      e->gsum_impl == HBH_GSUM_BUCKET || (e->gsum_impl == HBH_GSUM_AUTO && bucket_min > 0 && n >= bucket_min);
  if (bucket)
    HBH_CHECK((g2 ? hbl::group_bucket_g2 : hbl::group_bucket_g1)(s, d.ntile, (int)n, d.max_len, d_pts, d.scalars, d.perm,
                                                                 d.tile_off, d.tile_len, tiles));
  else
    HBH_CHECK((g2 ? hbl::group_sum_g2 : hbl::group_sum_g1)(s, d.ntile, (int)n, d.max_len, d_pts, d.scalars, d.perm,
                                                          d.tile_off, d.tile_len, tiles));
  HBH_CHECK((g2 ? hbl::group_join_g2 : hbl::group_join_g1)(s, d.ncomb, d.ctile, tiles, d_out));
  return HBH_OK;
}

// The grouped check of one call.  a: the G1 points of side 1 (pk_i / D_i); b: sig_i (G2, dec = false)
// or pk_i (G1, dec = true); q1: the table of side 1 (H / H_uv); q2: W (dec only).
int run_grouped(hbh_engine* e, size_t n, const uint8_t* a, const uint8_t* b, bool dec, const uint8_t* q1,
                const uint8_t* q2, size_t ntab, const uint32_t* idx, const uint8_t* scalars, uint8_t* v,
                hbh_grouped_stats* stats) {
  if (stats) *stats = hbh_grouped_stats{0, 0, 0, 0};
  if (n == 0) return HBH_OK;
  if (!a || !b || !q1 || (dec && !q2) || !v) return fail(HBH_ERR_ARG, "null pointer");
  int rc = check_idx(idx, n, ntab);
  if (rc) return rc;
  std::vector<uint32_t> iota;
  if (!idx) {  // identity map: every item is alone in its group
    iota.resize(n);
    for (size_t i = 0; i < n; i++) iota[i] = (uint32_t)i;
    idx = iota.data();
  }
  GroupPlan P;
  if (!plan_groups(n, idx, ntab, 2, P)) return fail(HBH_ERR_ARG, "index out of range");
  std::vector<uint8_t> r;
  rc = rlc_scalars(n, scalars, r);
  if (rc) return rc;
  const size_t bsz = dec ? HBH_G1_BYTES : HBH_G2_BYTES;
  const size_t nc = P.comb.size();
  std::vector<uint8_t> gv(nc, 0);
  std::vector<uint32_t> packed;
  if (nc) {
    if (ntab > (size_t)1 << 30) return fail(HBH_ERR_ARG, "batch too large");
    EngineCall call(e, nullptr, true);
    if (call.rc) return call.rc;
    hipStream_t s = call.s;
    GroupDev d;
    rc = upload_plan(e, s, P, r, packed, d);
    if (rc) return rc;
    HBH_CHECK(upload(s, e->in_p1, a, n * HBH_G1_BYTES));
    HBH_CHECK(upload(s, dec ? e->in_p2 : e->in_d, b, n * bsz));
    HBH_CHECK(upload(s, e->in_q1, q1, ntab * HBH_G2_BYTES));
    if (dec) HBH_CHECK(upload(s, e->in_q2, q2, ntab * HBH_G2_BYTES));
    HBH_CHECK(e->work.ensure(2 * (size_t)d.ntile * hbl::group_tile_bytes(true)));
    HBH_CHECK(e->out_x.ensure(nc * HBH_G1_BYTES));
    HBH_CHECK(e->in_c.ensure(nc * bsz));
    HBH_CHECK(e->out_v.ensure(nc));
    {
      StageScope tm(e, s, HBH_STAGE_CURVE);
      // one residue r_i per item on both sides: X4 where a sum is in G2, X2 where both are in G1
      const int form = e->gscalar_form == HBH_GSCALAR_DIGITS ? (dec ? HBH_GFORM_X2 : HBH_GFORM_X4) : HBH_GFORM_INT128;
      rc = launch_group_sums(e, s, false, n, e->in_p1.p, d, 0, e->out_x.p, form);
      if (!rc) rc = launch_group_sums(e, s, !dec, n, dec ? e->in_p2.p : e->in_d.p, d, 1, e->in_c.p, form);
      if (rc) return rc;
    }
    // sig: e(sum r pk, H) == e(g1, sum r sig);  dec: e(sum r D, H_uv) == e(sum r pk, W)
    if (dec)
      rc = run_pairing_dev(e, s, nc, e->out_x.p, e->in_q1.p, ntab, d.centry, e->in_c.p, e->in_q2.p, ntab, d.centry, 1,
                           (uint8_t*)e->out_v.p);
    else
      rc = run_pairing_dev(e, s, nc, e->out_x.p, e->in_q1.p, ntab, d.centry, nullptr, e->in_c.p, nc, nullptr, 1,
                           (uint8_t*)e->out_v.p);
    if (rc) return rc;
    HBH_CHECK(download(s, gv.data(), e->out_v, nc));
    rc = call.finish();
    if (rc) return rc;
  }
  // exact verdicts for the failed groups and the singles: the per-share call on the gathered items
  std::vector<uint32_t> list;
  plan_fallback(P, gv.data(), list);
  if (stats) {
    stats->groups = (uint32_t)nc;
    for (uint8_t ok : gv) stats->groups_passed += ok ? 1 : 0;
    stats->singles = (uint32_t)P.singles.size();
    stats->fallback_items = (uint32_t)list.size();
  }
  std::memset(v, 1, n);
  const size_t m = list.size();
  if (!m) return HBH_OK;
  std::vector<uint8_t> ga(m * HBH_G1_BYTES), gb(m * bsz), fv(m, 0);
  std::vector<uint32_t> gi(m);
  for (size_t k = 0; k < m; k++) {
    std::memcpy(&ga[k * HBH_G1_BYTES], a + (size_t)list[k] * HBH_G1_BYTES, HBH_G1_BYTES);
    std::memcpy(&gb[k * bsz], b + (size_t)list[k] * bsz, bsz);
    gi[k] = idx[list[k]];
  }
  if (dec)
    rc = run_pairing_eq_host(e, m, ga.data(), q1, ntab, gi.data(), gb.data(), q2, ntab, gi.data(), fv.data());
  else
    rc = run_pairing_eq_host(e, m, ga.data(), q1, ntab, gi.data(), nullptr, gb.data(), m, nullptr, fv.data());
  if (rc) return rc;
  for (size_t k = 0; k < m; k++) v[list[k]] = fv[k];
  return HBH_OK;
}

}  // namespace

extern "C" {

int hbh_verify_sig_shares_grouped(hbh_engine* e, size_t n, const uint8_t* pks, const uint8_t* sigs,
                                  const uint8_t* hashes, size_t ndocs, const uint32_t* doc_idx, const uint8_t* scalars,
                                  uint8_t* v, hbh_grouped_stats* stats) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  return run_grouped(e, n, pks, sigs, false, hashes, nullptr, ndocs, doc_idx, scalars, v, stats);
}

int hbh_verify_dec_shares_grouped(hbh_engine* e, size_t n, const uint8_t* shares, const uint8_t* pks, const uint8_t* huv,
                                  const uint8_t* w, size_t ncts, const uint32_t* ct_idx, const uint8_t* scalars,
                                  uint8_t* v, hbh_grouped_stats* stats) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  return run_grouped(e, n, shares, pks, true, huv, w, ncts, ct_idx, scalars, v, stats);
}

int hbh_dbg_group_sums(hbh_engine* e, size_t n, const uint8_t* g1_pts, const uint8_t* g2_pts, size_t ngroups,
                       const uint32_t* group_idx, const uint8_t* scalars, uint8_t* out_g1, uint8_t* out_g2) {
  return hbh_dbg_group_sums_form(e, HBH_GFORM_INT128, n, g1_pts, g2_pts, ngroups, group_idx, scalars, out_g1, out_g2);
}

int hbh_dbg_group_sums_form(hbh_engine* e, int form, size_t n, const uint8_t* g1_pts, const uint8_t* g2_pts,
                            size_t ngroups, const uint32_t* group_idx, const uint8_t* scalars, uint8_t* out_g1,
                            uint8_t* out_g2) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (form != HBH_GFORM_INT128 && form != HBH_GFORM_X4 && form != HBH_GFORM_X2)
    return fail(HBH_ERR_ARG, "unknown group scalar form");
  if (form == HBH_GFORM_X2 && g2_pts) return fail(HBH_ERR_ARG, "the X2 form has no G2 sum");
  if ((g1_pts && !out_g1) || (g2_pts && !out_g2)) return fail(HBH_ERR_ARG, "null pointer");
  if (g1_pts) std::memset(out_g1, 0, ngroups * HBH_G1_BYTES);  // an absent entry sums to O
  if (g2_pts) std::memset(out_g2, 0, ngroups * HBH_G2_BYTES);
  if (n == 0) return HBH_OK;
  if (!group_idx || !scalars) return fail(HBH_ERR_ARG, "null pointer");
  GroupPlan P;
  if (!plan_groups(n, group_idx, ngroups, 1, P)) return fail(HBH_ERR_ARG, "index out of range");
  const std::vector<uint8_t> r(scalars, scalars + n * RLC_BYTES);
  const size_t nc = P.comb.size();
  std::vector<uint32_t> packed;
  std::vector<uint8_t> s1(g1_pts ? nc * HBH_G1_BYTES : 0), s2(g2_pts ? nc * HBH_G2_BYTES : 0);
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  GroupDev d;
  int rc = upload_plan(e, s, P, r, packed, d);
  if (rc) return rc;
  HBH_CHECK(e->work.ensure(2 * (size_t)d.ntile * hbl::group_tile_bytes(true)));
  StageScope tm(e, s, HBH_STAGE_CURVE);
  if (g1_pts) {
    HBH_CHECK(upload(s, e->in_p1, g1_pts, n * HBH_G1_BYTES));
    HBH_CHECK(e->out_x.ensure(nc * HBH_G1_BYTES));
    rc = launch_group_sums(e, s, false, n, e->in_p1.p, d, 0, e->out_x.p, form);
    if (rc) return rc;
    HBH_CHECK(download(s, s1.data(), e->out_x, s1.size()));
  }
  if (g2_pts) {
    HBH_CHECK(upload(s, e->in_d, g2_pts, n * HBH_G2_BYTES));
    HBH_CHECK(e->in_c.ensure(nc * HBH_G2_BYTES));
    rc = launch_group_sums(e, s, true, n, e->in_d.p, d, 1, e->in_c.p, form);
    if (rc) return rc;
    HBH_CHECK(download(s, s2.data(), e->in_c, s2.size()));
  }
  tm.stop();
  rc = call.finish();
  if (rc) return rc;
  for (size_t c = 0; c < nc; c++) {
    const size_t k = P.entry[P.comb[c]];
    if (g1_pts) std::memcpy(out_g1 + k * HBH_G1_BYTES, &s1[c * HBH_G1_BYTES], HBH_G1_BYTES);
    if (g2_pts) std::memcpy(out_g2 + k * HBH_G2_BYTES, &s2[c * HBH_G2_BYTES], HBH_G2_BYTES);
  }
  return HBH_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- batched independent checks
// Opt-in forms of hbh_verify_signatures / hbh_verify_ciphertexts_uv (include/hbbft_hip.h): the items share
// no G2 point, so a group of HBH_BATCH_GROUP items is settled by ONE final exponentiation over the product
// of its Miller values,
//   prod_i f(r_i A_i, H_i) * f(-C, sum_i r_i B_i),   A = pk / U, B = sig / W, H = hash_g2 / Q_bp, C = g1 / G1K
// (batch_plan.hpp plans the groups and tiles; k_scale_digits_g1 scales, the digit kernels of the grouped
// checks sum, k_*_miller_prod multiplies a tile's Miller values, the wave kernel adds the closing pair
// and runs the final exponentiation).  The items of a failed group and a single last item take the
// per-item check on the hashes already in HBM, so every reported 0 is exact.
#include "batch_plan.hpp"

namespace {

static_assert(HBH_BATCH_GROUP == BATCH_GROUP, "the ABI's group size is batch_plan.hpp's");

struct BatchWidth {
  hipError_t (*prod)(hipStream_t, int, int, const void*, const void*, int, int, uint32_t*);
  uint32_t lanes;
};

// The Miller-product kernel of a call: a forced PAIR / QUAD / OCT is honoured, every other setting takes
// AUTO's ladder read against the lane-kernel slots (two items per slot).  Call with e->mu held (inside the
// EngineCall).
BatchWidth batch_width(const hbh_engine* e, size_t slots) {
  int impl = e->impl;
  if (impl != HBH_IMPL_PAIR && impl != HBH_IMPL_QUAD && impl != HBH_IMPL_OCT)
    impl = slots <= HBH_AUTO_OCT_MAX ? HBH_IMPL_OCT : slots <= HBH_AUTO_QUAD_MAX ? HBH_IMPL_QUAD : HBH_IMPL_PAIR;
  if (impl == HBH_IMPL_OCT) return {hbl::oct_miller_prod, 8};
  if (impl == HBH_IMPL_QUAD) return {hbl::quad_miller_prod, 4};
  return {hbl::pair_miller_prod, 2};
}

// The tile products of the plan's groups over the device points d_p / d_q into value g * nf + t of
// e->fval (t < tiles per group; the caller fills the values above).
int launch_miller_prod(hbh_engine* e, hipStream_t s, const BatchPlan& B, const BatchWidth& w, const void* d_p,
                       const void* d_q, uint32_t nf) {
  const uint32_t tpg = batch_tiles_per_group(w.lanes);
  HBH_CHECK(w.prod(s, (int)batch_miller_tiles(B, w.lanes), (int)B.nitems, d_p, d_q, (int)tpg, (int)nf, (uint32_t*)e->fval.p));
  return HBH_OK;
}

// a: pk_i / U_i (G1); b: sig_i / W_i (G2); ct: Ciphertext::verify (the messages are V_i, hashed with U_i
// to Q_bp) instead of PublicKey::verify
int run_batched(hbh_engine* e, size_t n, const uint8_t* a, const uint8_t* b, bool ct, const uint8_t* data,
                const size_t* offsets, const uint8_t* scalars, uint8_t* v, hbh_grouped_stats* stats) {
  if (stats) *stats = hbh_grouped_stats{0, 0, 0, 0};
  if (n == 0) return HBH_OK;
  if (!a || !b || !v) return fail(HBH_ERR_ARG, "null pointer");
  int rc = check_msgs(n, data, offsets);
  if (rc) return rc;
  std::vector<uint8_t> r;
  rc = rlc_scalars(n, scalars, r);
  if (rc) return rc;
  BatchPlan B;
  plan_batch(n, 2, B);
  const size_t nc = B.ngroup;
  bool device;
  std::vector<uint8_t> g1k;
  {  // where the hash runs is settled before the call opens, as in the unbatched calls (the host form hashes first)
    std::lock_guard<std::mutex> lk(e->mu);
    device = hash_on_device(e, n);
    if (ct && e->g1k.empty()) {
      e->g1k.resize(HBH_G1_BYTES);
      rc = hbh_hash_bp_g1(e->g1k.data());
      if (rc) {
        e->g1k.clear();
        return fail(rc, hbh_host_last_error());
      }
    }
    if (ct) g1k = e->g1k;
  }
  const hbl::HashForm form = ct ? hbl::HASH_FORM_BP : hbl::HASH_FORM_FULL;
  // every host array a queued copy reads lives to the end of the call
  std::vector<uint8_t> h, seeds, state, fixed, gv(nc, 0), ga, gk, fv;
  std::vector<uint32_t> packed, list;
  if (!device) {
    h.resize(n * HBH_G2_BYTES);
    rc = ct ? hbh_hash_g1_g2_bp(n, a, data, offsets, h.data(), 0) : hbh_hash_g2(n, data, offsets, h.data(), 0);
    if (rc) return fail(rc, hbh_host_last_error());
  } else {
    seeds.resize(n * 32);
    state.resize(n);
    hbh__hash_seeds(n, ct ? a : nullptr, data, offsets, seeds.data());
  }
  EngineCall call(e, nullptr, true);  // holds e->mu
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  const BatchWidth w = batch_width(e, batch_slots(B));  // under the call's lock, as hbh_dbg_pairing_product
  // the hashes H_i / Q_i: in e->in_q1 for the group checks and the fallback alike
  if (!device) {
    HBH_CHECK(upload(s, e->in_q1, h.data(), n * HBH_G2_BYTES));
  } else {
    HBH_CHECK(upload(s, e->in_a, seeds.data(), n * 32));
    HBH_CHECK(e->in_q1.ensure(n * HBH_G2_BYTES));
    rc = launch_hash(e, s, n, (const uint8_t*)e->in_a.p, e->in_q1.p, form);
    if (rc) return rc;
    HBH_CHECK(download(s, state.data(), e->hash_state, n));
    HBH_CHECK(hipStreamSynchronize(s));
    const std::vector<uint32_t> left = hash_leftovers(state);
    if (!left.empty()) {  // host-hashed, then patched into the table
      fixed.resize(n * HBH_G2_BYTES);
      (ct ? hbh__hash_g2_bp_seeds : hbh__hash_g2_seeds)(left.size(), left.data(), seeds.data(), fixed.data());
      for (uint32_t i : left)
        HBH_CHECK(h2d(s, (uint8_t*)e->in_q1.p + (size_t)i * HBH_G2_BYTES, fixed.data() + (size_t)i * HBH_G2_BYTES,
                      HBH_G2_BYTES));
    }
  }
  HBH_CHECK(upload(s, e->in_p1, a, n * HBH_G1_BYTES));
  HBH_CHECK(upload(s, e->in_d, b, n * HBH_G2_BYTES));
  if (nc) {
    GroupDev d;
    rc = upload_plan(e, s, B.groups, r, packed, d);  // the seeds in e->in_a are spent: the stream was synchronised
    if (rc) return rc;
    const uint32_t tpg = batch_tiles_per_group(w.lanes), nf = tpg + 1;
    HBH_CHECK(e->work.ensure(2 * (size_t)d.ntile * hbl::group_tile_bytes(true)));
    HBH_CHECK(e->in_p2.ensure(n * HBH_G1_BYTES));
    HBH_CHECK(e->in_c.ensure(nc * HBH_G2_BYTES));
    HBH_CHECK(e->fval.ensure((nc * nf + nc) * 576));
    HBH_CHECK(e->out_x.ensure(nc * HBH_G1_BYTES));
    HBH_CHECK(e->out_v.ensure(nc));
    {
      StageScope tm(e, s, HBH_STAGE_CURVE);
      HBH_CHECK(hbl::scale_digits_g1(s, (int)B.nitems, e->in_p1.p, d.scalars, e->in_p2.p));
      rc = launch_group_sums(e, s, true, n, e->in_d.p, d, 0, e->in_c.p, HBH_GFORM_X4);
      if (rc) return rc;
    }
    if (ct) {  // the closing pair's G1K, one per group
      gk.resize(nc * HBH_G1_BYTES);
      for (size_t c = 0; c < nc; c++) std::memcpy(&gk[c * HBH_G1_BYTES], g1k.data(), HBH_G1_BYTES);
      HBH_CHECK(upload(s, e->in_q2, gk.data(), gk.size()));
    }
    {
      StageScope tm(e, s, HBH_STAGE_PAIRING);
      rc = launch_miller_prod(e, s, B, w, e->in_p2.p, e->in_q1.p, nf);
      if (rc) return rc;
      // the closing pair f(-C, S_c) of every group: side 0 inactive (P = O), side 1 negated; its values
      // land behind the tile values and move to slot tpg of their groups
      uint32_t* fin = (uint32_t*)e->fval.p;
      uint32_t* closing = fin + nc * nf * 144;
      HBH_CHECK(hipMemsetAsync(e->out_x.p, 0, nc * HBH_G1_BYTES, s));
      const hbl::PairSideDesc s0 = {e->out_x.p, e->in_c.p, nullptr, nullptr, nullptr, nc};
      const hbl::PairSideDesc s1 = {ct ? e->in_q2.p : nullptr, e->in_c.p, nullptr, nullptr, nullptr, nc};
      HBH_CHECK(hbl::wave_verify(s, (int)nc, s0, s1, hbl::WAVE_NEG_P2 | hbl::WAVE_MILLER_ONLY, nullptr, closing));
      HBH_CHECK(hipMemcpy2DAsync(fin + tpg * 144, (size_t)nf * 576, closing, 576, 576, nc, hipMemcpyDeviceToDevice, s));
      HBH_CHECK(hbl::wave_prod_fe(s, (int)nc, (int)nf, fin, (uint8_t*)e->out_v.p));
    }
    HBH_CHECK(download(s, gv.data(), e->out_v, nc));
    HBH_CHECK(hipStreamSynchronize(s));
  }
  plan_batch_fallback(B, gv.data(), list);
  if (stats) {
    stats->groups = (uint32_t)nc;
    for (uint8_t ok : gv) stats->groups_passed += ok ? 1 : 0;
    stats->singles = (uint32_t)B.groups.singles.size();
    stats->fallback_items = (uint32_t)list.size();
  }
  std::memset(v, 1, n);
  const size_t m = list.size();
  if (m) {
    // the per-item check of the unbatched call on the listed items: P gathered, Q through the index map
    // into the tables in HBM (n points each: no table is built for a map this sparse)
    ga.resize(m * HBH_G1_BYTES);
    fv.assign(m, 0);
    for (size_t k = 0; k < m; k++) std::memcpy(&ga[k * HBH_G1_BYTES], a + (size_t)list[k] * HBH_G1_BYTES, HBH_G1_BYTES);
    HBH_CHECK(upload(s, e->in_p2, ga.data(), ga.size()));
    HBH_CHECK(upload(s, e->in_i1, list.data(), m * 4));
    HBH_CHECK(e->out_v.ensure(m));
    const uint32_t* d_idx = (const uint32_t*)e->in_i1.p;
    if (ct) {  // e(G1K, W_i) == e(U_i, Q_i)
      gk.resize(m * HBH_G1_BYTES);
      for (size_t k = 0; k < m; k++) std::memcpy(&gk[k * HBH_G1_BYTES], g1k.data(), HBH_G1_BYTES);
      HBH_CHECK(upload(s, e->in_q2, gk.data(), gk.size()));
      rc = run_pairing_sides(e, s, m, {e->in_q2.p, e->in_d.p, nullptr, nullptr, d_idx, n},
                             {e->in_p2.p, e->in_q1.p, nullptr, nullptr, d_idx, n}, Resident(), 1, (uint8_t*)e->out_v.p);
    } else {  // e(pk_i, H_i) == e(g1, sig_i)
      rc = run_pairing_sides(e, s, m, {e->in_p2.p, e->in_q1.p, nullptr, nullptr, d_idx, n},
                             {nullptr, e->in_d.p, nullptr, nullptr, d_idx, n}, Resident(), 1, (uint8_t*)e->out_v.p);
    }
    if (rc) return rc;
    HBH_CHECK(download(s, fv.data(), e->out_v, m));
  }
  rc = call.finish();
  if (rc) return rc;
  for (size_t k = 0; k < m; k++) v[list[k]] = fv[k];
  return HBH_OK;
}

}  // namespace

extern "C" {

int hbh_verify_signatures_batched(hbh_engine* e, size_t n, const uint8_t* pks, const uint8_t* sigs, const uint8_t* data,
                                  const size_t* offsets, const uint8_t* scalars, uint8_t* v, hbh_grouped_stats* stats) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  return run_batched(e, n, pks, sigs, false, data, offsets, scalars, v, stats);
}

int hbh_verify_ciphertexts_uv_batched(hbh_engine* e, size_t n, const uint8_t* u, const uint8_t* data,
                                      const size_t* offsets, const uint8_t* w, const uint8_t* scalars, uint8_t* v,
                                      hbh_grouped_stats* stats) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  return run_batched(e, n, u, w, true, data, offsets, scalars, v, stats);
}

int hbh_dbg_pairing_product(hbh_engine* e, size_t n, const uint8_t* p, const uint8_t* q, uint8_t* out) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (n == 0) return HBH_OK;
  if (!p || !q || !out) return fail(HBH_ERR_ARG, "null pointer");
  if (n > (size_t)1 << 26) return fail(HBH_ERR_ARG, "batch too large");
  BatchPlan B;
  plan_batch(n, 1, B);
  const size_t nc = B.ngroup;
  EngineCall call(e, nullptr, true);  // holds e->mu
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  const BatchWidth w = batch_width(e, batch_slots(B));
  const uint32_t tpg = batch_tiles_per_group(w.lanes);
  HBH_CHECK(upload(s, e->in_p1, p, n * HBH_G1_BYTES));
  HBH_CHECK(upload(s, e->in_q1, q, n * HBH_G2_BYTES));
  HBH_CHECK(e->fval.ensure(nc * tpg * 576));
  HBH_CHECK(e->out_v.ensure(nc * 576));
  {
    StageScope tm(e, s, HBH_STAGE_PAIRING);
    const int rc = launch_miller_prod(e, s, B, w, e->in_p1.p, e->in_q1.p, tpg);
    if (rc) return rc;
    HBH_CHECK(hbl::wave_prod_fe(s, (int)nc, (int)tpg, (const uint32_t*)e->fval.p, nullptr, (uint32_t*)e->out_v.p,
                                hbl::WAVE_CONJ_VALUE));
  }
  HBH_CHECK(download(s, out, e->out_v, nc * 576));
  return call.finish();
}

}  // extern "C"
