// The pairing checks of the C ABI: which kernel a call takes, the line tables of shared G2 sides, the
// host-pointer and device-pointer calls, and the device-resident G2 sets.
#include "constants.hpp"  // the field modulus, for hbh_g2_set_add's canonical-coordinate check
#include "engine_impl.hpp"

using namespace hbe;

namespace {

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

int g2_set_call_check(const hbh_g2_set* gs) {
  if (!gs) return fail(HBH_ERR_ARG, "null G2 set");
  if (!gs->e) return fail(HBH_ERR_ARG, "G2 set detached: its engine was destroyed");
  return HBH_OK;
}

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

}  // namespace

int hbe::run_pairing_sides(hbh_engine* e, hipStream_t s, size_t n, const hbl::PairSideDesc& d1,
                           const hbl::PairSideDesc& d2, const Resident& res, int flags, uint8_t* d_v, uint32_t* d_value,
                           int slot) {
  if (n == 0) return HBH_OK;
  if (n > (size_t)1 << 30 || d1.nq > (size_t)1 << 30 || d2.nq > (size_t)1 << 30) return fail(HBH_ERR_ARG, "batch too large");
  return launch_pair(e, s, resolve_impl(e, n), n, d1, d2, res, flags, d_v, d_value, slot);
}

int hbe::run_pairing_dev(hbh_engine* e, hipStream_t s, size_t n, const void* d_p1, const void* d_q1, size_t nq1,
                         const uint32_t* d_i1, const void* d_p2, const void* d_q2, size_t nq2, const uint32_t* d_i2,
                         int flags, uint8_t* d_v, uint32_t* d_value, int slot) {
  return run_pairing_sides(e, s, n, {d_p1, d_q1, nullptr, nullptr, d_i1, nq1}, {d_p2, d_q2, nullptr, nullptr, d_i2, nq2},
                           Resident(), flags, d_v, d_value, slot);
}

int hbe::check_idx(const uint32_t* idx, size_t n, size_t table) {
  if (!idx) return table == n ? HBH_OK : fail(HBH_ERR_ARG, "identity index map requires table size == n");
  for (size_t i = 0; i < n; i++)
    if (idx[i] >= table) return fail(HBH_ERR_ARG, "index out of range");
  return HBH_OK;
}

int hbe::run_pairing_eq_host(hbh_engine* e, size_t n, const uint8_t* p1, const uint8_t* q1, size_t nq1,
                             const uint32_t* i1, const uint8_t* p2, const uint8_t* q2, size_t nq2, const uint32_t* i2,
                             uint8_t* v, hbh_g2_set* set1, hbh_g2_set* set2) {
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

void hbe::release_g2_set_device(hbh_g2_set* gs) {
  if (gs->mem) (void)hipFree(gs->mem);
  gs->mem = gs->lines = gs->q = nullptr;
  gs->qinf = nullptr;
  gs->slots.reset(0);
  gs->e = nullptr;
}

extern "C" {

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

// ---------------------------------------------------------------- device-resident G2 sets
// The G2 point every share of an instance is checked against -- H of a ThresholdSign document
// (src/threshold_sign.rs:223), H_uv and W of a ThresholdDecrypt ciphertext (src/threshold_decrypt.rs:227)
// -- lives as long as the instance and is read by every drain that verifies its shares: a set keeps
// such points prepared in HBM (line table, affine point, infinity byte per slot), so a drain names
// slots and its verify kernel starts without the serial table walk (k_oct_prep).

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
