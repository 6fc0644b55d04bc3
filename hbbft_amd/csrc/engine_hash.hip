// Hashing to G2 on the device (k_hash.hip, k_hash_quad.hip) and the calls that hash their messages there:
// the engine forms of hash_g2 / hash_g1_g2, PublicKey::verify and Ciphertext::verify from the messages,
// and encryption.
#include "engine_impl.hpp"

// host_hash.cpp, not part of the public ABI: the curve half of hash_g2 from one seed, out[which[k]] =
// the point of that seed; the same for the Q form (hbh_hash_g1_g2_bp's bytes)
extern "C" void hbh__hash_g2_seeds(size_t n, const uint32_t* which, const uint8_t* seeds, uint8_t* out);
extern "C" void hbh__hash_g2_bp_seeds(size_t n, const uint32_t* which, const uint8_t* seeds, uint8_t* out);

using namespace hbe;

int hbe::check_msgs(size_t n, const uint8_t* data, const size_t* offsets) {
  if (!offsets || (!data && offsets[n] != 0)) return fail(HBH_ERR_ARG, "null pointer");
  for (size_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i]) return fail(HBH_ERR_ARG, "offsets not ascending");
  if (n > (size_t)1 << 26) return fail(HBH_ERR_ARG, "batch too large");
  return HBH_OK;
}

bool hbe::hash_runs_on_device(hbh_engine* e, size_t n) {
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->hash_impl != HBH_HASH_AUTO) return e->hash_impl == HBH_HASH_DEVICE;
  return HBH_AUTO_HASH_DEVICE_MIN != 0 && n >= HBH_AUTO_HASH_DEVICE_MIN;
}

int hbe::engine_g1k(hbh_engine* e, std::vector<uint8_t>& out) {
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->g1k.empty()) {
    e->g1k.resize(HBH_G1_BYTES);
    const int rc = hbh_hash_bp_g1(e->g1k.data());
    if (rc) {
      e->g1k.clear();
      return fail(rc, hbh_host_last_error());
    }
  }
  out = e->g1k;
  return HBH_OK;
}

namespace {

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

// the host stage's points of those messages, at their indices of out (the other entries stay)
void hash_on_host(const std::vector<uint32_t>& left, const std::vector<uint8_t>& seeds, hbl::HashForm form, uint8_t* out) {
  if (left.empty()) return;
  (form == hbl::HASH_FORM_BP ? hbh__hash_g2_bp_seeds : hbh__hash_g2_seeds)(left.size(), left.data(), seeds.data(), out);
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
  hash_on_host(hash_leftovers(state), seeds, form, out);
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
  if (!hash_runs_on_device(e, n)) {
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

int hbe::hash_to_table(hbh_engine* e, hipStream_t s, size_t n, hbl::HashForm form, DevBuf& dst, HashStage& st) {
  st.state.resize(n);
  HBH_CHECK(upload(s, e->in_a, st.seeds.data(), n * 32));
  HBH_CHECK(dst.ensure(n * HBH_G2_BYTES));
  const int rc = launch_hash(e, s, n, (const uint8_t*)e->in_a.p, dst.p, form);
  if (rc) return rc;
  HBH_CHECK(download(s, st.state.data(), e->hash_state, n));
  HBH_CHECK(hipStreamSynchronize(s));
  const std::vector<uint32_t> left = hash_leftovers(st.state);
  if (!left.empty()) st.fixed.resize(n * HBH_G2_BYTES);
  hash_on_host(left, st.seeds, form, st.fixed.data());
  for (uint32_t i : left)  // patched into the table
    HBH_CHECK(h2d(s, (uint8_t*)dst.p + (size_t)i * HBH_G2_BYTES, st.fixed.data() + (size_t)i * HBH_G2_BYTES, HBH_G2_BYTES));
  return HBH_OK;
}

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
  if (!hash_runs_on_device(e, n)) {
    std::vector<uint8_t> h(n * HBH_G2_BYTES);
    rc = hbh_hash_g2(n, data, offsets, h.data(), 0);
    if (rc) return fail(rc, hbh_host_last_error());
    return run_pairing_eq_host(e, n, pks, h.data(), n, nullptr, nullptr, sigs, n, nullptr, v);
  }
  HashStage st;
  st.seeds.resize(n * 32);
  hbh__hash_seeds(n, nullptr, data, offsets, st.seeds.data());
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  // the hashes are written straight into the Q1 staging buffer of the pairing path and stay in HBM
  rc = hash_to_table(e, s, n, hbl::HASH_FORM_FULL, e->in_q1, st);
  if (rc) return rc;
  HBH_CHECK(upload(s, e->in_p1, pks, n * HBH_G1_BYTES));
  HBH_CHECK(upload(s, e->in_q2, sigs, n * HBH_G2_BYTES));
  HBH_CHECK(e->out_v.ensure(n));
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
  const bool device = hash_runs_on_device(e, n);
  std::vector<uint8_t> k, g1k(n * HBH_G1_BYTES);  // P1 = G1K for every check
  rc = engine_g1k(e, k);
  if (rc) return rc;
  for (size_t i = 0; i < n; i++) std::memcpy(g1k.data() + i * HBH_G1_BYTES, k.data(), HBH_G1_BYTES);
  // e(G1K, W) == e(U, Q_bp): sides as Engine.verify_ciphertexts_bp's (P1 = G1K, Q1 = W, P2 = U, Q2 = Q)
  if (!device) {
    std::vector<uint8_t> q(n * HBH_G2_BYTES);
    rc = hbh_hash_g1_g2_bp(n, u, data, offsets, q.data(), 0);
    if (rc) return fail(rc, hbh_host_last_error());
    return run_pairing_eq_host(e, n, g1k.data(), w, n, nullptr, u, q.data(), n, nullptr, v);
  }
  HashStage st;
  st.seeds.resize(n * 32);
  hbh__hash_seeds(n, u, data, offsets, st.seeds.data());
  EngineCall call(e, nullptr, true);
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  // the Q_bp are written straight into the Q2 staging buffer of the pairing path and stay in HBM
  rc = hash_to_table(e, s, n, hbl::HASH_FORM_BP, e->in_q2, st);
  if (rc) return rc;
  HBH_CHECK(upload(s, e->in_p1, g1k.data(), n * HBH_G1_BYTES));
  HBH_CHECK(upload(s, e->in_q1, w, n * HBH_G2_BYTES));
  HBH_CHECK(upload(s, e->in_p2, u, n * HBH_G1_BYTES));
  HBH_CHECK(e->out_v.ensure(n));
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
  if (!hash_runs_on_device(e, n)) {
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
