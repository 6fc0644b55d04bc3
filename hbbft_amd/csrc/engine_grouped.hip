// The random-combination checks of the C ABI.
//
// Grouped share checks, opt-in forms of hbh_verify_sig_shares / hbh_verify_dec_shares (include/hbbft_hip.h):
// the items that share a table entry are settled by ONE pairing check on their random linear combination
// (group_plan.hpp plans the groups, k_rlc.hip sums them, k_rlc_digits.hip under the digit forms of the
// scalars); the items of a group whose check fails, and the items alone in their group, take the
// per-share check, so every reported 0 is exact.
//
// Batched independent checks, opt-in forms of hbh_verify_signatures / hbh_verify_ciphertexts_uv: the items
// share no G2 point, so a group of HBH_BATCH_GROUP items is settled by ONE final exponentiation over the
// product of its Miller values,
//   prod_i f(r_i A_i, H_i) * f(-C, sum_i r_i B_i),   A = pk / U, B = sig / W, H = hash_g2 / Q_bp, C = g1 / G1K
// (batch_plan.hpp plans the groups and tiles; k_scale_digits_g1 scales, the digit kernels of the grouped
// checks sum, k_*_miller_prod multiplies a tile's Miller values, the wave kernel adds the closing pair
// and runs the final exponentiation).  The items of a failed group and a single last item take the
// per-item check on the hashes already in HBM, so every reported 0 is exact.
#include <sys/random.h>

#include "batch_plan.hpp"
#include "engine_impl.hpp"
#include "group_digits.hpp"
#include "group_plan.hpp"

using namespace hbe;

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
  // the form of an INT128 sum: forced, or AUTO by the items of the call (a threshold of 0: never BUCKET)
  const size_t bucket_min = g2 ? HBH_AUTO_GSUM_G2_BUCKET_MIN : HBH_AUTO_GSUM_G1_BUCKET_MIN;
  if (form != HBH_GFORM_INT128)
    HBH_CHECK((g2 ? hbl::group_digits_g2 : hbl::group_digits_g1)(s, form, d.ntile, (int)n, d.max_len, d_pts, d.scalars,
                                                                 d.perm, d.tile_off, d.tile_len, tiles));
  else if (e->gsum_impl == HBH_GSUM_BUCKET || (e->gsum_impl == HBH_GSUM_AUTO && bucket_min > 0 && n >= bucket_min))
    HBH_CHECK((g2 ? hbl::group_bucket_g2 : hbl::group_bucket_g1)(s, d.ntile, (int)n, d.max_len, d_pts, d.scalars, d.perm,
                                                                 d.tile_off, d.tile_len, tiles));
  else
    HBH_CHECK((g2 ? hbl::group_sum_g2 : hbl::group_sum_g1)(s, d.ntile, (int)n, d.max_len, d_pts, d.scalars, d.perm,
                                                          d.tile_off, d.tile_len, tiles));
  HBH_CHECK((g2 ? hbl::group_join_g2 : hbl::group_join_g1)(s, d.ncomb, d.ctile, tiles, d_out));
  return HBH_OK;
}

// what a grouped or batched call reports: its group verdicts gv, its single items, its fallback list
void fill_stats(hbh_grouped_stats* stats, const std::vector<uint8_t>& gv, size_t singles, const std::vector<uint32_t>& list) {
  if (!stats) return;
  *stats = hbh_grouped_stats{(uint32_t)gv.size(), 0, (uint32_t)singles, (uint32_t)list.size()};
  for (uint8_t ok : gv) stats->groups_passed += ok ? 1 : 0;
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
  fill_stats(stats, gv, P.singles.size(), list);
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
  // where the hash runs is settled before the call opens, as in the unbatched calls (the host form hashes first)
  const bool device = hash_runs_on_device(e, n);
  std::vector<uint8_t> g1k;
  if (ct) rc = engine_g1k(e, g1k);
  if (rc) return rc;
  // every host array a queued copy reads lives to the end of the call
  HashStage st;
  std::vector<uint8_t> h, gv(nc, 0), ga, gk, fv;
  std::vector<uint32_t> packed, list;
  if (!device) {
    h.resize(n * HBH_G2_BYTES);
    rc = ct ? hbh_hash_g1_g2_bp(n, a, data, offsets, h.data(), 0) : hbh_hash_g2(n, data, offsets, h.data(), 0);
    if (rc) return fail(rc, hbh_host_last_error());
  } else {
    st.seeds.resize(n * 32);
    hbh__hash_seeds(n, ct ? a : nullptr, data, offsets, st.seeds.data());
  }
  EngineCall call(e, nullptr, true);  // holds e->mu
  if (call.rc) return call.rc;
  hipStream_t s = call.s;
  const BatchWidth w = batch_width(e, batch_slots(B));  // under the call's lock, as hbh_dbg_pairing_product
  // the hashes H_i / Q_i: in e->in_q1 for the group checks and the fallback alike
  if (!device)
    HBH_CHECK(upload(s, e->in_q1, h.data(), n * HBH_G2_BYTES));
  else
    rc = hash_to_table(e, s, n, ct ? hbl::HASH_FORM_BP : hbl::HASH_FORM_FULL, e->in_q1, st);
  if (rc) return rc;
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
  fill_stats(stats, gv, B.groups.singles.size(), list);
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
