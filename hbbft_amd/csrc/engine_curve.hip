// The curve calls of the C ABI: multiplications, interpolation and the combine-and-verify master check
// (with its split form), rows and evaluations of commitments, the Ack check on uploaded commitments, the
// point decoders, and the device-pointer forms of these.
#include "engine_impl.hpp"
#include "interp_pair.hpp"
#include "wire.hpp"
// host arithmetic and planning (no HIP, tested on the CPU: tests/test_engine_host.py)
#include "ack_plan.hpp"
#include "host_fr.hpp"
#include "wire_host.hpp"

extern "C" int hbh__host_g1_neg(const uint8_t* pk, uint8_t* neg_out);  // host_hash.cpp, not part of the public ABI

using namespace hbe;

int hbe::ensure_fbtab(hbh_engine* e, hipStream_t s) {
  if (e->fbtab_ready) return HBH_OK;
  HBH_CHECK(e->fbtab.ensure(hbl::fb_table_bytes()));
  HBH_CHECK(hbl::fb_table(s, e->fbtab.p));
  e->fbtab_ready = true;
  return HBH_OK;
}

// split master check when the call has at most split_waves_max(t) one-pair Miller waves
// (ncomb x (t + 2)).  Crossover against interpolate-then-verify, interpolated linearly between the
// measured batch sizes of profiles/r03/split_sweep_auto.jsonl: t = 21 at ~45 combines (~1,046 waves;
// 32 combines split 2.81 vs 3.60 ms, 48 combines 3.80 vs 3.70 ms), t = 33 at ~38 combines (~1,340
// waves; 33 combines 4.26 vs 4.66 ms, 40 combines 4.75 vs 4.59 ms).  One wave cap cannot fit both
// (ADVICE r3), so the cap grows with t through those two points: 540 + 24 t.
// HBH_SPLIT_MAX=<combines> in the environment replaces the rule by a plain combine count (A/B).
inline size_t split_waves_max(int t) { return 540 + 24 * (size_t)t; }

namespace {

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

// xs[k] = idx[k] + 1: the x of node idx as a small Fr integer (threshold_crypto into_fr_plus_1)
int plus_one(const uint32_t* idx, size_t count, std::vector<uint32_t>& xs) {
  xs.resize(count);
  for (size_t k = 0; k < count; k++) {
    if (idx[k] == 0xffffffffu) return fail(HBH_ERR_ARG, "node index out of range");
    xs[k] = idx[k] + 1;
  }
  return HBH_OK;
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
  std::vector<uint32_t> xs;
  rc = plus_one(idx, ncomb * m, xs);
  if (rc) return rc;
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

// ---------------------------------------------------------------- device-resident variants
// Inputs and outputs in device memory, asynchronous on `stream` (NULL = engine stream), ordered
// after the engine's previous call like hbh_verify_pairing_eq_dev.
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
  std::vector<uint32_t> xs;
  rc = plus_one(idx, ncomb * m, xs);
  if (rc) return rc;
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
