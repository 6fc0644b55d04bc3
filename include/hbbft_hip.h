/* hbbft_hip.h -- C ABI of the MI355X batch engine for hbbft's BLS12-381 threshold-crypto hot path.
 *
 * This is the drop-in boundary.  hbbft itself never calls curve arithmetic: its
 * three protocol modules call `threshold_crypto` 0.3 methods synchronously, one share at a time.
 * Each entry point below is the batched replacement for one of those calls; a Rust binding
 *  drains the shares a `Step` would verify into one call.
 *
 * Conventions
 *  - Plain pointers + sizes, caller-owned buffers, nothing retained after return.
 *  - Points are affine, canonical (non-Montgomery) little-endian integers:
 *      G1 = x(48 B) || y(48 B)                         (HBH_G1_BYTES = 96)
 *      G2 = x.c0 || x.c1 || y.c0 || y.c1 (48 B each)   (HBH_G2_BYTES = 192)
 *    The point at infinity is all-zero bytes.  Points must be on the curve and in the prime-order
 *    subgroup, as threshold_crypto's deserialisation guarantees for every point that reaches the
 *    reference's verify calls; the engine does not re-check membership.
 *  - Scalars (Fr) are 32-byte little-endian canonical integers.
 *  - Verdicts are one byte per item (1 = valid, 0 = invalid), never an error: an invalid share is
 *    a Fault in hbbft, not an Err (src/threshold_sign.rs:191-194, src/threshold_decrypt.rs:192-195).
 *  - Every function returns an hbh_status; HBH_OK = 0.
 *  - `_dev` variants take device pointers (HBM-resident inputs) and an optional hipStream_t
 *    (passed as void*, NULL = the engine's stream); they are asynchronous on that stream.
 *  - One engine handle binds one GPU.  Calls on one handle are serialised by the handle's mutex;
 *    distinct handles may be used from distinct threads.
 */
#ifndef HBBFT_HIP_H
#define HBBFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HBH_G1_BYTES 96
#define HBH_G2_BYTES 192
#define HBH_FR_BYTES 32

typedef enum {
  HBH_OK = 0,
  HBH_ERR_ARG = 1,       /* null pointer / size out of range / index out of range */
  HBH_ERR_DEVICE = 2,    /* HIP runtime error (message via hbh_last_error) */
  HBH_ERR_NOMEM = 3,     /* device allocation failed */
  HBH_ERR_NOT_ENOUGH_SHARES = 4,  /* threshold_crypto Error::NotEnoughShares */
  HBH_ERR_DUPLICATE_ENTRY = 5     /* threshold_crypto Error::DuplicateEntry */
} hbh_status;

typedef struct hbh_engine hbh_engine;

/* Engine lifetime.  `device` is a HIP device ordinal. */
int hbh_engine_create(int device, hbh_engine** out);
int hbh_engine_destroy(hbh_engine* eng);
/* Last error message of this thread (static storage, never NULL). */
const char* hbh_last_error(void);
/* Number of HIP devices visible to this process. */
int hbh_device_count(int* out);

/* ---------------------------------------------------------------- device-resident variants
 * Same results as the host-pointer calls, with every array in device memory (HBM) and the call
 * asynchronous on `stream` (hipStream_t as void*, NULL = engine stream); ordered after the
 * engine's previous call as hbh_verify_pairing_eq_dev.  Index arrays are not inspected on the host.
 *   hbh_interpolate_g*_dev: d_idx node indices (x = idx + 1; an index of 0xffffffff gives status
 *     HBH_ERR_ARG for its combine), d_status written per combine as hbh_interpolate_g*.
 *   hbh_g*_decompress_dev: compressed encodings in HBM, flags parsed on the device.
 *   hbh_bivar_ack_check_dev: the caller supplies the row plan -- nrow distinct (part, x) requests
 *     (d_row_part, d_row_x, part < nparts of d_commits) and d_row_of[a] = the row of ack a -- that
 *     hbh_bivar_ack_check derives on the host; d_vals = 32-byte LE scalars. */
int hbh_interpolate_g1_dev(hbh_engine* eng, void* stream, size_t ncomb, int t, const uint32_t* d_idx,
                           const void* d_pts, void* d_out, int* d_status);
int hbh_interpolate_g2_dev(hbh_engine* eng, void* stream, size_t ncomb, int t, const uint32_t* d_idx,
                           const void* d_pts, void* d_out, int* d_status);
int hbh_g1_decompress_dev(hbh_engine* eng, void* stream, size_t n, const uint8_t* d_in, void* d_out, uint8_t* d_ok);
int hbh_g2_decompress_dev(hbh_engine* eng, void* stream, size_t n, const uint8_t* d_in, void* d_out, uint8_t* d_ok);
int hbh_bivar_ack_check_dev(hbh_engine* eng, void* stream, size_t nack, int t, const void* d_commits, size_t nrow,
                            const uint32_t* d_row_part, const uint32_t* d_row_x, const uint32_t* d_row_of,
                            const uint32_t* d_ys, const void* d_vals, uint8_t* d_verdicts);

/* ---------------------------------------------------------------- engine pool (multi-device)
 * One engine per shard; devices[s] is shard s's device (a device may appear more than once: each
 * shard has its own stream and workspaces).  A pool call splits its batch by INSTANCE (document /
 * ciphertext / combine / SyncKeyGen part) into contiguous instance ranges of about equal item
 * counts, runs every shard on its own host thread, and writes verdicts and points back in the
 * caller's order -- byte-identical to the single-engine call.  No cross-device collective exists
 * on this path.  Errors: the first failing shard's code, with "shard s: ..." in
 * hbh_last_error.  Replaces the reference's single synchronous verifier per node
 * (src/traits.rs:297-336) with a node-wide fan-out over the GPUs of one host. */
typedef struct hbh_pool hbh_pool;
int hbh_pool_create(const int* devices, int nshards, hbh_pool** out);
int hbh_pool_destroy(hbh_pool* pool);
int hbh_pool_shards(const hbh_pool* pool, int* out);
int hbh_pool_engine(hbh_pool* pool, int shard, hbh_engine** out);
int hbh_pool_set_pairing_impl(hbh_pool* pool, int impl);
int hbh_pool_verify_sig_shares(hbh_pool* pool, size_t n, const uint8_t* pks, const uint8_t* sigs,
                               const uint8_t* hashes, size_t ndocs, const uint32_t* doc_idx, uint8_t* verdicts);
int hbh_pool_verify_dec_shares(hbh_pool* pool, size_t n, const uint8_t* shares, const uint8_t* pks,
                               const uint8_t* huv, const uint8_t* w, size_t ncts, const uint32_t* ct_idx,
                               uint8_t* verdicts);
int hbh_pool_combine_verify_g2(hbh_pool* pool, size_t ncomb, int t, const uint32_t* idx, const uint8_t* shares,
                               const uint8_t* master_pk, const uint8_t* hashes, uint8_t* out, int* status,
                               uint8_t* verdicts);
int hbh_pool_interpolate_g1(hbh_pool* pool, size_t ncomb, int t, const uint32_t* idx, const uint8_t* pts,
                            uint8_t* out, int* status);
int hbh_pool_bivar_ack_check(hbh_pool* pool, size_t nack, int t, size_t nparts, const uint8_t* commits,
                             const uint32_t* part_idx, const uint32_t* xs, const uint32_t* ys, const uint8_t* vals,
                             uint8_t* verdicts);

/* ---------------------------------------------------------------- pairing-equality checks
 * Generic batched check  e(P1[i], Q1[q1_idx[i]]) == e(P2[i], Q2[q2_idx[i]])  for i < n,
 * computed as one 2-pair multi-Miller loop + one final exponentiation per item.
 * Q tables hold the G2 points shared by many items (H per document, W / H_uv per ciphertext);
 * q*_idx == NULL means the identity map (table size must then be n).
 * Replaces every pairing comparison on the path:
 *   PublicKeyShare::verify_g2   (src/threshold_sign.rs:223)   P1=pk_i, Q1=H, P2=g1, Q2=sig_i
 *   PublicKey::verify_g2        (src/threshold_sign.rs:264)   P1=pk,   Q1=H, P2=g1, Q2=sig
 *   PublicKey::verify (signed votes / key-gen messages, src/dynamic_honey_badger/votes.rs:157,
 *     dynamic_honey_badger.rs:520)                                P1=pk,   Q1=hash_g2(msg), P2=g1, Q2=sig
 *   Ciphertext::verify          (src/threshold_decrypt.rs:142) P1=g1, Q1=W, P2=U, Q2=H_uv
 *   verify_decryption_share     (src/threshold_decrypt.rs:227) P1=D_i, Q1=H_uv, P2=pk_i, Q2=W
 */
int hbh_verify_pairing_eq(hbh_engine* eng, size_t n,
                          const uint8_t* p1, const uint8_t* q1_table, size_t nq1, const uint32_t* q1_idx,
                          const uint8_t* p2, const uint8_t* q2_table, size_t nq2, const uint32_t* q2_idx,
                          uint8_t* verdicts);

/* PublicKeyShare::verify_g2(share, hash) batched (src/threshold_sign.rs:216-225):
 *   verdict[i] = e(pk[i], hashes[doc_idx[i]]) == e(g1, sigs[i]). */
int hbh_verify_sig_shares(hbh_engine* eng, size_t n, const uint8_t* pks, const uint8_t* sigs,
                          const uint8_t* hashes, size_t ndocs, const uint32_t* doc_idx, uint8_t* verdicts);

/* PublicKeyShare::verify_decryption_share(share, ct) batched (src/threshold_decrypt.rs:220-229):
 *   verdict[i] = e(D[i], huv[ct_idx[i]]) == e(pk[i], w[ct_idx[i]]);
 * huv = hash_g1_g2(U, V) is computed once per ciphertext on the host (the reference recomputes it
 * per check, SURVEY §8a a8 -- the value is identical). */
int hbh_verify_dec_shares(hbh_engine* eng, size_t n, const uint8_t* shares, const uint8_t* pks,
                          const uint8_t* huv, const uint8_t* w, size_t ncts, const uint32_t* ct_idx,
                          uint8_t* verdicts);

/* Ciphertext::verify batched (src/threshold_decrypt.rs:142): verdict[i] = e(g1, w[i]) == e(u[i], huv[i]). */
int hbh_verify_ciphertexts(hbh_engine* eng, size_t n, const uint8_t* u, const uint8_t* w,
                           const uint8_t* huv, uint8_t* verdicts);

/* Device-pointer variant of hbh_verify_pairing_eq (inputs already in HBM).  Asynchronous on
 * `stream` (hipStream_t as void*, NULL = engine stream).  d_p1 / d_p2 == NULL means the G1
 * generator for every item (PublicKeyShare::verify_g2 has P2 = g1, Ciphertext::verify P1 = g1).
 * Calls on different streams are ordered by the engine (each call waits for the previous call's
 * device work before reusing the engine's workspaces).  Index arrays live in device memory and are
 * not inspected on the host: an index >= its table size yields verdict 0 (both implementations). */
int hbh_verify_pairing_eq_dev(hbh_engine* eng, void* stream, size_t n,
                              const void* d_p1, const void* d_q1_table, size_t nq1, const uint32_t* d_q1_idx,
                              const void* d_p2, const void* d_q2_table, size_t nq2, const uint32_t* d_q2_idx,
                              uint8_t* d_verdicts);

/* Device-resident prepared G2 points (the counterpart of pairing's G2Prepared).  The shared G2 point
 * of an instance -- H = hash_g2(doc) of a ThresholdSign document (src/threshold_sign.rs:223), H_uv and
 * W of a ThresholdDecrypt ciphertext (src/threshold_decrypt.rs:227) -- outlives the drains that verify
 * shares against it.  A G2 set prepares such a point once into HBM (its Miller-loop line table, its
 * affine point and its infinity byte: 24,129 B per slot) and calls name it by slot afterwards, so a
 * call builds no line table for that side (no HBH_STAGE_PREPARE launch) and uploads no G2 bytes for it.
 *   hbh_g2_set_create / _destroy: `capacity` slots on `eng`, allocated once (a set never grows, its
 *     tables never move).  Ownership as commitment sets: hbh_engine_destroy frees the device memory
 *     and detaches the set, after which every call naming it returns HBH_ERR_ARG and
 *     hbh_g2_set_destroy only frees the handle; a set used with another engine is HBH_ERR_ARG.
 *   hbh_g2_set_add: prepares n points (ABI G2, the ABI's subgroup contract; a coordinate >= p is
 *     HBH_ERR_ARG) into the lowest free slots and returns them in slots[0..n); one table launch per
 *     call, ordered after every earlier call on any stream and before every later one.  Fewer than n
 *     free slots: HBH_ERR_ARG, nothing is added.
 *   hbh_g2_set_release: frees slots for reuse; a slot that is not live (or named twice) is
 *     HBH_ERR_ARG and nothing is freed.
 *   hbh_g2_set_size: live slots and capacity.
 *   hbh_verify_pairing_eq_set: hbh_verify_pairing_eq where a side with a non-NULL set takes its Q from
 *     the set: q*_table must be NULL and nq* 0, and q*_idx (required: no identity map) holds slots,
 *     every one live, else HBH_ERR_ARG.  A side with a NULL set is exactly hbh_verify_pairing_eq's
 *     (per-check Q or a per-call shared table); both sides may name the same set.  Same verdicts.
 *   hbh_verify_sig_shares_set: hbh_verify_sig_shares with H = docs[doc_slot[i]].
 *   hbh_verify_dec_shares_set: hbh_verify_dec_shares with H_uv = cts[huv_slot[i]], W = cts[w_slot[i]].
 *   hbh_verify_pairing_eq_set_dev: hbh_verify_pairing_eq_dev likewise (same ordering between streams).
 *     Slot arrays live in device memory and are not inspected: a slot >= capacity yields verdict 0, a
 *     released slot is the caller's error (it reads whatever point holds the slot).
 * With both sides resident the wave kernels (HBH_IMPL_WAVE2 / WAVE / WAVEP) read both tables at any n;
 * with one they walk it from the stored affine point, as they walk a shared side of a small call.
 * Sets belong to one engine: the pool has no set entry points. */
typedef struct hbh_g2_set hbh_g2_set;
int hbh_g2_set_create(hbh_engine* eng, size_t capacity, hbh_g2_set** out);
int hbh_g2_set_destroy(hbh_g2_set* set);
int hbh_g2_set_add(hbh_g2_set* set, size_t n, const uint8_t* pts, uint32_t* slots);
int hbh_g2_set_release(hbh_g2_set* set, size_t n, const uint32_t* slots);
int hbh_g2_set_size(const hbh_g2_set* set, size_t* live, size_t* capacity);
int hbh_verify_pairing_eq_set(hbh_engine* eng, size_t n,
                              const uint8_t* p1, hbh_g2_set* set1, const uint8_t* q1_table, size_t nq1, const uint32_t* q1_idx,
                              const uint8_t* p2, hbh_g2_set* set2, const uint8_t* q2_table, size_t nq2, const uint32_t* q2_idx,
                              uint8_t* verdicts);
int hbh_verify_sig_shares_set(hbh_engine* eng, size_t n, const uint8_t* pks, const uint8_t* sigs,
                              hbh_g2_set* docs, const uint32_t* doc_slot, uint8_t* verdicts);
int hbh_verify_dec_shares_set(hbh_engine* eng, size_t n, const uint8_t* shares, const uint8_t* pks,
                              hbh_g2_set* cts, const uint32_t* huv_slot, const uint32_t* w_slot, uint8_t* verdicts);
int hbh_verify_pairing_eq_set_dev(hbh_engine* eng, void* stream, size_t n,
                                  const void* d_p1, hbh_g2_set* set1, const void* d_q1_table, size_t nq1, const uint32_t* d_q1_idx,
                                  const void* d_p2, hbh_g2_set* set2, const void* d_q2_table, size_t nq2, const uint32_t* d_q2_idx,
                                  uint8_t* d_verdicts);

/* ---------------------------------------------------------------- grouped share checks (opt-in)
 * hbh_verify_sig_shares / hbh_verify_dec_shares with ONE pairing check per group of items that share a
 * table entry (the shares of one document share H; the shares of one ciphertext share H_uv and W):
 *   sig shares of document d:   e(sum r_i pk_i, H_d)    == e(g1, sum r_i sig_i)
 *   dec shares of ciphertext c: e(sum r_i D_i,  H_uv_c) == e(sum r_i pk_i, W_c)
 * with one scalar r_i in [1, 2^128) per item.  A group whose check holds reports every member valid; the
 * items of a group whose check fails, and the items alone in their group, are re-checked share by share
 * by the call above, so a verdict of 0 is always exact.  A verdict of 1 from a passed group is the
 * reference's verdict except with probability at most 1 / (2^128 - 1) per group holding an invalid
 * share -- PROVIDED the points are in the prime-order subgroups (the ABI's contract) and the scalars
 * are uniform in [1, 2^128), independent of the inputs, and unknown to whoever chose the shares.
 *   scalars == NULL: the engine draws n x 128 bits from the OS (getrandom) and replaces a zero draw.
 *     This is the form the bound above is stated for.
 *   scalars != NULL: n x 16 bytes, little-endian, USED AS GIVEN (an all-zero scalar is HBH_ERR_ARG).
 *     The bound then holds only if the caller's scalars meet the conditions above: scalars a share
 *     sender can predict let two invalid shares cancel inside a group.  For tests and for callers
 *     with their own randomness.
 * Index and argument errors, and n = 0, are as in the per-share calls.  stats (may be NULL): groups =
 * groups of at least two items (each one pairing check), groups_passed = those whose check held,
 * singles = items alone in their group, fallback_items = items re-checked share by share (the items of
 * the failed groups plus the singles).  The group sums are accounted under HBH_STAGE_CURVE, the group
 * checks and the fallback under HBH_STAGE_PAIRING / HBH_STAGE_PREPARE as any pairing check.  Stateless:
 * no _dev, pool or G2-set form.  What the grouped call costs against the per-share call on an MI355X:
 * profiles/r16/README.md. */
typedef struct {
  uint32_t groups, groups_passed, singles, fallback_items;
} hbh_grouped_stats;
int hbh_verify_sig_shares_grouped(hbh_engine* eng, size_t n, const uint8_t* pks, const uint8_t* sigs,
                                  const uint8_t* hashes, size_t ndocs, const uint32_t* doc_idx,
                                  const uint8_t* scalars, uint8_t* verdicts, hbh_grouped_stats* stats);
int hbh_verify_dec_shares_grouped(hbh_engine* eng, size_t n, const uint8_t* shares, const uint8_t* pks,
                                  const uint8_t* huv, const uint8_t* w, size_t ncts, const uint32_t* ct_idx,
                                  const uint8_t* scalars, uint8_t* verdicts, hbh_grouped_stats* stats);
/* Kernels of the two group sums of a grouped call and of hbh_dbg_group_sums (same bytes from either: the
 * scalars are the same integers, only the order of the additions differs, and the sums leave the device
 * as canonical affine points; verdicts, hbh_grouped_stats and the bound above do not depend on the form):
 *   HBH_GSUM_CHAIN (k_rlc.hip): one double-and-add chain per (item, digit of the scalar); every item
 *     pays its own doublings.
 *   HBH_GSUM_BUCKET (k_rlc_bucket.hip): two-bit windows, three buckets per window in LDS, one wave per
 *     tile of a group; the doublings are paid once per tile.
 *   HBH_GSUM_AUTO (the default): BUCKET for a sum of a call of at least HBH_AUTO_GSUM_G1_BUCKET_MIN (a
 *     G1 sum) / HBH_AUTO_GSUM_G2_BUCKET_MIN (the G2 sum) items (0: never), CHAIN below; the two sums of
 *     one call may take different forms.  Thresholds: the smallest swept size from which BUCKET's median
 *     HBH_STAGE_CURVE time is below CHAIN's by more than both cells' min-max spread, at that and every
 *     larger swept size (profiles/r17/README.md, tools/grouped_bench.py --sum-impl both).
 * A forced form runs for every call.  Any other value returns HBH_ERR_ARG and changes nothing. */
#define HBH_GSUM_AUTO 0
#define HBH_GSUM_CHAIN 1
#define HBH_GSUM_BUCKET 2
#define HBH_AUTO_GSUM_G1_BUCKET_MIN 0
#define HBH_AUTO_GSUM_G2_BUCKET_MIN 0
int hbh_engine_set_group_sum_impl(hbh_engine* eng, int impl);
/* How a grouped call READS and DRAWS its scalars (still 16 bytes per item; |x| = 0xd201000000010000 is the
 * curve parameter, r = |x|^4 - |x|^2 + 1 the group order):
 *   HBH_GSCALAR_INT128 (the default): one little-endian integer r_i < 2^128, as described above.
 *   HBH_GSCALAR_DIGITS: short little-endian digits in the endomorphism basis (k_rlc_digits.hip):
 *     hbh_verify_sig_shares_grouped reads X4: four u32 digits a0..a3,
 *         r_i = a0 + a1 |x| + a2 |x|^2 + a3 |x|^3          <= (2^32 - 1)(1 + |x| + |x|^2 + |x|^3) < 2^224 < r;
 *     hbh_verify_dec_shares_grouped reads X2: two u64 digits b0, b1,
 *         r_i = b0 + b1 |x|^2                              <= (2^64 - 1)(1 + |x|^2) < 2^192 < r.
 *     The integer r_i is below r, so it is its own residue, and the digits are below |x| (X4) / |x|^2 (X2),
 *     so the base-|x| (base-|x|^2) representation is unique: distinct tuples are distinct residues mod r.
 *     The all-zero tuple is excluded exactly as the zero scalar is (redrawn when the engine draws, HBH_ERR_ARG
 *     when given), so the engine's draw is uniform over 2^128 - 1 distinct non-zero residues and the bound
 *     above -- at most 1 / (2^128 - 1) per group holding an invalid share -- holds under the same conditions,
 *     read for the form's digits: uniform non-zero tuples, independent of the inputs, unknown to whoever
 *     chose the shares.  (The bound needs only that the r_i of a group's other items fix at most one
 *     residue for which the group's equation holds.)  Both sums of a call use the SAME residue r_i for item i:
 *     a signature call applies the X4 residue on its G1 side (as (a0 + a1 |x|) P + (a2 + a3 |x|) [x^2] P) and
 *     on its G2 side (as a0 Q - a1 psi(Q) + a2 psi^2(Q) - a3 psi^3(Q), psi = [x] on G2); a decryption call
 *     applies the X2 residue on both G1 sides.  Every chain is then 32 (G2), 96 (G1, X4) or 64 (G1, X2) steps
 *     of one joint double-and-add instead of 64 + 64 (G2) or 128 (G1).
 * Given scalars are used as given in the form's layout.  Verdicts of 0, the fallback, hbh_grouped_stats and the
 * stage accounting do not depend on the form.  hbh_engine_set_group_sum_impl governs INT128 only: the digit
 * forms always run their own kernels.  Any other value returns HBH_ERR_ARG and changes nothing.  Measured
 * against INT128 and the per-share call: profiles/r22/README.md (tools/grouped_bench.py --scalar-form both). */
#define HBH_GSCALAR_INT128 0
#define HBH_GSCALAR_DIGITS 1
int hbh_engine_set_group_scalar_form(hbh_engine* eng, int form);

/* ---------------------------------------------------------------- combine (interpolate at 0)
 * threshold_crypto interpolate(t, samples) for `ncomb` independent combines of exactly t+1
 * samples each (the first t+1 of the reference's iterator, in its order): out[c] =
 * sum_k lambda_k(0) * P[c][k] with x_k = idx[c][k] + 1.  status[c] = HBH_OK or
 * HBH_ERR_DUPLICATE_ENTRY (two equal indices), as threshold_crypto reports it.  t = 0 returns the
 * single sample.  A caller holding fewer than t+1 shares reports HBH_ERR_NOT_ENOUGH_SHARES itself
 * (the reference checks that before interpolating).
 *   PublicKeySet::combine_signatures (src/threshold_sign.rs:249-259)   -> hbh_interpolate_g2
 *   PublicKeySet::decrypt's G1 interpolation (src/threshold_decrypt.rs:242-250; the XOR with
 *   hash(g) stays on the host)                                         -> hbh_interpolate_g1 */
int hbh_interpolate_g2(hbh_engine* eng, size_t ncomb, int t, const uint32_t* idx, const uint8_t* pts, uint8_t* out,
                       int* status);
int hbh_interpolate_g1(hbh_engine* eng, size_t ncomb, int t, const uint32_t* idx, const uint8_t* pts, uint8_t* out,
                       int* status);

/* ThresholdSign::combine_and_verify_sig (src/threshold_sign.rs:249-270) for `ncomb` documents in
 * one device pass: out[c] = combine_signatures(first t+1 shares) as hbh_interpolate_g2, then
 * verdict[c] = PublicKey::verify_g2(out[c], hashes[c]) = (e(master_pk, H_c) == e(g1, out[c]))
 * (:260-266) without a host round trip in between.  status[c] as hbh_interpolate_g2; verdict[c]
 * = 0 is the reference's Error::VerificationFailed; verdicts of a combine whose status is not
 * HBH_OK are meaningless (the reference returns the combine error first).  A master_pk coordinate
 * >= p is HBH_ERR_ARG.  Calls of at most 540 + 24 t one-pair Miller waves (ncomb x (t + 2); at most
 * 384 combines) evaluate the same verdict as prod_k e(lambda_k g1, share_k) * e(-master_pk, H_c) == 1 on a
 * second stream while the first interpolates ("split master check"; the environment
 * variable HBH_SPLIT_CHECK=0 at engine creation selects interpolate-then-verify for every size;
 * HBH_SPLIT_MAX=<n> replaces the wave-count rule by "at most n combines per call"). */
int hbh_combine_verify_g2(hbh_engine* eng, size_t ncomb, int t, const uint32_t* idx, const uint8_t* shares,
                          const uint8_t* master_pk, const uint8_t* hashes, uint8_t* out, int* status,
                          uint8_t* verdicts);

/* ---------------------------------------------------------------- scalar multiplication
 * out[i] = k_i * P_i, k_i a 32-byte little-endian integer (any value < 2^256).  Public-data helper
 * for commitments (Poly::commitment = g1 * c_i, src/sync_key_gen.rs:508), public-key-share
 * derivation (src/network_info.rs:59-62) and synthetic-input generation.  Secret keys stay on the
 * host in the reference flow (sign_g2 / decrypt_share). */
int hbh_g1_mul(hbh_engine* eng, size_t n, const uint8_t* pts, const uint8_t* scalars, uint8_t* out);
int hbh_g2_mul(hbh_engine* eng, size_t n, const uint8_t* pts, const uint8_t* scalars, uint8_t* out);
/* out[i] = g1 * k_i with a fixed-base comb table of the generator (32 mixed additions per scalar,
 * table built on the engine's first use): BivarPoly::commitment / Poly::commitment
 * (src/sync_key_gen.rs:346-357, 508) and key derivation.  Same points as hbh_g1_mul(g1, k). */
int hbh_g1_mul_gen(hbh_engine* eng, size_t n, const uint8_t* scalars, uint8_t* out);

/* ---------------------------------------------------------------- SyncKeyGen commitments
 * commits: nparts BivarCommitments of degree t, each (t+1)(t+2)/2 G1 points in threshold_crypto's
 * coeff_pos order (j(j+1)/2 + i for i <= j).
 * hbh_bivar_row: BivarCommitment::row(x) (src/sync_key_gen.rs:496) for nrow (part_idx, x) pairs;
 *   out = nrow * (t+1) G1 points.  Compare with Poly::commitment (hbh_g1_mul of g1) for :508.
 * hbh_bivar_ack_check: verdict[a] = (BivarCommitment::evaluate(x_a, y_a) == g1 * val_a)
 *   (src/sync_key_gen.rs:542); vals are 32-byte LE Fr values (the decrypted Ack values).
 *   x, y are the 1-based node indices the reference passes (our_idx + 1, sender_idx + 1). */
int hbh_bivar_row(hbh_engine* eng, size_t nrow, int t, size_t nparts, const uint8_t* commits, const uint32_t* part_idx,
                  const uint32_t* xs, uint8_t* out);
int hbh_bivar_ack_check(hbh_engine* eng, size_t nack, int t, size_t nparts, const uint8_t* commits,
                        const uint32_t* part_idx, const uint32_t* xs, const uint32_t* ys, const uint8_t* vals,
                        uint8_t* verdicts);

/* Device-resident commitments.  A SyncKeyGen instance keeps every Part's BivarCommitment for its
 * lifetime (ProposalState::commit, src/sync_key_gen.rs:254-262) and checks rows (:496) and Acks
 * (:542) against it on every drain.  A commitment set holds such commitments (one degree t per set)
 * in HBM, uploaded once, plus the Jacobian rows row(x) computed so far; calls name parts by their
 * index in the set and upload only indices and values.
 *   hbh_commit_set_create / _destroy: an empty set of degree t on `eng` (destroy waits for the
 *     engine's work).  The engine owns its sets' device memory: hbh_engine_destroy frees it and
 *     detaches the sets, after which every call on such a set returns HBH_ERR_ARG and
 *     hbh_commit_set_destroy only frees the handle (either destruction order is safe).
 *   hbh_commit_set_add: append nparts commitments ((t+1)(t+2)/2 ABI G1 points each, coeff_pos
 *     order); *first (may be NULL) = the set index of the first one.
 *   hbh_commit_set_size: commitments and cached rows held.
 *   hbh_bivar_row_set / hbh_bivar_ack_check_set: hbh_bivar_row / hbh_bivar_ack_check with part_idx
 *     into the set (same outputs). */
typedef struct hbh_commit_set hbh_commit_set;
int hbh_commit_set_create(hbh_engine* eng, int t, hbh_commit_set** out);
int hbh_commit_set_destroy(hbh_commit_set* cs);
int hbh_commit_set_add(hbh_commit_set* cs, size_t nparts, const uint8_t* commits, size_t* first);
int hbh_commit_set_size(const hbh_commit_set* cs, size_t* nparts, size_t* nrows);
int hbh_bivar_row_set(hbh_commit_set* cs, size_t nrow, const uint32_t* part_idx, const uint32_t* xs, uint8_t* out);
int hbh_bivar_ack_check_set(hbh_commit_set* cs, size_t nack, const uint32_t* part_idx, const uint32_t* xs,
                            const uint32_t* ys, const uint8_t* vals, uint8_t* verdicts);

/* Commitment::evaluate(x) = sum_j C_j x^j for n (commitment, x) requests; commits holds ncommits
 * Commitments of t+1 G1 points each, out = n G1 points.  PublicKeySet::public_key_share(i) is
 * evaluate(i + 1): NetworkInfo::new precomputes it for every node (src/network_info.rs:59-62), and
 * a SyncKeyGen node does the same for the generated key (src/sync_key_gen.rs:449 via
 * PublicKeySet::from(commit)).  xs are the 1-based integers the reference passes. */
int hbh_commitment_eval(hbh_engine* eng, size_t n, int t, size_t ncommits, const uint8_t* commits,
                        const uint32_t* commit_idx, const uint32_t* xs, uint8_t* out);

/* ---------------------------------------------------------------- wire formats
 * pairing 0.14 G1Compressed::into_affine for n 48-byte compressed G1 points (zcash encoding:
 * big-endian x, 0x80 = compressed, 0x40 = infinity, 0x20 = larger y).  out[i] = the ABI point,
 * ok[i] = 1 iff the encoding is well formed, x < p, x^3 + 4 is a square and the point lies in the
 * prime-order subgroup -- the checks threshold_crypto's deserialisation runs on every PublicKey,
 * PublicKeyShare, DecryptionShare and Ciphertext U before it reaches the verify calls (serde
 * decoding of hbbft's messages; decode sites listed in SURVEY §8f f2).
 * A point with ok[i] == 0 is written as all-zero bytes; the caller rejects the message as the
 * reference's deserialisation error does. */
int hbh_g1_decompress(hbh_engine* eng, size_t n, const uint8_t* in, uint8_t* out, uint8_t* ok);
/* G2Compressed::into_affine for n 96-byte compressed G2 points (x.c1 || x.c0 big-endian, flags in
 * the first byte; y^2 = x^3 + 4(1 + u); larger y by pairing 0.14's Fq2 order: c1, then c0);
 * out = ABI G2 points.  Same ok / all-zero convention as hbh_g1_decompress. */
int hbh_g2_decompress(hbh_engine* eng, size_t n, const uint8_t* in, uint8_t* out, uint8_t* ok);
/* Decoding kernels of hbh_g1_decompress, hbh_g2_decompress and their _dev forms (same bytes and ok
 * verdicts from either):
 *   HBH_DEC_LANE (k_wire.hip): 64 points per workgroup, one lane per point takes the square root
 *     while one lane per point runs the whole subgroup chain -- throughput.
 *   HBH_DEC_SPLIT (k_wire_split.hip): 16 points per workgroup, one lane per point takes the square
 *     root while FOUR lanes per point split the group operations of the subgroup chain -- latency:
 *     a small batch takes the time of the root chain instead of the (longer) subgroup chain.
 *   HBH_DEC_AUTO (the default): SPLIT for n <= HBH_AUTO_DEC_G1_SPLIT_MAX / HBH_AUTO_DEC_G2_SPLIT_MAX
 *     points per call (0: never), LANE above.  Thresholds: the largest swept size at which SPLIT's
 *     median kernel time is below LANE's by more than both cells' min-max spread
 *     (profiles/r07/decode_latency_sweep.json: wins at 4,096, loses at 16,384; refined in
 *     profiles/r07/decode_latency_refine.json: 8,192 points are 512 workgroups = one wave on every
 *     SIMD, and 8,208 start a second round; tools/decode_bench.py --impl both).
 * A forced form runs for every n.  Any other value returns HBH_ERR_ARG and changes nothing. */
#define HBH_DEC_AUTO 0
#define HBH_DEC_LANE 1
#define HBH_DEC_SPLIT 2
#define HBH_AUTO_DEC_G1_SPLIT_MAX 8192
#define HBH_AUTO_DEC_G2_SPLIT_MAX 8192
int hbh_engine_set_decode_impl(hbh_engine* eng, int impl);

/* ---------------------------------------------------------------- hashing to G2 on the device
 * threshold_crypto hash_g2 / hash_g1_g2 for large batches of PUBLIC inputs (documents, signed messages,
 * the (U, V) of ciphertexts; every secret-key operation keeps the host stage, and so do the secret parts
 * of encryption: of hbh_engine_encrypt only the SHA3 seeds of the public (U, V) reach the device).  SHA3 and
 * the message assembly run on the host (hbh_hash_g2's code and worker threads); the curve half --
 * sampling x from the seeded ChaCha20 stream, the square root, the sign choice and the cofactor
 * multiplication (csrc/hash_sample.hpp, k_hash.hip) -- runs on the GPU.  Output bytes are hbh_hash_g2's.
 * A hash is a serial chain of milliseconds however many lanes walk it (one, or four: hbh_engine_set_hash_form),
 * so small calls belong on the host stage (hbh_engine_set_hash_impl).
 *   hbh_engine_hash_g2 / hbh_engine_hash_g1_g2: arguments and output as hbh_hash_g2 / hbh_hash_g1_g2.
 *   hbh_hash_g2_dev: d_seeds = n 32-byte seeds (sha3_256 of each message) in HBM, d_out = n ABI G2 points
 *     in HBM; asynchronous on `stream` and ordered like the other _dev calls.  The sampler runs a fixed
 *     number of rounds (HBH_HASH_ROUNDS: one candidate x per unresolved message and round, each a square
 *     with probability 1/2).  A message that needed more candidates is UNRESOLVED: its output is the
 *     all-zero point, which hash_g2 never returns (h2 (x, y) = O is resampled); the caller hashes it with
 *     hbh_hash_g2.  The host-pointer calls do that themselves, so their outputs are always complete.
 *   hbh_verify_signatures: PublicKey::verify(sig, msg) in one call (DHB signed votes and key-gen messages,
 *     src/dynamic_honey_badger/votes.rs:157, dynamic_honey_badger.rs:520):
 *     verdict[i] = e(pk[i], hash_g2(msg_i)) == e(g1, sig[i]), messages as hbh_hash_g2's.  On the device form
 *     the hashes never leave HBM: they are the Q1 table of hbh_verify_pairing_eq under the identity map.
 *   hbh_engine_set_hash_impl: HBH_HASH_HOST (the host stage, hbh_hash_g2's workers), HBH_HASH_DEVICE, or
 *     HBH_HASH_AUTO (the default): DEVICE for calls of at least HBH_AUTO_HASH_DEVICE_MIN messages (0:
 *     never), HOST below.  Governs every host-pointer call of this section; same bytes and verdicts from
 *     either.
 *     Threshold: the smallest swept size from which DEVICE's median host-to-host time is below HOST's by
 *     more than both cells' min-max spread, at that and every larger swept size, DEVICE taking the better of
 *     its two forms (384 with the QUAD form: profiles/r24/README.md; 4,096 with the LANE form alone:
 *     profiles/r14/README.md; tools/hash_bench.py).  Any other value returns HBH_ERR_ARG and changes nothing.
 *   hbh_engine_set_hash_form: how many lanes walk one hash when a call runs on the device.  HBH_HFORM_LANE
 *     is the throughput form above (k_hash.hip).  HBH_HFORM_QUAD is its latency form (k_hash_quad.hip): four
 *     lanes per message -- the sampler tries a message's next four candidates side by side, one launch for
 *     15 messages in 16, and the cofactor multiplication runs on lane quads (the lane-pair Fp2 and group law
 *     of the split decoders).  HBH_HFORM_AUTO (the default): QUAD for device runs of at most
 *     HBH_AUTO_HASH_QUAD_MAX messages (0: never; HBH_HASH_QUAD_ALL: every size), LANE above.  Any other
 *     value returns HBH_ERR_ARG and changes nothing.  A setter of its own: hbh_engine_set_hash_impl says
 *     WHERE a call runs, this one HOW the device runs it, and it has no effect on a call that takes the host
 *     stage.  It governs every device run of the hash: hbh_engine_hash_g2 / _hash_g1_g2 / _hash_g1_g2_bp,
 *     hbh_hash_g2_dev, hbh_verify_signatures, hbh_verify_ciphertexts_uv and hbh_engine_encrypt; each still
 *     records one HBH_STAGE_HASH entry per call.
 *     Bytes: QUAD writes LANE's and the host stage's bytes, in the full and in the Q form.
 *     Round cap: HBH_HASH_ROUNDS (and hbh_dbg_set_hash_rounds) caps the CANDIDATES tried per message under
 *     either form -- QUAD runs ceil(cap / 4) sampler launches and masks the lanes whose candidate would be
 *     past the cap -- so both forms leave exactly the same messages unresolved, and hbh_hash_g2_dev writes
 *     the same bytes, zero points included, under either.
 *     Thresholds: a form wins at a size when the other's median host-to-host time exceeds its own by more
 *     than the two cells' min-max spreads together.  HBH_AUTO_HASH_QUAD_MAX is the largest swept size up to
 *     which QUAD wins at every swept size from the smallest; HBH_AUTO_HASH_DEVICE_MIN is the smallest swept
 *     size from which the better device form beats HOST at that and every larger one.  The sweep of
 *     profiles/r24/README.md (tools/hash_bench.py --form both; sizes 64 .. 65,536) set them: QUAD wins at every
 *     size (hash stage 4.5 against 14.1 ms at 64 messages, 7.2 against 23.3 ms at 10,100, 18.8 against 26.4 ms
 *     at 65,536), so HBH_AUTO_HASH_QUAD_MAX is HBH_HASH_QUAD_ALL, and HBH_AUTO_HASH_DEVICE_MIN is 384 (refined between the swept 256 and 1,024).
 * The Q form (k_hash_clear_bp): the device stops at the Budroni-Pintore image Q_bp of the sampled point,
 * hash_g1_g2(U, V) = [KCOF] Q_bp (hbh_hash_g1_g2_bp below), for the callers that fold [KCOF] into a pairing
 * side or into a scalar they multiply by anyway.  HOST, DEVICE and AUTO as above; messages left after
 * HBH_HASH_ROUNDS are hashed on the host stage and patched in.
 *   hbh_engine_hash_g1_g2_bp: arguments and output bytes as hbh_hash_g1_g2_bp.
 *   hbh_verify_ciphertexts_uv: Ciphertext::verify from the ciphertext itself (SecretKey::decrypt's check,
 *     sync_key_gen.rs:503-506, 535-538): verdict[i] = e(G1K, W_i) == e(U_i, Q_bp(U_i, V_i)), the verdicts of
 *     hbh_verify_ciphertexts bit for bit (U = O and W = O included).  u = n ABI G1 points, V_i =
 *     data[offsets[i] .. offsets[i+1]), w = n ABI G2 points.  On the device form the hashes are written
 *     into the Q2 table of the pairing check and never leave HBM.
 *   hbh_engine_encrypt: hbh_encrypt's arguments (without threads) and bytes.  hbh_encrypt_uv on the host
 *     workers, the seeds sha3_256(hash_g1_g2's message of (U_i, V_i)), Q_bp on the device, hbh_encrypt_w on
 *     the host workers.  ONLY THOSE SEEDS CROSS TO THE DEVICE: they are hashes of the public wire message
 *     (U, V).  The nonces, pk r, the plaintexts and the scalars KCOF r stay in host memory. */
#define HBH_HASH_AUTO 0
#define HBH_HASH_HOST 1
#define HBH_HASH_DEVICE 2
#define HBH_HASH_ROUNDS 32
#define HBH_AUTO_HASH_DEVICE_MIN 384 /* profiles/r24 (the QUAD form; 4,096 with the LANE form alone, profiles/r14) */
#define HBH_HFORM_AUTO 0
#define HBH_HFORM_LANE 1
#define HBH_HFORM_QUAD 2
#define HBH_HASH_QUAD_ALL ((size_t)-1) /* a value of HBH_AUTO_HASH_QUAD_MAX: QUAD at every size */
#define HBH_AUTO_HASH_QUAD_MAX (HBH_HASH_QUAD_ALL) /* QUAD wins at every swept size, 64 .. 65,536 (profiles/r24) */
int hbh_engine_set_hash_form(hbh_engine* eng, int form);
int hbh_engine_hash_g2(hbh_engine* eng, size_t n, const uint8_t* data, const size_t* offsets, uint8_t* out);
int hbh_engine_hash_g1_g2(hbh_engine* eng, size_t n, const uint8_t* u, const uint8_t* data, const size_t* offsets,
                          uint8_t* out);
int hbh_hash_g2_dev(hbh_engine* eng, void* stream, size_t n, const uint8_t* d_seeds, void* d_out);
int hbh_verify_signatures(hbh_engine* eng, size_t n, const uint8_t* pks, const uint8_t* sigs, const uint8_t* data,
                          const size_t* offsets, uint8_t* verdicts);
int hbh_engine_set_hash_impl(hbh_engine* eng, int impl);
int hbh_engine_hash_g1_g2_bp(hbh_engine* eng, size_t n, const uint8_t* u, const uint8_t* data, const size_t* offsets,
                             uint8_t* out);
int hbh_verify_ciphertexts_uv(hbh_engine* eng, size_t n, const uint8_t* u, const uint8_t* data, const size_t* offsets,
                              const uint8_t* w, uint8_t* verdicts);
int hbh_engine_encrypt(hbh_engine* eng, size_t n, const uint8_t* pks, int pk_per_item, const uint8_t* data,
                       const size_t* offsets, const uint8_t* nonces, uint8_t* u_out, uint8_t* v_out, uint8_t* w_out);

/* ---------------------------------------------------------------- batched independent checks (opt-in)
 * hbh_verify_signatures / hbh_verify_ciphertexts_uv with ONE final exponentiation per group of
 * HBH_BATCH_GROUP items.  These items share no G2 point, so the grouped share checks above do not apply;
 * the random combination is taken over whole pairings instead:
 *   signatures:   prod_i e(r_i pk_i, H_i) * e(-g1,  sum_i r_i sig_i) == 1
 *   ciphertexts:  prod_i e(r_i U_i,  Q_i) * e(-G1K, sum_i r_i W_i)   == 1      (Q_i = Q_bp(U_i, V_i))
 * Group g holds the items [256 g, min(n, 256 g + 256)) in call order; a last group of one item is a
 * single and takes the per-item check.  Per group: r_i P_i per item (k_rlc_digits.hip k_scale_digits_g1),
 * the G2 sum (the digit kernels of the grouped share checks), the Miller values of the items multiplied up
 * a tree inside the lane kernel (pair_side.hpp lane_miller_prod: two items per slot, no final
 * exponentiation; 1, 2 or 4 tiles per group on lane pairs, quads, octos), the closing pair as one
 * Miller-only wave check, and one product + final exponentiation (the wave kernel's product mode).
 * A group whose check holds reports every member valid; the items of a group whose check fails, and the
 * single, are re-checked item by item by the unbatched pairing path, so a verdict of 0 is always exact.
 * A verdict of 1 from a passed group is the reference's verdict except with probability at most
 * 1 / (2^128 - 1) per group holding an invalid item -- PROVIDED the points are in the prime-order
 * subgroups (the ABI's contract) and the scalars are uniform, independent of the inputs, and unknown to
 * whoever chose the items.
 *   Scalars: 16 bytes per item, ALWAYS read as X4 digits (four LE u32 a0..a3, r_i = a0 + a1 |x| + a2 |x|^2 +
 *     a3 |x|^3: the layout hbh_verify_sig_shares_grouped reads under HBH_GSCALAR_DIGITS, with the same
 *     uniqueness argument), the same residue on the G1 side and in the G2 sum.
 *     hbh_engine_set_group_scalar_form and hbh_engine_set_group_sum_impl do not govern these calls.
 *     scalars == NULL: the engine draws them from the OS (getrandom) and replaces an all-zero draw: the form
 *     the bound is stated for.  scalars != NULL: USED AS GIVEN (an all-zero tuple is HBH_ERR_ARG); the bound
 *     then holds only if the caller's scalars meet the conditions above.
 *   Hashing: exactly as in the unbatched calls (hbh_engine_set_hash_impl / _hash_form, the Q form for
 *     ciphertexts, leftovers of the sampler rounds patched in from the host stage).  The hashes computed
 *     for the call serve the group checks AND the fallback: no item is hashed twice, on the device form
 *     they stay in HBM, and a call records one HBH_STAGE_HASH entry, fallback or not.
 *   Stages: the scaling and the sums under HBH_STAGE_CURVE; the Miller product, the closing pair, the
 *     final exponentiation and the fallback under HBH_STAGE_PAIRING.
 *   Width: hbh_engine_set_pairing_impl forced to HBH_IMPL_PAIR, _QUAD or _OCT is honoured by the Miller
 *     product; any other forced value and HBH_IMPL_AUTO choose by lane-kernel slots, ceil(items / 2):
 *     OCT up to HBH_AUTO_OCT_MAX slots, QUAD up to HBH_AUTO_QUAD_MAX, PAIR above.  Those thresholds were
 *     measured for the full check; swept for this kernel at 1,024, 10,100 and 65,536 items (all valid,
 *     pairing stage: OCT 5.3 / 5.5 ms against QUAD 6.3 and PAIR 9.2-9.3 at the first two, PAIR 10.7 and QUAD
 *     10.8-11.1 against OCT 15.9 at the third; tools/batched_bench.py, profiles/r25/README.md) the ladder
 *     picks the fastest width at each, so the kernel has no HBH_AUTO_BATCH_* constants of its own; the
 *     crossovers between were not swept.  A forced width also governs the fallback, as it governs any
 *     pairing call; under AUTO the fallback runs as a pairing call of its size.
 *   Infinities as in the unbatched calls, through a passed group as through the fallback: pk = O with
 *     sig = O is valid, pk = O with sig != O is invalid (the group's sum then fails its check), the same
 *     for U = O / W = O.
 * Argument errors and n = 0 are as in the unbatched calls.  stats (may be NULL) as in the grouped share
 * checks: groups = groups of at least two items, groups_passed, singles (0 or 1), fallback_items = the
 * items of the failed groups plus the single.  Stateless: no _dev, pool or G2-set form, and no AUTO
 * switch between the batched and the per-item call: the caller opts in.
 * Op model per item (hbbft_amd/workcount.py batched_model, Fp products): per-item check about 19.4 k;
 * batched about 10.8 k with no failed group (ratio 0.56; the pairing stage alone 0.32); a failed group
 * pays both.  MEASURED on an MI355X (profiles/r25/README.md; a form wins a cell when the other's median
 * exceeds its own by more than both cells' min-max spreads together) the batched call is NOT faster
 * host-to-host at any swept size: it loses at 1,024 items (8.4 -> 17.3 ms) and at 10,100 items (signatures
 * 18.2 -> 21.3 ms, ciphertexts 17.6 -> 20.8 ms all valid; more with bad groups) and ties at 65,536 (57.5 ->
 * 59.9, 55.4 -> 55.0 ms).  HBH_STAGE_PAIRING falls as modelled in direction (8.1 -> 5.5 ms at 10,100, 21.6 ->
 * 10.7 ms at 65,536), but HBH_STAGE_CURVE, which the unbatched call does not have, costs 5.5 ms flat up to
 * 10,100 items (G2 sums 3.1-3.2 ms, G1 scaling 2.3 ms: one chain per lane on a device they do not fill) and
 * 10.2-10.6 ms at 65,536; and at 1,024 items the lane kernels' Miller product alone (5.3 ms) is slower than
 * the wave kernels' whole unbatched check (1.9 ms).  Use it only where a measurement of the caller's own
 * sizes says otherwise.
 *   hbh_dbg_pairing_product: out[g] = (prod_{i in group g} e(P_i, Q_i))^3 in hbh_dbg_pairing's 576-byte
 *     format, one value per group of HBH_BATCH_GROUP items (a last group of one item included), through
 *     the same Miller-product launch and product + final exponentiation, with no closing pair. */
#define HBH_BATCH_GROUP 256
int hbh_verify_signatures_batched(hbh_engine* eng, size_t n, const uint8_t* pks, const uint8_t* sigs,
                                  const uint8_t* data, const size_t* offsets, const uint8_t* scalars,
                                  uint8_t* verdicts, hbh_grouped_stats* stats);
int hbh_verify_ciphertexts_uv_batched(hbh_engine* eng, size_t n, const uint8_t* u, const uint8_t* data,
                                      const size_t* offsets, const uint8_t* w, const uint8_t* scalars,
                                      uint8_t* verdicts, hbh_grouped_stats* stats);
int hbh_dbg_pairing_product(hbh_engine* eng, size_t n, const uint8_t* p, const uint8_t* q, uint8_t* out);

/* ---------------------------------------------------------------- host stage (CPU, no engine)
 * What the north star keeps on the host, batched over `threads` std::thread workers (0 = all
 * hardware threads).  Variable-length inputs are concatenated in `data` with n+1 ascending byte
 * offsets (item i = data[offsets[i] .. offsets[i+1])).  Conventions: host_hash.cpp header and
 * SURVEY.md Appendix B.  Error text of these functions: hbh_host_last_error().
 *   hbh_hash_g2       threshold_crypto hash_g2(msg) -> G2 (ThresholdSign::set_document,
 *                     src/threshold_sign.rs:151; BA coin documents, binary_agreement.rs:442)
 *   hbh_hash_g1_g2    hash_g1_g2(U, V) -> G2 (Ciphertext::verify / verify_decryption_share's H_uv,
 *                     src/threshold_decrypt.rs:142,227)
 *   hbh_xor_with_hash V xor ChaCha20(sha3(compress(g))) low bytes; out has data's layout
 *                     (PublicKeySet::decrypt, src/threshold_decrypt.rs:249; SecretKey::decrypt,
 *                     src/sync_key_gen.rs:505,537)
 *   hbh_signature_parity  Signature::parity() per G2 point (the BA coin, binary_agreement.rs:402)
 *   hbh_g1_compress / hbh_g2_compress  pairing 0.14 compressed encodings (48 / 96 B)
 *   hbh_host_g1_mul / hbh_host_g2_mul  k * P with SECRET k on the host: SecretKeyShare::sign_g2
 *                     (threshold_sign.rs:167), decrypt_share_no_verify (threshold_decrypt.rs:161),
 *                     SecretKey::decrypt's U * sk (sync_key_gen.rs:505,537)
 *   hbh_host_g1_add   out[i] = a[i] + b[i] (public points; SyncKeyGen::generate's sum of
 *                     commitment rows, src/sync_key_gen.rs:449)
 *   hbh_encrypt       PublicKey::encrypt_with_rng with caller-drawn Fr nonces (32 B LE each):
 *                     U = g1 r, V = msg xor stream(pk r), W = hash_g1_g2(U, V) r
 *                     (sync_key_gen.rs:346-357,386-390; honey_badger/epoch_state.rs:224-237);
 *                     pks holds one key, or one per item when pk_per_item != 0
 *   hbh_fr_poly_eval  Poly::evaluate over Fr for many polynomials and points: out[p * npts + k] =
 *                     sum_j coeffs[p * ncoef + j] x_k^j mod r (32 B LE scalars in and out, coefficients
 *                     < r; xs are small node indices).  SyncKeyGen's rows of BivarPoly::row(x)
 *                     (sync_key_gen.rs:349-352) and the Ack values row.evaluate(i + 1) (:386-390)
 *   hbh_host_threads  the worker count `threads` = 0 means: the CPUs this process may use
 *                     (affinity mask, cgroup v2 cpu.max quota, HBH_HOST_THREADS / OMP_NUM_THREADS) */
const char* hbh_host_last_error(void);
int hbh_host_threads(int* out);
int hbh_hash_g2(size_t n, const uint8_t* data, const size_t* offsets, uint8_t* out, int threads);
int hbh_hash_g1_g2(size_t n, const uint8_t* u, const uint8_t* data, const size_t* offsets, uint8_t* out,
                   int threads);
int hbh_xor_with_hash(size_t n, const uint8_t* g, const uint8_t* data, const size_t* offsets, uint8_t* out,
                      int threads);
/* Ciphertext::verify without the last scalar multiplication of hash_g1_g2 (round 5): out[i] = Q_i,
 * a G2 point with hash_g1_g2(U_i, V_i) = [KCOF] Q_i for one fixed scalar KCOF (G2::rand's cofactor
 * multiplication h2 (x, y) = [KCOF] Q, Q = the Budroni-Pintore image of (x, y)).  By
 * bilinearity Ciphertext::verify(U, V, W) = e(g1, W) == e(U, [KCOF] Q) = e(G1K, W) == e(U, Q) with
 * G1K = [KCOF^-1 mod r] g1 (hbh_hash_bp_g1): hbh_verify_pairing_eq(P1 = G1K, Q1 = W, P2 = U, Q2 = Q)
 * gives the reference's verdict bit for bit (SecretKey::decrypt, sync_key_gen.rs:503-506, 535-538). */
int hbh_hash_g1_g2_bp(size_t n, const uint8_t* u, const uint8_t* data, const size_t* offsets, uint8_t* out,
                      int threads);
int hbh_hash_bp_g1(uint8_t* out);
int hbh_signature_parity(size_t n, const uint8_t* sigs, uint8_t* out);
int hbh_g1_compress(size_t n, const uint8_t* pts, uint8_t* out);
int hbh_g2_compress(size_t n, const uint8_t* pts, uint8_t* out);
int hbh_host_g1_mul(size_t n, const uint8_t* pts, const uint8_t* scalars, uint8_t* out, int threads);
int hbh_host_g2_mul(size_t n, const uint8_t* pts, const uint8_t* scalars, uint8_t* out, int threads);
int hbh_host_g1_add(size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out);
int hbh_encrypt(size_t n, const uint8_t* pks, int pk_per_item, const uint8_t* data, const size_t* offsets,
                const uint8_t* nonces, uint8_t* u_out, uint8_t* v_out, uint8_t* w_out, int threads);
/* hbh_encrypt split at its hash, so that a caller can take Q_bp of (U, V) from any source between the
 * halves (hbh_hash_g1_g2_bp, hbh_engine_hash_g1_g2_bp, a cache); hbh_engine_encrypt is that sequence.
 *   hbh_encrypt_uv  U = g1 r and V = msg xor stream(pk r): hbh_encrypt's arguments, key handling (one key
 *                   or one per item; a comb for a key with at least 16 items, GLV below) and U / V bytes
 *   hbh_encrypt_w   W_i = [KCOF r_i mod r] Q_i by one GLS multiplication, Q_i = Q_bp of (U_i, V_i) (n ABI
 *                   G2 points); an all-zero Q_i gives the all-zero W_i
 * hbh_encrypt_uv, then Q = hbh_hash_g1_g2_bp(U, V), then hbh_encrypt_w gives hbh_encrypt's bytes.  (U, V)
 * is the public wire message; the nonce r and pk r are secret and never leave these two calls. */
int hbh_encrypt_uv(size_t n, const uint8_t* pks, int pk_per_item, const uint8_t* data, const size_t* offsets,
                   const uint8_t* nonces, uint8_t* u_out, uint8_t* v_out, int threads);
int hbh_encrypt_w(size_t n, const uint8_t* qbp, const uint8_t* nonces, uint8_t* w_out, int threads);
int hbh_fr_poly_eval(size_t npoly, size_t ncoef, const uint8_t* coeffs, size_t npts, const uint64_t* xs, uint8_t* out,
                     int threads);

/* ---------------------------------------------------------------- implementation selection
 * Pairing implementations with identical verdicts (tests/test_gpu_pairing.py cross-checks them
 * against each other and the C oracle):
 *   HBH_IMPL_PAIR (k_pair.hip): TWO lanes per check, each lane holding one component of every Fp2
 *     value; the Miller loop walks per-check G2 points in registers and reads line tables only for
 *     G2 points shared through an index map; Miller loop and final exponentiation in one kernel.
 *     Throughput path.
 *   HBH_IMPL_WAVE (k_wave.hip): one 64-lane wave per check; the check's Fp2 products run on 32 lane
 *     pairs side by side.  Latency path (one check: the master check of combine_and_verify_sig).
 *   HBH_IMPL_QUAD (k_quad.hpp): FOUR lanes per check -- two lane pairs holding the check's state
 *     side by side and splitting each step's independent products (k_pair's work per check in
 *     ~0.55 of its per-lane time).  Mid-size path: 16,384 checks are one wave per SIMD.
 *   HBH_IMPL_OCT (k_oct.hpp): EIGHT lanes per check -- four lane pairs, four independent products per
 *     round.  Small-batch path: 8,192 checks are one wave per SIMD.
 *   HBH_IMPL_WAVE2 (k_wave64.hip, round 6): TWO 64-lane waves per check (64 lane pairs): the Miller
 *     loop multiplies a step's two lines together beside f^2 and takes their product in one stage,
 *     149 stages per two-pair check instead of WAVE's 210-211.  Latency path for calls of up to
 *     HBH_AUTO_WAVE2_MAX checks (AUTO; plain checks -- the split master check's modes stay on WAVE).
 *   HBH_IMPL_WAVEP (k_wavep.hip): WAVE's one wave per check and its stage programs, with two
 *     checks (waves) per workgroup; the final exponentiation's cyclotomic-squaring runs and its
 *     inversion -- 18 and 2 useful lanes of 64 on WAVE -- run for both checks together on one of the
 *     workgroup's waves (18 lanes per check, csrc/cyc_pack.hpp), the waves taking turns: 492 k VALU
 *     instructions per check against WAVE's 648 k.  Plain checks only, like WAVE2.  AUTO uses it for
 *     calls of HBH_AUTO_WAVEP_MIN..HBH_AUTO_WAVEP_MAX checks, ahead of the ladder below (MIN > MAX
 *     would mean never).  The range is the run of swept sizes at which its median kernel time is
 *     below WAVE's and OCT's by more than both cells' min-max spread (profiles/r08/wavep_sweep.json,
 *     wavep_refine.json, wavep_refine_auto.json, README.md there): 1,025..1,536 checks, where WAVE
 *     needs a second wave on some SIMDs and WAVEP still runs one round of workgroups -- 2.46-2.48 ms
 *     against 2.64-2.78 (-6 to -11 %).  Outside it the form does not win: 1,024 checks 2.48 against
 *     1.80, 2,048 checks 2.59 against 2.71 and 4,096 checks 4.98 against 5.08 (both inside the
 *     spread), OCT from 4,160 on.
 *   HBH_IMPL_AUTO (the default): WAVE2 up to HBH_AUTO_WAVE2_MAX checks per call, WAVE up to
 *     HBH_AUTO_WAVE_MAX checks per call, OCT up to
 *     HBH_AUTO_OCT_MAX, QUAD up to HBH_AUTO_QUAD_MAX (each one wave per SIMD at its maximum), PAIR
 *     above -- the measured crossovers (profiles/r04/c8_sweep_wave_quad_pair.txt,
 *     c23_oct_wave_sweep.txt, kernel ms per call on the sign workload): 4,096 checks WAVE 5.3 /
 *     OCT 5.5 / QUAD 7.0 / PAIR 10.6; 4,608: WAVE 6.6 / OCT 5.5; 8,192: 10.2 / 5.5 / 7.0 / 10.7;
 *     16,384: WAVE 20.1 / OCT 11.6 / QUAD 7.1 / PAIR 11.1; 24,576: QUAD 14.3 (two rounds of waves) /
 *     PAIR 11.2.  Between 32,768 and 49,152 checks the lane
 *     pair needs a second wave on some SIMDs (40,960: 20.5 ms), so AUTO runs the first 32,768 on
 *     PAIR (one wave per SIMD, 11.5 ms) and the rest by the rules above (WAVE / OCT / QUAD) on the same
 *     stream; above 49,152, whole rounds of 65,536 checks (two lane-pair waves per SIMD) run on
 *     PAIR and the remainder follows the same rules.
 * Retired (selecting them returns HBH_ERR_ARG): HBH_IMPL_THREAD (0, round 1's one-thread kernel),
 * HBH_IMPL_LANE_COOP (1, six lanes per check) and HBH_IMPL_THREAD_SIGNED (2, one thread per check
 * on signed limbs) -- WAVE and PAIR cover every batch size faster. */
#define HBH_IMPL_THREAD 0
#define HBH_IMPL_LANE_COOP 1
#define HBH_IMPL_THREAD_SIGNED 2
#define HBH_IMPL_AUTO 3
#define HBH_IMPL_PAIR 4
#define HBH_IMPL_WAVE 5
#define HBH_IMPL_QUAD 6
#define HBH_IMPL_OCT 7
#define HBH_IMPL_WAVE2 8
#define HBH_IMPL_WAVEP 10  /* 9 is not assigned */
#define HBH_AUTO_WAVEP_MIN 1025  /* AUTO: WAVEP for MIN <= checks <= MAX, before the ladder below (MIN 1 / MAX 0: never) */
#define HBH_AUTO_WAVEP_MAX 1536
#define HBH_AUTO_WAVE2_MAX 512  /* AUTO: WAVE2 up to here (two waves per check), then WAVE (profiles/r06/latency_c6.txt) */
#define HBH_AUTO_WAVE_MAX 4096
#define HBH_AUTO_OCT_MAX 8192
#define HBH_AUTO_QUAD_MAX 16384
#define HBH_AUTO_SPLIT_LO 32768  /* AUTO: (32,768, 49,152] checks = PAIR on 32,768 + the rest by size */
#define HBH_AUTO_SPLIT_HI 49152
#define HBH_AUTO_PAIR_ROUND 65536  /* AUTO above HBH_AUTO_SPLIT_HI: whole rounds of 65,536 on PAIR, the rest by size */
int hbh_engine_set_pairing_impl(hbh_engine* eng, int impl);
/* Ack-check kernel of hbh_bivar_ack_check_set: HBH_ACK_QUAD (k_bivar_check_quad: four lanes per ack
 * split each G1 operation, Jacobian rows -- latency), HBH_ACK_LANE (k_bivar_check: one lane per ack,
 * affine rows and mixed additions -- throughput), HBH_ACK_AUTO (default: LANE from HBH_ACK_LANE_MIN
 * acks per call; measured crossover ~50,000 acks, profiles/r03/ack_kernel_sweep.txt: 40,000 acks
 * quad 6.4 / lane 7.0 ms, 160,000 acks 18.9 / 13.1 ms, 10^6 acks 112 / 53 ms).  Same verdicts.
 * Round 5: on the LANE path (and AUTO's), the acks of a row whose y form a dense run (>= 2 (t + 1) acks
 * over <= twice as many consecutive y: a node's drain, one Ack per sender per Part) are checked by
 * finite differences -- t + 1 Horner points, then t G1 additions per further y;
 * HBH_ACK_LANE_HORNER keeps every ack on the Horner kernel (A/B, parity tests). */
#define HBH_ACK_AUTO 0
#define HBH_ACK_QUAD 1
#define HBH_ACK_LANE 2
#define HBH_ACK_LANE_HORNER 3
#define HBH_ACK_LANE_MIN 65536
int hbh_engine_set_ack_impl(hbh_engine* eng, int impl);

/* ---------------------------------------------------------------- profiling
 * With profiling on, the engine records HIP events around each stage's kernels on the stream they
 * run on; hbh_engine_stage_time returns the summed device time and launch count since the last
 * hbh_engine_set_profiling call. */
#define HBH_STAGE_PREPARE 0 /* Miller-loop line tables (G2 walks) */
#define HBH_STAGE_PAIRING 1 /* multi-Miller loop + final exponentiation */
#define HBH_STAGE_CURVE 2   /* scalar multiplication / interpolation / bivariate checks */
#define HBH_STAGE_HASH 4    /* hashing to G2: sampler rounds + cofactor multiplication (one entry per call) */
#define HBH_NUM_STAGES 5    /* 3 is not assigned: hbh_engine_stage_time keeps answering HBH_ERR_ARG for it */
int hbh_engine_set_profiling(hbh_engine* eng, int on);
int hbh_engine_stage_time(hbh_engine* eng, int stage, double* total_ms, int* launches);

/* ---------------------------------------------------------------- debug / test entry points
 * hbh_dbg_pairing: out[i] = e(P[i], Q[i])^3 as 12 canonical Fp2 coefficients (c0.c0.c0, c0.c0.c1,
 * c0.c1.c0, ... c1.c2.c1; 48 B LE each = 576 B) -- the pairing value itself, for parity tests
 * against the oracle (the kernel's final exponentiation uses the exponent 3(p^12-1)/r). */
int hbh_dbg_pairing(hbh_engine* eng, size_t n, const uint8_t* p, const uint8_t* q, uint8_t* out);
/* hbh_dbg_set_hash_rounds: sampler rounds of the device form of hash_g2 (1..1024; 0 restores
 * HBH_HASH_ROUNDS).  A low value leaves messages unresolved on purpose, for the tests of the host-stage
 * path of the leftovers and of hbh_hash_g2_dev's report. */
int hbh_dbg_set_hash_rounds(hbh_engine* eng, int rounds);
/* hbh_dbg_group_sums: the sums the grouped share checks feed their pairing checks, for parity tests:
 * out_g1[k] = sum of r_i g1_pts[i] and out_g2[k] = sum of r_i g2_pts[i] over the items with
 * group_idx[i] == k, k < ngroups (ABI points, all-zero when the sum is the point at infinity or no item
 * names k; groups of one item are summed too).  g1_pts / g2_pts may be NULL (that output is then not
 * written); scalars: n x 16 bytes little-endian, any value.  A group index >= ngroups is HBH_ERR_ARG. */
int hbh_dbg_group_sums(hbh_engine* eng, size_t n, const uint8_t* g1_pts, const uint8_t* g2_pts, size_t ngroups,
                       const uint32_t* group_idx, const uint8_t* scalars, uint8_t* out_g1, uint8_t* out_g2);
/* hbh_dbg_group_sums_form: the same sums with the scalars read in `form`: HBH_GFORM_INT128 (the bytes of
 * hbh_dbg_group_sums), HBH_GFORM_X4 or HBH_GFORM_X2 (the digit layouts of HBH_GSCALAR_DIGITS; any tuple, the
 * all-zero one contributes O).  The other arguments and the error rules are those of hbh_dbg_group_sums;
 * X2 with a G2 list, and any other form, are HBH_ERR_ARG (no call sums G2 points under X2). */
#define HBH_GFORM_INT128 0
#define HBH_GFORM_X4 1
#define HBH_GFORM_X2 2
int hbh_dbg_group_sums_form(hbh_engine* eng, int form, size_t n, const uint8_t* g1_pts, const uint8_t* g2_pts,
                            size_t ngroups, const uint32_t* group_idx, const uint8_t* scalars, uint8_t* out_g1,
                            uint8_t* out_g2);

#ifdef __cplusplus
}
#endif

#endif /* HBBFT_HIP_H */
