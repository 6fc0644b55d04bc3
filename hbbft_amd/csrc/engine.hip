// Host side of the C ABI (include/hbbft_hip.h): device/stream/workspace management and batch
// orchestration of the HIP kernels behind launch.hpp.  No CPU fallback: every verdict comes from
// the GPU; without a usable device the calls fail with HBH_ERR_DEVICE.  This file: the thread's last
// error, the engine's life and its settings; the call families are in engine_*.hip (engine_impl.hpp).
#include "engine_impl.hpp"

using namespace hbe;

namespace {
thread_local std::string g_last_error = "";

// one setting of the engine, under its lock; `refused`: why the value is none the setting takes, or null
int set_option(hbh_engine* e, int hbh_engine::*field, int value, const char* refused) {
  if (!e) return fail(HBH_ERR_ARG, "null engine");
  if (refused) return fail(HBH_ERR_ARG, refused);
  std::lock_guard<std::mutex> lk(e->mu);
  e->*field = value;
  return HBH_OK;
}
}  // namespace

int hbe::fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

extern "C" {

const char* hbh_last_error(void) { return g_last_error.c_str(); }

// Not part of the public ABI: lets pool.cpp report a shard's failure on the calling thread.
void hbh__set_error(const char* msg) { g_last_error = msg ? msg : ""; }

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
  delete e;  // every DevBuf of the engine frees its memory here, after the streams were drained
  return HBH_OK;
}

int hbh_engine_set_pairing_impl(hbh_engine* e, int impl) {
  const bool unknown = impl != HBH_IMPL_PAIR && impl != HBH_IMPL_AUTO && impl != HBH_IMPL_WAVE && impl != HBH_IMPL_QUAD &&
                       impl != HBH_IMPL_OCT && impl != HBH_IMPL_WAVE2 && impl != HBH_IMPL_WAVEP;
  return set_option(e, &hbh_engine::impl, impl, unknown ? "unknown or retired pairing implementation" : nullptr);
}

int hbh_engine_set_ack_impl(hbh_engine* e, int impl) {
  const bool unknown = impl != HBH_ACK_AUTO && impl != HBH_ACK_QUAD && impl != HBH_ACK_LANE && impl != HBH_ACK_LANE_HORNER;
  return set_option(e, &hbh_engine::ack_impl, impl, unknown ? "unknown Ack-check implementation" : nullptr);
}

int hbh_engine_set_decode_impl(hbh_engine* e, int impl) {
  const bool unknown = impl != HBH_DEC_AUTO && impl != HBH_DEC_LANE && impl != HBH_DEC_SPLIT;
  return set_option(e, &hbh_engine::dec_impl, impl, unknown ? "unknown point-decoding implementation" : nullptr);
}

int hbh_engine_set_group_sum_impl(hbh_engine* e, int impl) {
  const bool unknown = impl != HBH_GSUM_AUTO && impl != HBH_GSUM_CHAIN && impl != HBH_GSUM_BUCKET;
  return set_option(e, &hbh_engine::gsum_impl, impl, unknown ? "unknown group-sum implementation" : nullptr);
}

int hbh_engine_set_group_scalar_form(hbh_engine* e, int form) {
  const bool unknown = form != HBH_GSCALAR_INT128 && form != HBH_GSCALAR_DIGITS;
  return set_option(e, &hbh_engine::gscalar_form, form, unknown ? "unknown group scalar form" : nullptr);
}

int hbh_engine_set_hash_impl(hbh_engine* e, int impl) {
  const bool unknown = impl != HBH_HASH_AUTO && impl != HBH_HASH_HOST && impl != HBH_HASH_DEVICE;
  return set_option(e, &hbh_engine::hash_impl, impl, unknown ? "unknown hash-to-G2 implementation" : nullptr);
}

int hbh_engine_set_hash_form(hbh_engine* e, int form) {
  const bool unknown = form != HBH_HFORM_AUTO && form != HBH_HFORM_LANE && form != HBH_HFORM_QUAD;
  return set_option(e, &hbh_engine::hash_form, form, unknown ? "unknown hash-to-G2 device form" : nullptr);
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
