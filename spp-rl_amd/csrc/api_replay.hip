// libspprl C-ABI, the replay unit: the replay handle (ring writes, gathers, obs statistics: serial, side stream and
// both data-parallel paths), the MT19937 handle, and the free-standing stream utilities (sppRand*, synth env,
// episode accumulation, obs normalize).  Compiles replay.hip and stats.hip, and nothing of the agent: the agent
// reaches a ring through replay_dev / launch_replay_stage (host_base.h) alone.
#include <stdlib.h>

#include <algorithm>

#include "host_base.h"
#include "mlp.h"  // IC<N> (stats.hip)
#include "replay.h"

#include "replay.hip"
#include "stats.hip"

namespace spp {

// ================================================================== MT19937 (numpy legacy)
struct MT {
  uint32_t mt[624];
  int mti;
  void seed(uint32_t s) {
    mt[0] = s;
    for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    mti = 624;
  }
  uint32_t next() {
    if (mti >= 624) {
      for (int k = 0; k < 624; k++) {
        uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % 624] & 0x7fffffffu);
        mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      mti = 0;
    }
    uint32_t y = mt[mti++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
};

}  // namespace spp

struct sppMT19937 {
  spp::MT mt;
};

using namespace spp;

// ================================================================== replay handle
// sppReplayObsStats on a side stream beside the update's kernels (SPP_STATS_OVERLAP overrides, read when the
// handle is made).  On: faster on MI355X by the project's bench rule.
constexpr int kStatsOverlapDefault = 1;

struct sppReplay {
  ReplayDev d{};
  int device = 0, num_cu = 256;
  int64_t obs_idx = 0, ts_idx = 0, len = 0;
  // pinned ring for per-step index uploads
  static constexpr int kRing = 4;
  int64_t* pinned[kRing] = {};
  int64_t* dev_meta[kRing] = {};
  hipEvent_t ev[kRing] = {};
  int ring_cap = 0, ring_pos = 0;
  // obs-stats scratch
  double* st_part = nullptr;
  double* st_mean = nullptr;
  uint32_t* st_state = nullptr;
  uint32_t* st_hist = nullptr;
  // sample-bracketed single-device path (stats.hip)
  uint32_t *sf_samp = nullptr, *sf_bounds = nullptr, *sf_cpart = nullptr, *sf_wgl = nullptr, *sf_wgn = nullptr, *sf_ovf = nullptr,
           *sf_ovf_n = nullptr;
  double* sf_part = nullptr;
  // Ring generation: bumped by every entry point that can change the live rows (AddObs / AddStep /
  // Reset / GetView, whose caller may write).  sf_bounds holds the bracket of generation sf_gen
  // over sf_len rows: a later call on the same rows reuses it (the sample and its bracket would be
  // recomputed bit for bit).  Any bounds give the exact result (a rank outside the bracket falls
  // back to the raw column), so the generation only decides the cost, never the value.
  uint64_t gen = 0, sf_gen = ~0ull;
  int64_t sf_len = -1;
  bool bounds_dp1 = false;  // sf_bounds holds the union bracket of the last sppReplayObsStatsDP1 phase 1
  int st_cap_lim = 0, st_ovf_lim = 0;  // sppReplaySetObsStatsCaps (0: the full capacities)
  void* dp_q = nullptr;  // one-pass data-parallel statistics: per (column, target, rank) query state
  uint32_t* dp_cand = nullptr;  // and the compacted local candidates + counts
  // Side stream of sppReplayObsStats (SPP_STATS_OVERLAP): the statistics kernels run on `side`
  // (least priority, non-blocking) beside whatever the caller's stream still holds, and write `shadow`
  // [mean | std | max | min][ob]; k_st_publish copies it to the caller's arrays on the caller's stream.
  //   ev_rows     recorded on the writer's stream after the last ring write (AddObs / AddStep): side waits on it
  //   ev_done     recorded on side after each call's kernels: the publish, later ring writers and every other
  //               user of the sf_* scratch wait on it
  //   ev_scratch  recorded on a caller's stream after it used the sf_* scratch or refreshed the shadow itself
  //               (the serial path, the data-parallel paths): side waits on it once
  int overlap = 0;
  hipStream_t side = nullptr;
  hipEvent_t ev_rows = nullptr, ev_done = nullptr, ev_scratch = nullptr;
  bool rows_rec = false, done_rec = false, scratch_rec = false;
  float* shadow = nullptr;
  bool shadow_valid = false;  // shadow == the caller's arrays as of the last call (else: the serial path)
  bool view_open = false;     // gen was last bumped by GetView: the caller may write the rows at any time
  const float* last_out[4] = {};
  uint64_t n_overlapped = 0, n_serial = 0;
};

extern "C" {

sppStatus sppMTCreate(sppMTHandle* out, uint32_t seed) {
  SPP_REQUIRE(out, SPP_E_INVALID_ARG, "null out");
  auto* h = new sppMT19937;
  h->mt.seed(seed);
  *out = h;
  return SPP_OK;
}
sppStatus sppMTRandint(sppMTHandle h, int64_t high, int64_t n, int64_t* out) {
  SPP_REQUIRE(h && out && high >= 1 && high <= (int64_t)1 << 32, SPP_E_INVALID_ARG, "randint: bad args (high=%lld)",
              (long long)high);
  const uint64_t rng = (uint64_t)(high - 1);
  if (rng == 0) {
    for (int64_t i = 0; i < n; ++i) out[i] = 0;
    return SPP_OK;
  }
  uint64_t mask = rng;
  mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
  for (int64_t i = 0; i < n; ++i) {
    uint32_t v;
    do { v = h->mt.next() & (uint32_t)mask; } while (v > rng);
    out[i] = v;
  }
  return SPP_OK;
}
sppStatus sppMTDestroy(sppMTHandle h) {
  delete h;
  return SPP_OK;
}

sppStatus sppRandNormal(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
  SPP_REQUIRE(out || n == 0, SPP_E_INVALID_ARG, "null out");
  if (n == 0) return SPP_OK;
  const int64_t groups = (n + 3) / 4;
  hipLaunchKernelGGL(k_rand_normal, dim3(cdiv(groups, 256)), dim3(256), 0, S(stream), out, n, seed, offset);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}
sppStatus sppRandIndex(int64_t* out, int64_t n, int64_t high, uint64_t seed, uint64_t offset, void* stream) {
  SPP_REQUIRE((out || n == 0) && high >= 1, SPP_E_INVALID_ARG, "bad args");
  if (n == 0) return SPP_OK;
  hipLaunchKernelGGL(k_rand_index, dim3(cdiv(n, 256)), dim3(256), 0, S(stream), out, n, high, seed, offset);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

// ------------------------------------------------------------------ replay
sppStatus sppReplayCreate(sppReplayHandle* out, int64_t cap, int ob, int aout, int ac, int device) {
  SPP_REQUIRE(out && cap > 0 && ob > 0 && aout > 0 && ac > 0, SPP_E_INVALID_ARG, "replay create: bad args");
  SPP_REQUIRE(cap < (int64_t)1 << 31, SPP_E_INVALID_ARG, "replay create: capacity %lld >= 2^31 (32-bit slots)",
              (long long)cap);
  SPP_CHECK_HIP(hipSetDevice(device));
  auto* h = new sppReplay;
  h->device = device;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) h->num_cu = prop.multiProcessorCount;
  }
  ReplayDev& d = h->d;
  d.cap = cap;
  d.ob = ob;
  d.aout = aout;
  d.ac = ac;
  d.rw = rec_words(aout, ac);
  hipError_t e = hipSuccess;
  e = e ? e : hipMalloc(&d.obs, sizeof(float) * cap * ob);
  e = e ? e : hipMalloc(&d.obs_idx, sizeof(int64_t) * cap);
  e = e ? e : hipMalloc(&d.rec, sizeof(uint32_t) * cap * d.rw);  // (hipMalloc: 256-B aligned, records 64 B)
  e = e ? e : hipMemset(d.obs, 0, sizeof(float) * cap * ob);
  e = e ? e : hipMemset(d.obs_idx, 0, sizeof(int64_t) * cap);
  e = e ? e : hipMemset(d.rec, 0, sizeof(uint32_t) * cap * d.rw);
  if (e != hipSuccess) {
    set_error("replay alloc (%lld x %d): %s", (long long)cap, ob, hipGetErrorString(e));
    delete h;
    return SPP_E_OOM;
  }
  for (int i = 0; i < sppReplay::kRing; ++i) SPP_CHECK_HIP(hipEventCreateWithFlags(&h->ev[i], hipEventDisableTiming));
  {
    const char* e = getenv("SPP_STATS_OVERLAP");
    h->overlap = (e && *e) ? (atoi(e) != 0) : kStatsOverlapDefault;
  }
  *out = h;
  return SPP_OK;
}

// ---- side stream of the obs statistics (the fields' comment in sppReplay)
static sppStatus side_ensure(sppReplayHandle h) {
  if (h->side) return SPP_OK;
  int cur = 0;
  SPP_CHECK_HIP(hipGetDevice(&cur));
  if (cur != h->device) SPP_CHECK_HIP(hipSetDevice(h->device));
  int least = 0, greatest = 0;
  hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
  // non-blocking: the caller's stream may be the null stream, which a blocking stream would wait for
  e = e ? e : hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, least);
  e = e ? e : hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming);
  e = e ? e : hipEventCreateWithFlags(&h->ev_scratch, hipEventDisableTiming);
  e = e ? e : hipMalloc(&h->shadow, sizeof(float) * 4 * h->d.ob);
  if (cur != h->device) hipSetDevice(cur);
  SPP_CHECK_HIP(e);
  return SPP_OK;
}
// before a ring write, or a use of the sf_* scratch, on stream st: the side stream's last statistics call is done
static sppStatus side_wait_done(sppReplayHandle h, hipStream_t st) {
  if (h->done_rec) SPP_CHECK_HIP(hipStreamWaitEvent(st, h->ev_done, 0));
  return SPP_OK;
}
// after the last ring write of an entry point on stream st
static sppStatus side_rows_written(sppReplayHandle h, hipStream_t st) {
  h->view_open = false;
  if (!h->overlap) return SPP_OK;
  if (!h->ev_rows) SPP_CHECK_HIP(hipEventCreateWithFlags(&h->ev_rows, hipEventDisableTiming));
  SPP_CHECK_HIP(hipEventRecord(h->ev_rows, st));
  h->rows_rec = true;
  return SPP_OK;
}
// after stream st used the sf_* scratch (and perhaps wrote the caller's statistics arrays) itself
static sppStatus side_scratch_used(sppReplayHandle h, hipStream_t st, bool shadow_stale) {
  if (shadow_stale) h->shadow_valid = false;
  if (!h->side) return SPP_OK;
  SPP_CHECK_HIP(hipEventRecord(h->ev_scratch, st));
  h->scratch_rec = true;
  return SPP_OK;
}

sppStatus sppReplayDestroy(sppReplayHandle h) {
  if (!h) return SPP_OK;
  hipSetDevice(h->device);
  if (h->side) hipStreamSynchronize(h->side);
  hipDeviceSynchronize();
  if (h->side) hipStreamDestroy(h->side);
  if (h->ev_rows) hipEventDestroy(h->ev_rows);
  if (h->ev_done) hipEventDestroy(h->ev_done);
  if (h->ev_scratch) hipEventDestroy(h->ev_scratch);
  hipFree(h->shadow);
  ReplayDev& d = h->d;
  hipFree(d.obs); hipFree(d.obs_idx); hipFree(d.rec); hipFree((void*)d.acm_cols);
  for (int i = 0; i < sppReplay::kRing; ++i) {
    if (h->pinned[i]) hipHostFree(h->pinned[i]);
    if (h->dev_meta[i]) hipFree(h->dev_meta[i]);
    hipEventDestroy(h->ev[i]);
  }
  hipFree(h->st_part); hipFree(h->st_mean); hipFree(h->st_state); hipFree(h->st_hist);
  hipFree(h->sf_samp); hipFree(h->sf_bounds); hipFree(h->sf_part); hipFree(h->sf_cpart); hipFree(h->sf_wgl); hipFree(h->sf_wgn);
  hipFree(h->sf_ovf); hipFree(h->sf_ovf_n); hipFree(h->dp_q); hipFree(h->dp_cand);
  delete h;
  return SPP_OK;
}

sppStatus sppReplayAddObs(sppReplayHandle h, const float* obs, int E, int64_t* slots, void* stream) {
  SPP_REQUIRE(h && obs && E > 0 && E <= h->d.cap, SPP_E_INVALID_ARG, "add_obs: bad args");
  const int64_t base = h->obs_idx;
  ++h->gen;
  sppStatus sw = side_wait_done(h, S(stream));  // a statistics call on the side stream may still read the rows
  if (sw) return sw;
  hipLaunchKernelGGL(k_replay_add_obs, dim3(cdiv((int64_t)E * h->d.ob, 256)), dim3(256), 0, S(stream), h->d.obs,
                     h->d.cap, h->d.ob, obs, E, base);
  SPP_CHECK_HIP(hipGetLastError());
  sw = side_rows_written(h, S(stream));
  if (sw) return sw;
  for (int e = 0; e < E; ++e) {
    if (slots) slots[e] = (base + e) % h->d.cap;
  }
  h->obs_idx = (base + E) % h->d.cap;
  return SPP_OK;
}

// pinned host / device metadata ring of the per-step (prev, next, ts) uploads, >= E entries
static sppStatus ring_reserve(sppReplayHandle h, int E) {
  if (E <= h->ring_cap) return SPP_OK;
  hipDeviceSynchronize();
  for (int i = 0; i < sppReplay::kRing; ++i) {
    if (h->pinned[i]) hipHostFree(h->pinned[i]);
    if (h->dev_meta[i]) hipFree(h->dev_meta[i]);
    h->pinned[i] = nullptr;
    h->dev_meta[i] = nullptr;
    SPP_CHECK_HIP(hipHostMalloc(&h->pinned[i], sizeof(int64_t) * 3 * E));
    SPP_CHECK_HIP(hipMalloc(&h->dev_meta[i], sizeof(int64_t) * 3 * E));
  }
  h->ring_cap = E;
  return SPP_OK;
}

sppStatus sppReplayAddStep(sppReplayHandle h, const int64_t* prev, const int64_t* next, int E, const float* act,
                           const float* acm, const float* rew, const uint8_t* done, const uint8_t* end, void* stream) {
  SPP_REQUIRE(h && prev && next && E > 0 && rew && done && end, SPP_E_INVALID_ARG, "add_step: bad args");
  // A refused call leaves no trace: every env's slots are checked before anything changes, and the wrap rule
  // runs on copies of the cursors that are stored (with the metadata slot and the generation) only once the
  // whole batch has passed.
  for (int e = 0; e < E; ++e)
    SPP_REQUIRE(prev[e] >= 0 && prev[e] < h->d.cap && next[e] >= 0 && next[e] < h->d.cap, SPP_E_INVALID_ARG,
                "add_step: slot out of range");
  sppStatus rs = ring_reserve(h, E);
  if (rs) return rs;
  const int slot = h->ring_pos;
  SPP_CHECK_HIP(hipEventSynchronize(h->ev[slot]));  // the copy that last used this slot is done
  int64_t* m = h->pinned[slot];
  // add_timestep wrap rule (replay_buffer.py:65-75) applied sequentially in env order
  int64_t ts_idx = h->ts_idx, len = h->len;
  for (int e = 0; e < E; ++e) {
    m[e] = prev[e];
    m[E + e] = next[e];
    m[2 * E + e] = ts_idx;
    if (next[e] < ts_idx) {
      len = ts_idx + 1;
      ts_idx = 0;
    } else {
      ts_idx += 1;
    }
    len = std::max(ts_idx, len);
    SPP_REQUIRE(ts_idx <= h->d.cap, SPP_E_STATE, "add_step: ts ring overflow (obs ring too small)");
    if (ts_idx == h->d.cap) ts_idx = h->d.cap - 1;  // unreachable with the reference wrap rule
  }
  h->ts_idx = ts_idx;
  h->len = len;
  h->ring_pos = (slot + 1) % sppReplay::kRing;
  ++h->gen;
  SPP_CHECK_HIP(hipMemcpyAsync(h->dev_meta[slot], m, sizeof(int64_t) * 3 * E, hipMemcpyHostToDevice, S(stream)));
  SPP_CHECK_HIP(hipEventRecord(h->ev[slot], S(stream)));
  sppStatus sw = side_wait_done(h, S(stream));  // k_st_pass on the side stream reads obs_idx
  if (sw) return sw;
  const int64_t n_el = (int64_t)E * (h->d.aout + h->d.ac + 1);
  hipLaunchKernelGGL(k_replay_add_step, dim3(cdiv(n_el, 256)), dim3(256), 0, S(stream), h->d, h->dev_meta[slot], E,
                     act, acm, rew, done, end);
  SPP_CHECK_HIP(hipGetLastError());
  return side_rows_written(h, S(stream));
}

sppStatus sppReplayState(sppReplayHandle h, int64_t* obs_idx, int64_t* ts_idx, int64_t* len) {
  SPP_REQUIRE(h, SPP_E_INVALID_ARG, "null handle");
  if (obs_idx) *obs_idx = h->obs_idx;
  if (ts_idx) *ts_idx = h->ts_idx;
  if (len) *len = h->len;
  return SPP_OK;
}
sppStatus sppReplayReset(sppReplayHandle h) {
  SPP_REQUIRE(h, SPP_E_INVALID_ARG, "null handle");
  h->obs_idx = h->ts_idx = h->len = 0;
  ++h->gen;  // (no device write: the last rows event still covers every row)
  h->view_open = false;
  return SPP_OK;
}

sppStatus sppReplayGather(sppReplayHandle h, const int64_t* idx, int B, float* obs, float* nobs, float* act,
                          float* rew, int8_t* done, float* acm, void* stream) {
  SPP_REQUIRE(h && idx && B > 0, SPP_E_INVALID_ARG, "gather: bad args");
  hipLaunchKernelGGL(k_replay_gather_rm, dim3(cdiv(B, 256)), dim3(256), 0, S(stream), h->d, idx, B, obs, nobs, act,
                     rew, done, acm);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppReplaySetAcmColumns(sppReplayHandle h, const int* cols, int n) {
  SPP_REQUIRE(h && (n == 0 || (cols && n == h->d.ob)), SPP_E_INVALID_ARG,
              "acm columns: %d columns for ob = %d (acm_cat feeds the AcM 2 x len(acm_ob_idx) inputs, which it takes "
              "only when len(acm_ob_idx) = ob)", n, h ? h->d.ob : 0);
  for (int i = 0; i < n; ++i)
    SPP_REQUIRE(cols[i] >= 0 && cols[i] < h->d.ob, SPP_E_INVALID_ARG, "acm columns: index %d out of range", cols[i]);
  SPP_CHECK_HIP(hipSetDevice(h->device));
  SPP_CHECK_HIP(hipDeviceSynchronize());  // (a gather in flight may still read the old map)
  SPP_CHECK_HIP(hipFree((void*)h->d.acm_cols));
  h->d.acm_cols = nullptr;
  if (n == 0) return SPP_OK;
  int* d = nullptr;
  SPP_CHECK_HIP(hipMalloc(&d, sizeof(int) * n));
  SPP_CHECK_HIP(hipMemcpy(d, cols, sizeof(int) * n, hipMemcpyHostToDevice));
  h->d.acm_cols = d;
  return SPP_OK;
}

sppStatus sppReplayGatherAcm(sppReplayHandle h, const int64_t* idx, int B, float* x, float* y, void* stream) {
  SPP_REQUIRE(h && idx && x && y && B > 0, SPP_E_INVALID_ARG, "gather_acm: bad args");
  hipLaunchKernelGGL(k_replay_gather_acm, dim3(cdiv(B, kStageTile)), dim3(256), 0, S(stream), h->d, idx, B, x, y);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppReplayGetView(sppReplayHandle h, sppReplayView* v) {
  SPP_REQUIRE(h && v, SPP_E_INVALID_ARG, "null");
  ++h->gen;  // the caller may write the ring through the view
  // ... on any stream and at any time from now on, unseen by the library: the side stream drains here, and
  // sppReplayObsStats stays on its caller's stream until AddObs / AddStep / Reset write through the library again
  if (h->side) SPP_CHECK_HIP(hipStreamSynchronize(h->side));
  h->view_open = true;
  v->obs = h->d.obs;
  v->obs_idx = h->d.obs_idx;
  v->rec = h->d.rec;
  v->rec_words = h->d.rw;
  v->rec_acm = kRecAcm;
  v->rec_act = rec_act(h->d);
  return SPP_OK;
}

// §8b form of the constructor.  n_envs sizes the pinned per-step metadata ring up front;
// compat_mode 1 is the reference obs-index ring with the Q6 wrap rule (the only ring the
// reference has); store_fp64 0: the reference's float64 arrays only ever receive float32
// values (torch float32 obs, actions and rewards), so float32 storage is exact (Q5).
sppStatus sppReplayCreateEx(sppReplayHandle* out, int64_t cap, int ob, int aout, int ac, int n_envs,
                            int compat_mode, int store_fp64, int device) {
  SPP_REQUIRE(compat_mode == 1, SPP_E_INVALID_ARG,
              "replay create: compat_mode %d (only 1, the reference obs-index ring with the Q6 wrap, exists)",
              compat_mode);
  SPP_REQUIRE(store_fp64 == 0, SPP_E_INVALID_ARG,
              "replay create: store_fp64 %d (float32 storage is exact for every value the reference stores, Q5)",
              store_fp64);
  SPP_REQUIRE(n_envs > 0, SPP_E_INVALID_ARG, "replay create: n_envs %d", n_envs);
  sppStatus s = sppReplayCreate(out, cap, ob, aout, ac, device);
  if (s) return s;
  s = ring_reserve(*out, n_envs);
  if (s) {
    sppReplayDestroy(*out);
    *out = nullptr;
  }
  return s;
}

// BufferAcMOffPolicy.last_rollout (replay_buffer.py:335-383): the last complete episode is the
// *length timesteps first, first+1, ... (cyclic over [0, current_len)) ending at the last `end`
// at or before ts_idx - 1 (last_end, :170-177).  Synchronous (returns host values).
sppStatus sppReplayLastRollout(sppReplayHandle h, int64_t* first, int64_t* length, void* stream) {
  SPP_REQUIRE(h && first && length, SPP_E_INVALID_ARG, "last_rollout: null");
  const int64_t len = h->len;
  SPP_REQUIRE(len > 0, SPP_E_STATE, "last_rollout: empty buffer");
  hipStream_t st = S(stream);
  if (h->ts_idx == 0 && len == h->d.cap) {
    // python index ts_idx - 1 = -1 is the array's last element; when it is an end, the reference's
    // walk wraps to that same element at once (i = -2 -> current_len - 1) and stops: a 1-step rollout
    uint32_t w3 = 0;  // the last record's done | end word
    SPP_CHECK_HIP(hipMemcpyAsync(&w3, h->d.rec + (len - 1) * h->d.rw + 3, 4, hipMemcpyDeviceToHost, st));
    SPP_CHECK_HIP(hipStreamSynchronize(st));
    if ((w3 >> 8) & 1u) {
      *first = len - 1;
      *length = 1;
      return SPP_OK;
    }
  }
  const int64_t p = h->ts_idx > 0 ? std::min(h->ts_idx - 1, len - 1) : len - 1;
  int64_t* d = nullptr;
  SPP_CHECK_HIP(hipMallocAsync((void**)&d, 2 * sizeof(int64_t), st));
  hipLaunchKernelGGL(k_replay_last_rollout, dim3(1), dim3(1024), 0, st, (const uint32_t*)h->d.rec, h->d.rw, len, p,
                     d);
  int64_t hb[2] = {-1, -1};
  SPP_CHECK_HIP(hipMemcpyAsync(hb, d, sizeof(hb), hipMemcpyDeviceToHost, st));
  SPP_CHECK_HIP(hipFreeAsync(d, st));
  SPP_CHECK_HIP(hipStreamSynchronize(st));
  SPP_REQUIRE(hb[0] >= 0 && hb[1] >= 0, SPP_E_STATE, "last_rollout: no episode end in the buffer");
  int64_t T = (hb[0] - hb[1]) % len;
  if (T <= 0) T += len;
  *first = (hb[1] + 1) % len;
  *length = T;
  return SPP_OK;
}

static sppStatus stats_alloc(sppReplayHandle h) {
  const int ob = h->d.ob;
  const int G = std::min(ob, 32);
  if (!h->st_part) {
    SPP_CHECK_HIP(hipMalloc(&h->st_part, sizeof(double) * kStatsBlocks * ob * 2));
    SPP_CHECK_HIP(hipMalloc(&h->st_mean, sizeof(double) * ob * 2));
    SPP_CHECK_HIP(hipMalloc(&h->st_state, sizeof(uint32_t) * ob * 4 * 3));
    SPP_CHECK_HIP(hipMalloc(&h->st_hist, sizeof(uint32_t) * std::max(ob, G * 4) * 256));
    SPP_CHECK_HIP(hipMemset(h->st_hist, 0, sizeof(uint32_t) * std::max(ob, G * 4) * 256));  // k_stats_sel re-zeroes
    static bool attr = false;
    if (!attr) {  // > 64 KiB dynamic LDS for wide observations
      hipFuncSetAttribute((const void*)k_stats_p1, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      // (k_stats_pk: at most [32][4][256] or [128][4][64] counters = 128 KiB, beside its 4 KiB static table)
      hipFuncSetAttribute((const void*)k_stats_pk, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
      attr = true;
    }
  }
  return SPP_OK;
}

static void stats_pass1(sppReplayHandle h, uint32_t* hist, const float* pivot, hipStream_t st) {
  const int ob = h->d.ob;
  const size_t lds1 = sizeof(uint32_t) * (((ob * 256 + 1) & ~1)) + sizeof(double) * 16 * 16 * 2;
  hipLaunchKernelGGL(k_stats_p1, dim3(kStatsBlocks), dim3(256), lds1, st, h->d, h->len, hist, h->st_part, pivot);
}

// digit pass p (0-based) after the top byte, all columns: 8-bit digits at bits 16, 8, 0 when the
// [ob][4][256] LDS histogram fits 128 KiB (ob <= 32), else 6-bit digits at bits 18, 12, 6, 0
static int stats_dbits(sppReplayHandle h) { return h->d.ob <= 32 ? 8 : 6; }
static int stats_npass(sppReplayHandle h) { return 24 / stats_dbits(h); }
static int stats_shift(sppReplayHandle h, int p) { return 24 - stats_dbits(h) * (p + 1); }

static void stats_pk(sppReplayHandle h, int p, uint32_t* hist, hipStream_t st) {
  const size_t ldsk = sizeof(uint32_t) * h->d.ob * 4 * (1u << stats_dbits(h));
  // one 1024-thread block per CU (each flushes its LDS histogram with device atomics at the end)
  const int resident = 1;
  hipLaunchKernelGGL(k_stats_pk, dim3(h->num_cu * resident), dim3(kStatsPkThreads), ldsk, st, h->d, h->len,
                     stats_shift(h, p), stats_dbits(h), (const uint32_t*)h->st_state, hist);
}

static void stats_sel(sppReplayHandle h, int p, uint32_t* hist, int64_t n, float* max_obs, float* min_obs,
                      int first_update, hipStream_t st) {
  hipLaunchKernelGGL(k_stats_sel, dim3(h->d.ob), dim3(256), 0, st, hist, kStatsBlocks, h->d.ob, 0, h->d.ob,
                     stats_shift(h, p), stats_dbits(h), 0, (const double*)nullptr, n, h->st_state, h->st_mean,
                     max_obs, min_obs,
                     first_update);
}

static int st_nblk(sppReplayHandle h) {  // every pass workgroup resident at once (4 per CU)
  return std::max(1, std::min(kStNblkMax, 4 * h->num_cu));
}

// candidate-list capacities of the sample-bracketed statistics (sppReplaySetObsStatsCaps may lower them so
// the overflow paths run at small sizes; the allocations keep the full strides)
static int st_cap(sppReplayHandle h) {
  const int c = st_list_cap(h->d.ob);
  return h->st_cap_lim > 0 ? std::min(c, h->st_cap_lim) : c;
}
static int st_ovf_cap(sppReplayHandle h) {
  return h->st_ovf_lim > 0 ? std::min(kStOvfCap, h->st_ovf_lim) : kStOvfCap;
}

sppStatus sppReplaySetObsStatsCaps(sppReplayHandle h, int list_cap, int ovf_cap) {
  SPP_REQUIRE(h && list_cap >= 0 && ovf_cap >= 0, SPP_E_INVALID_ARG, "set_obs_stats_caps: bad args");
  if (h->side) SPP_CHECK_HIP(hipStreamSynchronize(h->side));  // (a test hook: no statistics call in flight across it)
  h->st_cap_lim = list_cap;
  h->st_ovf_lim = ovf_cap;
  return SPP_OK;
}

static sppStatus stats_fast_alloc(sppReplayHandle h) {
  if (h->sf_bounds) return SPP_OK;
  const int ob = h->d.ob, nb = kStNblkMax;
  SPP_CHECK_HIP(hipMalloc(&h->sf_bounds, sizeof(uint32_t) * ob * 4));
  SPP_CHECK_HIP(hipMalloc(&h->sf_samp, sizeof(uint32_t) * (size_t)ob * kStSampBig));
  SPP_CHECK_HIP(hipMalloc(&h->sf_part, sizeof(double) * nb * ob * 2));
  SPP_CHECK_HIP(hipMalloc(&h->sf_cpart, sizeof(uint32_t) * nb * ob * 6));
  SPP_CHECK_HIP(hipMalloc(&h->sf_wgl, sizeof(uint32_t) * (size_t)nb * ob * 2 * st_list_cap(ob)));
  SPP_CHECK_HIP(hipMalloc(&h->sf_wgn, sizeof(uint32_t) * (size_t)nb * ob * 2));
  SPP_CHECK_HIP(hipMalloc(&h->sf_ovf, sizeof(uint32_t) * (size_t)ob * 2 * kStOvfCap));
  SPP_CHECK_HIP(hipMalloc(&h->sf_ovf_n, sizeof(uint32_t) * ob * 2));
  SPP_CHECK_HIP(hipMemset(h->sf_ovf_n, 0, sizeof(uint32_t) * ob * 2));  // k_st_select re-zeroes
  return SPP_OK;
}

static sppStatus stats_chain(sppReplayHandle h, int64_t len, int nblk, float* mean, float* std, float* max_obs,
                             float* min_obs, int first_update, hipStream_t st);

sppStatus sppReplayObsStats(sppReplayHandle h, float* mean, float* std, float* max_obs, float* min_obs,
                            int first_update, void* stream) {
  SPP_REQUIRE(h && mean && std && max_obs && min_obs, SPP_E_INVALID_ARG, "obs_stats: bad args");
  const int64_t len = h->len;
  if (len <= 10) return SPP_OK;  // replay_buffer.py:84
  const int ob = h->d.ob;
  SPP_REQUIRE(ob <= 128, SPP_E_SHAPE, "obs_stats: ob %d > 128", ob);
  const int nblk = st_nblk(h);
  // per-lane counters are 16-bit: rows per lane = len / (waves * G) < 65536
  SPP_REQUIRE(len / ((int64_t)nblk * (kStPassThreads / 64) * st_groups(ob)) < 60000, SPP_E_INVALID_ARG,
              "obs_stats: len too large");
  sppStatus s = stats_fast_alloc(h);
  if (s) return s;
  hipStream_t st = S(stream);
  float* const out[4] = {mean, std, max_obs, min_obs};
  if (!h->overlap) {
    ++h->n_serial;
    return stats_chain(h, len, nblk, mean, std, max_obs, min_obs, first_update, st);
  }
  s = side_ensure(h);
  if (s) return s;
  // The side stream is taken only when the library can prove that the shadow holds what the caller's arrays
  // will hold once the caller's stream reaches this point, and that it sees every write of the rows.
  bool same = true;
  for (int i = 0; i < 4; ++i) same = same && h->last_out[i] == out[i];
  const bool side_ok = h->shadow_valid && same && !first_update && !h->view_open && h->rows_rec;
  for (int i = 0; i < 4; ++i) h->last_out[i] = out[i];
  float* const sh[4] = {h->shadow, h->shadow + ob, h->shadow + 2 * ob, h->shadow + 3 * ob};
  if (!side_ok) {  // today's code on the caller's stream, then shadow <- the caller's arrays
    s = side_wait_done(h, st);  // the scratch is shared with the side stream's calls
    if (s) return s;
    s = stats_chain(h, len, nblk, mean, std, max_obs, min_obs, first_update, st);
    if (s) return s;
    const StPublishArgs ra{{sh[0], sh[1], sh[2], sh[3]}, {mean, std, max_obs, min_obs}, ob};
    hipLaunchKernelGGL(k_st_publish, dim3(4), dim3(128), 0, st, ra);
    SPP_CHECK_HIP(hipGetLastError());
    s = side_scratch_used(h, st, false);
    if (s) return s;
    h->shadow_valid = true;
    ++h->n_serial;
    return SPP_OK;
  }
  // Never a wait on anything recorded on st now: the update queued ahead of this call is what the kernels run
  // beside.  ev_rows was recorded behind the last ring write, ev_scratch behind the last serial use of the scratch.
  SPP_CHECK_HIP(hipStreamWaitEvent(h->side, h->ev_rows, 0));
  if (h->scratch_rec) {
    SPP_CHECK_HIP(hipStreamWaitEvent(h->side, h->ev_scratch, 0));
    h->scratch_rec = false;  // the side stream's own order covers it from here on
  }
  s = stats_chain(h, len, nblk, sh[0], sh[1], sh[2], sh[3], 0, h->side);
  if (s) return s;
  SPP_CHECK_HIP(hipEventRecord(h->ev_done, h->side));
  h->done_rec = true;
  SPP_CHECK_HIP(hipStreamWaitEvent(st, h->ev_done, 0));  // this call's chain only: a later record does not move it
  const StPublishArgs pa{{mean, std, max_obs, min_obs}, {sh[0], sh[1], sh[2], sh[3]}, ob};
  hipLaunchKernelGGL(k_st_publish, dim3(4), dim3(128), 0, st, pa);
  SPP_CHECK_HIP(hipGetLastError());
  ++h->n_overlapped;
  return SPP_OK;
}

sppStatus sppReplayObsStatsInvalidate(sppReplayHandle h) {
  SPP_REQUIRE(h, SPP_E_INVALID_ARG, "null handle");
  h->shadow_valid = false;
  return SPP_OK;
}
int sppReplayStatsOverlap(sppReplayHandle h) { return h ? h->overlap : -1; }
sppStatus sppReplayStatsOverlapCounts(sppReplayHandle h, uint64_t* overlapped, uint64_t* serial) {
  SPP_REQUIRE(h, SPP_E_INVALID_ARG, "null handle");
  if (overlapped) *overlapped = h->n_overlapped;
  if (serial) *serial = h->n_serial;
  return SPP_OK;
}

// The statistics kernels of one call on stream st, outputs to the given arrays (the caller's, or the shadow).
static sppStatus stats_chain(sppReplayHandle h, int64_t len, int nblk, float* mean, float* std, float* max_obs,
                             float* min_obs, int first_update, hipStream_t st) {
  const int ob = h->d.ob;
  const bool big = len > kStBigLen;
  const int ns = (int)std::min<int64_t>(len, big ? kStSampBig : kStSampSmall);
  if (h->sf_gen != h->gen || h->sf_len != len) {  // else: the same rows' bracket is in sf_bounds
    hipLaunchKernelGGL(k_st_sample, dim3(cdiv(ns, 256)), dim3(256), 0, st, h->d, len, ns, h->sf_samp);
    if (big)
      hipLaunchKernelGGL(k_st_bracket<kStSampBig / 1024>, dim3(ob), dim3(1024), 0, st, h->sf_samp, ns, h->sf_bounds,
                         ns, (int64_t)0, 4);
    else
      hipLaunchKernelGGL(k_st_bracket<kStSampSmall / 1024>, dim3(ob), dim3(1024), 0, st, h->sf_samp, ns,
                         h->sf_bounds, ns, (int64_t)0, 4);
    h->sf_gen = h->gen;
    h->sf_len = len;
    h->bounds_dp1 = false;
  }
  const int cap = st_cap(h), ovf_cap = st_ovf_cap(h);
  StPassArgs pa{h->d, len, h->sf_bounds, nullptr, h->sf_part, h->sf_cpart, h->sf_wgl, h->sf_wgn, h->sf_ovf,
                h->sf_ovf_n, cap, ovf_cap};
  st_launch_pass(pa, nblk, st);
  StSelArgs sa{h->d, len, nblk, cap, h->sf_part, h->sf_cpart, h->sf_bounds, h->sf_wgl, h->sf_wgn, h->sf_ovf,
               h->sf_ovf_n, nullptr, mean, std, max_obs, min_obs, first_update, ovf_cap};
  hipLaunchKernelGGL(k_st_select, dim3(ob, 2), dim3(kStSelThreads), 0, st, sa);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

// ---- data-parallel statistics, one data pass per call (stats.hip "data-parallel: one data pass")
int sppReplayObsStatsDP1SampleRows(sppReplayHandle h, int world, int64_t n_global) {
  if (!h || world < 1) return -1;
  const int S = n_global > kStBigLen ? kStSampBig : kStSampSmall;
  return std::max(1, S / world);
}

sppStatus sppReplayObsStatsDP1(sppReplayHandle h, int phase, int world, int rank, const float* pivot, uint32_t* samp,
                               double* exch, uint32_t* hist, int64_t n_global, float* mean, float* std,
                               float* max_obs, float* min_obs, int first_update, void* stream) {
  const bool reuse = phase == (1 | SPP_DP1_REUSE_BRACKET);
  if (reuse) phase = 1;
  SPP_REQUIRE(h && pivot && samp && exch && hist && mean && std && max_obs && min_obs && phase >= 0 && phase <= 6 &&
                  world >= 1 && rank >= 0 && rank < world,
              SPP_E_INVALID_ARG, "obs_stats_dp1: bad args (phase %d, rank %d of %d)", phase, rank, world);
  SPP_REQUIRE(n_global > 10 && n_global < ((int64_t)1 << 31), SPP_E_INVALID_ARG, "obs_stats_dp1: n_global %lld",
              (long long)n_global);
  const int ob = h->d.ob;
  SPP_REQUIRE(ob <= 128, SPP_E_SHAPE, "obs_stats_dp1: ob %d > 128", ob);
  const int64_t len = h->len;
  const int nblk = st_nblk(h);
  SPP_REQUIRE(len / ((int64_t)nblk * (kStPassThreads / 64) * st_groups(ob)) < 60000, SPP_E_INVALID_ARG,
              "obs_stats_dp1: len too large");
  sppStatus s = stats_fast_alloc(h);
  if (s) return s;
  if (!h->dp_q) {
    SPP_CHECK_HIP(hipMalloc(&h->dp_q, sizeof(DpQuery) * ob * 4));
    SPP_CHECK_HIP(hipMalloc(&h->dp_cand, sizeof(uint32_t) * ((size_t)ob * 2 * kDpCandCap + ob * 2)));
  }
  uint32_t* dp_ncand = h->dp_cand + (size_t)ob * 2 * kDpCandCap;
  hipStream_t st = S(stream);
  const int Sl = sppReplayObsStatsDP1SampleRows(h, world, n_global);
  uint32_t* mine = samp + (int64_t)rank * ob * Sl;
  const int cap = st_cap(h), ovf_cap = st_ovf_cap(h);
  s = side_wait_done(h, st);  // the sf_* scratch is shared with sppReplayObsStats' side stream
  if (s) return s;
  StDpArgs da{h->d, len, n_global, nblk, cap, ovf_cap, h->sf_bounds, h->sf_wgl, h->sf_wgn, h->sf_ovf, h->sf_ovf_n,
              h->dp_cand, dp_ncand, exch, hist, (DpQuery*)h->dp_q, pivot, mean, std, max_obs, min_obs, first_update};
  if (phase == 0) {
    if (len > 0) hipLaunchKernelGGL(k_st_sample, dim3(cdiv(Sl, 256)), dim3(256), 0, st, h->d, len, Sl, mine);
    else SPP_CHECK_HIP(hipMemsetAsync(mine, 0, sizeof(uint32_t) * ob * Sl, st));  // (lockstep shards: not reached)
  } else if (phase == 1) {
    const int S = world * Sl;  // <= kStSampBig
    // margin 5 sigma + 4 sample ranks: a miss costs the raw-column select of the rounds, not correctness.
    // reuse (decided alike on every rank): keep the last union bracket; if the N = 1 path overwrote the
    // bounds since, recompute them from samp (the same union sample on every rank)
    if (!(reuse && h->bounds_dp1)) {
      if (S > kStSampSmall)
        hipLaunchKernelGGL(k_st_bracket<kStSampBig / 1024>, dim3(ob), dim3(1024), 0, st, (const uint32_t*)samp, S,
                           h->sf_bounds, Sl, (int64_t)ob * Sl, 5);
      else
        hipLaunchKernelGGL(k_st_bracket<kStSampSmall / 1024>, dim3(ob), dim3(1024), 0, st, (const uint32_t*)samp, S,
                           h->sf_bounds, Sl, (int64_t)ob * Sl, 5);
      h->bounds_dp1 = true;
      h->sf_gen = ~0ull;  // the N = 1 path must not take these (union) bounds for its own
    }
    StPassArgs pa{h->d, len, h->sf_bounds, pivot, h->sf_part, h->sf_cpart, h->sf_wgl, h->sf_wgn, h->sf_ovf,
                  h->sf_ovf_n, cap, ovf_cap};
    st_launch_pass(pa, nblk, st);
    hipLaunchKernelGGL(k_dp_reduce, dim3(ob, 2), dim3(kStSelThreads), 0, st, ob, nblk, cap, ovf_cap,
                       (const double*)h->sf_part,
                       (const uint32_t*)h->sf_cpart, (const uint32_t*)h->sf_wgl, (const uint32_t*)h->sf_wgn,
                       (const uint32_t*)h->sf_ovf, (const uint32_t*)h->sf_ovf_n, exch, h->dp_cand, dp_ncand);
  } else if (phase <= 5) {
    hipLaunchKernelGGL(k_dp_round, dim3(ob, 2), dim3(kStSelThreads), 0, st, da, phase - 2);
  } else {
    hipLaunchKernelGGL(k_dp_final, dim3(ob, 2), dim3(128), 0, st, da);
  }
  SPP_CHECK_HIP(hipGetLastError());
  return side_scratch_used(h, st, true);  // (phase 6 writes the caller's arrays: the shadow is stale)
}

int sppReplayObsStatsDPHistSize(sppReplayHandle h) {
  if (!h) return -1;
  const int ob = h->d.ob;
  return std::max(ob, std::min(ob, 32) * 4) * 256;
}

sppStatus sppReplayObsStatsDP(sppReplayHandle h, int step, const float* pivot, double* sums, uint32_t* hist,
                              int64_t n_global, float* mean, float* std, float* max_obs, float* min_obs,
                              int first_update, int* done, void* stream) {
  SPP_REQUIRE(h && pivot && sums && hist && mean && std && max_obs && min_obs && done && step >= 0,
              SPP_E_INVALID_ARG, "obs_stats_dp: bad args");
  const int ob = h->d.ob;
  SPP_REQUIRE(ob <= 16 * kStatsColsPerThread, SPP_E_SHAPE, "obs_stats_dp: ob %d > %d", ob, 16 * kStatsColsPerThread);
  // counts travel as int32 (the host's fused first exchange converts fp64 sums back to int32)
  SPP_REQUIRE(n_global > 10 && n_global < ((int64_t)1 << 31), SPP_E_INVALID_ARG, "obs_stats_dp: n_global %lld",
              (long long)n_global);
  sppStatus s = stats_alloc(h);
  if (s) return s;
  hipStream_t st = S(stream);
  // (its scratch is st_*, its own; it writes the caller's arrays, so the side stream's shadow goes stale and
  // the caller's stream first passes every publish still queued)
  s = side_wait_done(h, st);
  if (s) return s;
  h->shadow_valid = false;
  const int npass = stats_npass(h);
  SPP_REQUIRE(step <= npass + 1, SPP_E_INVALID_ARG, "obs_stats_dp: step %d > %d", step, npass + 1);
  *done = 0;
  if (step == 0) {  // local pass 1 -> sums [ob][2] about the shared pivot, top-byte histogram
    SPP_CHECK_HIP(hipMemsetAsync(hist, 0, sizeof(uint32_t) * sppReplayObsStatsDPHistSize(h), st));
    if (h->len > 0) {
      stats_pass1(h, hist, pivot, st);
      hipLaunchKernelGGL(k_stats_reduce_part, dim3(ob), dim3(256), 0, st, (const double*)h->st_part, kStatsBlocks,
                         ob, sums);
    } else {
      SPP_CHECK_HIP(hipMemsetAsync(sums, 0, sizeof(double) * ob * 2, st));
    }
  } else {
    if (step == 1) {  // global top byte + moments
      hipLaunchKernelGGL(k_stats_sel, dim3(ob), dim3(256), 0, st, hist, 1, ob, 0, ob, 24, 8, 1, (const double*)sums,
                         n_global, h->st_state, h->st_mean, max_obs, min_obs, first_update);
      hipLaunchKernelGGL(k_stats_moments_out, dim3(1), dim3(128), 0, st, h->d, (const double*)h->st_mean, mean, std,
                         pivot);
    } else {
      stats_sel(h, step - 2, hist, n_global, max_obs, min_obs, first_update, st);
    }
    if (step - 1 < npass) {
      if (h->len > 0) stats_pk(h, step - 1, hist, st);
    } else {
      *done = 1;
    }
  }
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppSynthEnvStep(const float* A, const float* obs, const float* action, int E, int ob, int ac,
                          float* next_obs, float* reward, void* stream) {
  SPP_REQUIRE(A && obs && action && next_obs && reward && E > 0, SPP_E_INVALID_ARG, "synth env: bad args");
  hipLaunchKernelGGL(k_synth_env, dim3(cdiv((int64_t)E * ob, 256)), dim3(256), 0, S(stream), A, obs, action, E, ob, ac, next_obs,
                     reward);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}


sppStatus sppRandUniform(float* out, int64_t n, const float* lo, const float* hi, int period, uint64_t seed,
                         uint64_t offset, void* stream) {
  SPP_REQUIRE((out || n == 0) && lo && hi && period > 0, SPP_E_INVALID_ARG, "rand uniform: bad args");
  if (n == 0) return SPP_OK;
  hipLaunchKernelGGL(k_rand_uniform, dim3(cdiv((n + 3) / 4, 256)), dim3(256), 0, S(stream), out, n, lo, hi, period,
                     seed, offset);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppEpisodeAccum(const float* rew, const uint8_t* end, int E, float* ep_ret, double* sums, void* stream) {
  SPP_REQUIRE(rew && ep_ret && sums && E > 0, SPP_E_INVALID_ARG, "episode accum: bad args");
  hipLaunchKernelGGL(k_episode_accum, dim3(cdiv(E, 256)), dim3(256), 0, S(stream), rew, end, E, ep_ret, sums);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppSynthEnvReset(float* obs, const uint8_t* mask, int E, int ob, uint64_t seed, uint64_t offset,
                           void* stream) {
  SPP_REQUIRE(obs && E > 0 && ob > 0, SPP_E_INVALID_ARG, "synth reset: bad args");
  hipLaunchKernelGGL(k_synth_reset, dim3(cdiv((int64_t)E * ob, 256)), dim3(256), 0, S(stream), obs, mask, E, ob, seed,
                     offset);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

sppStatus sppObsNormalize(const float* x, int64_t rows, int ob, const float* lo, const float* hi, const float* mean,
                          const float* std, int min_max, int inverse, float* out, void* stream) {
  SPP_REQUIRE(x && out && rows >= 0 && ob > 0, SPP_E_INVALID_ARG, "normalize: bad args");
  SPP_REQUIRE(min_max ? (lo && hi) : (mean && std), SPP_E_INVALID_ARG, "normalize: missing statistics");
  if (rows == 0) return SPP_OK;
  const int64_t n = rows * ob;
  hipLaunchKernelGGL(k_obs_normalize, dim3(cdiv(n, 256)), dim3(256), 0, S(stream), x, n, ob, lo, hi, mean, std,
                     min_max, inverse, out);
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}
}  // extern "C"

// ---- the agent's side of the ring (api.hip: sppAgentStageFromReplay; host_base.h)
namespace spp {

const ReplayDev& replay_dev(sppReplayHandle r) { return r->d; }

void launch_replay_stage(const ReplayDev& d, const int64_t* idx, int B, int Bp, float* S, float* S2, float* act,
                         float* AENV, float* R, float* DN, hipStream_t st) {
  // Wide rows (Ant, ob > 64) stage faster with k_replay_stage_fm2 (four gathers before one barrier,
  // division-free lane geometry: 0.30 -> 0.22 ms at B = 409,600); narrow rows (Hopper, HalfCheetah)
  // are faster with the 64-sample tiles of k_replay_stage_fm (0.059 vs 0.128 ms, 0.154 vs 0.292 ms).
  if (d.ob > 64)
    hipLaunchKernelGGL(k_replay_stage_fm2, dim3(cdiv(Bp, kStage2Tile)), dim3(256),
                       stage2_lds_bytes(d.ob, d.aout, d.ac, act != nullptr), st, d, idx, B, Bp, S, S2, act, AENV, R,
                       DN);
  else
    hipLaunchKernelGGL(k_replay_stage_fm, dim3(cdiv(Bp, kStageTile)), dim3(256),
                       sizeof(float) * kStageTile * std::max(d.ob, d.aout), st, d, idx, B, Bp, S, S2, act, AENV, R, DN);
}

}  // namespace spp
