// api.cpp — the C ABI of libtfhe_hip.so (include/tfhe_hip.h): device shards, key residency and
// broadcast, launch sequencing, error reporting.  Host code; kernels live in the .hip files.
//
// An engine (tfhe_ctx) spans ndev device shards.  A shard = one device ordinal + its own stream,
// key copy, twiddle tables and workspaces.  Keys reach shard 0 through a pinned staging ring and the
// other shards by RCCL broadcast (distinct ordinals) or device copies (a repeated ordinal); host-buffer
// PBS batches split into contiguous slices that the shards run concurrently.
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/tfhe_hip.h"
#include "client.h"
#include "gl64.h"
#include "host_common.h"
#include "pbs_kernels.h"

using tfhe::u32;
using tfhe::u64;

namespace {

thread_local std::string g_err;  // tfhe_hip_last_error; written through tfhe_hip_set_error (fail())

bool params_valid(const tfhe_params* p) {
  return p && p->n > 0 && p->k > 0 && p->N >= 32 && (p->N & (p->N - 1)) == 0 && p->pbs_level > 0 &&
         p->pbs_base_log > 0 && p->pbs_base_log * p->pbs_level < 64 && p->ks_level > 0 && p->ks_base_log > 0 &&
         p->ks_base_log * p->ks_level < 64 && p->transform <= TFHE_HIP_TRANSFORM_FFT64;
}

// the presets = the parameter shapes the device kernels of this build cover (P-GATE: N = 1024, PBS -> KS; P-FHEVM:
// N = 2048, KS -> PBS), each on both transforms
const struct {
  int id;
  tfhe_params p;
} PRESETS[] = {
    {TFHE_HIP_PRESET_GATE, {630, 1, 1024, 7, 3, 2, 8, -15, -25, 0, TFHE_HIP_TRANSFORM_NTT}},
    {TFHE_HIP_PRESET_FHEVM, {918, 1, 2048, 23, 1, 4, 4, -19, -47, 1, TFHE_HIP_TRANSFORM_NTT}},
    {TFHE_HIP_PRESET_GATE_FFT, {630, 1, 1024, 7, 3, 2, 8, -15, -25, 0, TFHE_HIP_TRANSFORM_FFT64}},
    {TFHE_HIP_PRESET_FHEVM_FFT, {918, 1, 2048, 23, 1, 4, 4, -19, -47, 1, TFHE_HIP_TRANSFORM_FFT64}},
    // preset 3 with n divisible by 2, 3 and 4: the multi-bit keys' grouping factors (tfhe_hip_load_keys_mb)
    {TFHE_HIP_PRESET_FHEVM_MB_FFT, {924, 1, 2048, 23, 1, 4, 4, -19, -47, 1, TFHE_HIP_TRANSFORM_FFT64}},
};

// a preset's shape: everything the kernels are specialised for (n and the noise parameters are free)
bool params_on_device(const tfhe_params* p) {
  for (auto& r : PRESETS)
    if (p->k == r.p.k && p->N == r.p.N && p->pbs_base_log == r.p.pbs_base_log && p->pbs_level == r.p.pbs_level &&
        p->ks_base_log == r.p.ks_base_log && p->ks_level == r.p.ks_level && p->order == r.p.order &&
        p->transform == r.p.transform)
      return true;
  return false;
}

// ---- RCCL, loaded on first use (a process that already holds torch's librccl reuses that copy) -----------
struct Rccl {
  bool tried = false, ok = false;
  std::string why;
  ncclResult_t (*comm_init_all)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*bcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*group_start)() = nullptr;
  ncclResult_t (*group_end)() = nullptr;
  ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
  const char* (*err)(ncclResult_t) = nullptr;
};

Rccl& rccl() {
  static Rccl r;
  static std::mutex m;
  std::lock_guard<std::mutex> lk(m);
  if (r.tried) return r;
  r.tried = true;
  void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
  if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) {
    r.why = std::string("dlopen librccl.so.1: ") + dlerror();
    return r;
  }
  r.comm_init_all = (decltype(r.comm_init_all))dlsym(h, "ncclCommInitAll");
  r.bcast = (decltype(r.bcast))dlsym(h, "ncclBroadcast");
  r.group_start = (decltype(r.group_start))dlsym(h, "ncclGroupStart");
  r.group_end = (decltype(r.group_end))dlsym(h, "ncclGroupEnd");
  r.comm_destroy = (decltype(r.comm_destroy))dlsym(h, "ncclCommDestroy");
  r.err = (decltype(r.err))dlsym(h, "ncclGetErrorString");
  r.ok = r.comm_init_all && r.bcast && r.group_start && r.group_end && r.comm_destroy && r.err;
  if (!r.ok) r.why = "librccl.so.1 lacks ncclCommInitAll / ncclBroadcast / ncclGroupStart / ncclGroupEnd";
  return r;
}

}  // namespace

constexpr int TIMING_SLOTS = 4;

// One device's slice of an engine: a device slot (host_common.h) plus keys, tables and workspaces.
struct tfhe_shard : device_slot {
  int cus = 0;                  // compute units (queried once, shard_init)
  u64* d_bsk = nullptr;        // transform domain (NTT layout x N^-1, or Fourier)
  size_t bsk_cap = 0;          // bytes (a multi-bit key is larger than the classic one)
  u64* d_tw_mb = nullptr;      // the multi-bit back end's own tables (first tfhe_hip_load_keys_mb)
  u64* d_ksk = nullptr;         // standard KSK (VALU keyswitch; RCCL broadcast source / target)
  void* d_ks_planes = nullptr;  // KSK recoded into 8 signed byte planes (ks_mfma.hip)
  u64* d_tw = nullptr;          // twiddle tables of the device transform
  u64* d_ms_zeros = nullptr;    // modulus-switch noise reduction zeros (order 1)
  // workspaces, ordered across streams by the slot's ws_begin / ws_end
  u64* d_big = nullptr;
  size_t big_cap = 0;  // bytes
  u64* d_acc = nullptr;  // blind-rotation accumulators of a many-LUT PBS
  size_t acc_cap = 0;    // bytes
  u64* d_expand = nullptr;  // expanded compact list, the PBS input of tfhe_hip_expand_cast (d_big is the PBS's own)
  size_t expand_cap = 0;    // bytes
  u64* d_oprf = nullptr;  // seeded masks with body 0, the PBS input of tfhe_hip_oprf (rows x (n + 1))
  size_t oprf_cap = 0;    // bytes
  u64* d_lin = nullptr;  // assembled rows, the PBS input of tfhe_hip_lincomb_pbs (rows x (io_dim + 1))
  size_t lin_cap = 0;    // bytes
  // term description of a lincomb launch (lincomb_stage): packed on the host into one of two pinned slots, copied
  // into d_lin_meta; a slot is refilled only after the event recorded behind its previous copy
  void* d_lin_meta = nullptr;
  size_t lin_meta_cap = 0;  // bytes
  void* h_lin_meta[2] = {nullptr, nullptr};
  size_t h_lin_meta_cap[2] = {0, 0};  // bytes
  hipEvent_t lin_meta_done[2] = {nullptr, nullptr};
  bool lin_meta_used[2] = {false, false};
  int lin_meta_next = 0;
  void* d_ks_dig = nullptr;
  size_t ks_dig_cap = 0;  // bytes
  // timing: start/stop event pairs per slot (0 = blind rotate, 1 = keyswitch, 2 = MS noise reduction,
  // 3 = the ingest stage of a call: unpack / extract of a decompression, the expansion of a compact list, or the
  // seeded masks of tfhe_hip_oprf)
  std::vector<hipEvent_t> ev[TIMING_SLOTS];
  std::vector<hipEvent_t> ev_pool;
};

struct tfhe_ctx {
  tfhe_params p{};
  std::vector<tfhe_shard> sh;
  bool bsk = false;   // a BSK is resident: the rotation-only calls work (tfhe_hip_load_bsk or tfhe_hip_load_keys)
  bool keys = false;  // BSK and KSK of one key set: every call works (tfhe_hip_load_keys)
  bool ks_valu = false;  // TFHE_HIP_KS_VALU=1: the VALU keyswitch kernel instead (A/B runs)
  const tfhe::br_engine* eng = nullptr;  // the blind-rotation back end of (transform, N), set once in tfhe_hip_create
  size_t lat_max = 0;  // batches up to this size (per shard) run the latency kernel (default: eng->lat_max)
  uint32_t grouping = 1;  // 2..4: multi-bit keys are resident and every blind rotation runs eng_mb
  const tfhe::br_engine_mb* eng_mb = nullptr;  // the multi-bit back end on eng's ring, if any
  uint32_t ms_count = 0;
  double ms_bound = 0, ms_r_sigma = 0, ms_var128 = 0;
  int bcast_mode = 0;  // tfhe_hip_key_bcast_mode
  std::vector<ncclComm_t> comms;
  std::mutex mu;
  bool timing = false;
  double seeded_ms[3] = {0, 0, 0};  // the last seeded load on shard 0: upload, expansion, conversion (device ms)
};

namespace {

using shard = tfhe_shard;

hipEvent_t take_event(shard& s) {
  if (!s.ev_pool.empty()) {
    hipEvent_t e = s.ev_pool.back();
    s.ev_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

void timed_begin(tfhe_ctx* c, shard& s, int which, hipStream_t st) {
  if (!c->timing) return;
  hipEvent_t e = take_event(s);
  if (e) {
    (void)hipEventRecord(e, st);
    s.ev[which].push_back(e);
  }
}
void timed_end(tfhe_ctx* c, shard& s, int which, hipStream_t st) {
  if (!c->timing) return;
  if (s.ev[which].size() % 2 == 0) return;  // begin failed
  hipEvent_t e = take_event(s);
  if (e) {
    (void)hipEventRecord(e, st);
    s.ev[which].push_back(e);
  } else {
    s.ev_pool.push_back(s.ev[which].back());
    s.ev[which].pop_back();
  }
}

uint32_t io_dim(const tfhe_params& p) { return p.order == 0 ? p.n : p.k * p.N; }

// the one place that picks the blind-rotation kernel by batch size (launch_br, tfhe_hip_br_kernel)
bool latency_batch(const tfhe_ctx* c, size_t B) { return B <= c->lat_max; }

hipError_t launch_br(tfhe_ctx* c, shard& s, const u64* in, size_t B, const u64* luts, const u32* idx, size_t n_lut,
                     u64* out_big, u64* out_acc, hipStream_t st) {
  if (c->grouping > 1)
    return c->eng_mb->blind_rotate(in, B, (int)c->p.n, (int)c->grouping, luts, idx, (int)n_lut, s.d_bsk, s.d_tw,
                                   s.d_tw_mb, out_big, out_acc, st);
  return c->eng->blind_rotate(in, B, (int)c->p.n, luts, idx, (int)n_lut, s.d_bsk, s.d_tw, out_big, out_acc,
                              latency_batch(c, B), s.cus, st);
}

uint32_t log2u(uint32_t x) {
  uint32_t l = 0;
  while ((1u << l) < x) l++;
  return l;
}

hipError_t launch_ms(tfhe_ctx* c, shard& s, u64* small, size_t B, int* picks, hipStream_t st) {
  return tfhe::launch_ms_reduce(small, B, (int)c->p.n, s.d_ms_zeros, (int)c->ms_count, (int)log2u(2 * c->p.N),
                                c->ms_bound, c->ms_r_sigma, c->ms_var128, picks, st);
}

int launch_ks(tfhe_ctx* c, shard& s, const u64* in_big, size_t B, u64* out, hipStream_t st) {
  const int big_dim = (int)(c->p.k * c->p.N);
  if (c->ks_valu || !s.d_ks_planes) {
    HIP_TRY(tfhe::launch_keyswitch(in_big, B, big_dim, s.d_ksk, (int)c->p.n, (int)c->p.ks_base_log,
                                   (int)c->p.ks_level, out, st));
    return 0;
  }
  RC_TRY(ws_grow(s, &s.d_ks_dig, &s.ks_dig_cap, tfhe::ks_digits_bytes(B, big_dim, (int)c->p.ks_level)));
  HIP_TRY(tfhe::launch_keyswitch_mfma(in_big, B, big_dim, s.d_ks_planes, (int)c->p.n, (int)c->p.ks_base_log,
                                      (int)c->p.ks_level, s.d_ks_dig, out, st));
  return 0;
}

struct many_args {  // the many-LUT arguments of tfhe_hip_pbs_many*; a null pointer = plain PBS
  uint32_t n_fn, stride;
};

// what a PBS entry point runs: the parameter set's full PBS (keyswitch and rotation in its `order`, optionally
// many-LUT), or the rotation alone (tfhe_hip_bootstrap: B x (n+1) -> B x (kN+1), BSK only)
struct pbs_kind {
  const many_args* m = nullptr;
  bool rotation_only = false;
};

// Blind rotation + extraction of the degree-0 sample, B x (n+1) -> B x (kN+1), timed in slot 0.
int bootstrap_device(tfhe_ctx* c, shard& s, const u64* d_in, size_t B, const u64* d_luts, size_t n_lut,
                     const u32* d_idx, u64* d_out, hipStream_t st) {
  timed_begin(c, s, 0, st);
  HIP_TRY(launch_br(c, s, d_in, B, d_luts, d_idx, n_lut, d_out, nullptr, st));
  timed_end(c, s, 0, st);
  return 0;
}

// PBS on device buffers (caller holds c->mu and has set the shard's device; workspaces ordered by the
// caller's ws_begin / ws_end).  Order 0 (P-GATE): BR + SE -> KS; order 1 (P-FHEVM): KS -> [MS noise
// reduction] -> BR + SE.
// Plain PBS (m null): the blind rotation extracts its one sample itself, d_out: B x (io_dim + 1).
// Many-LUT PBS (m, checked by check_many): the rotation writes the shard's accumulator workspace and
// sample_extract_many.hip takes the samples at degrees f * stride, f < n_fn, timed with the rotation in slot 0;
// order 0 then keyswitches the n_fn * B rows.  d_out: B x n_fn x (io_dim + 1), ciphertext-major.
int pbs_device(tfhe_ctx* c, shard& s, const u64* d_in, size_t B, const u64* d_luts, size_t n_lut, const u32* d_idx,
               const many_args* m, u64* d_out, hipStream_t st) {
  const size_t big = (size_t)c->p.k * c->p.N + 1, small = (size_t)c->p.n + 1;
  const size_t rows = B * (m ? m->n_fn : 1);
  RC_TRY(ws_grow(s, (void**)&s.d_big, &s.big_cap, (c->p.order == 0 ? rows * big : B * small) * sizeof(u64)));
  if (m) RC_TRY(ws_grow(s, (void**)&s.d_acc, &s.acc_cap, B * (size_t)(c->p.k + 1) * c->p.N * sizeof(u64)));
  auto rotate = [&](const u64* in, u64* out) -> int {  // blind rotation + sample extraction, slot 0
    timed_begin(c, s, 0, st);
    if (m) {
      HIP_TRY(launch_br(c, s, in, B, d_luts, d_idx, n_lut, nullptr, s.d_acc, st));
      HIP_TRY(tfhe::launch_sample_extract_many(s.d_acc, B, (int)c->p.k, (int)c->p.N, !c->eng->fft, (int)m->n_fn,
                                               (int)m->stride, out, st));
    } else {
      HIP_TRY(launch_br(c, s, in, B, d_luts, d_idx, n_lut, out, nullptr, st));
    }
    timed_end(c, s, 0, st);
    return 0;
  };
  if (c->p.order == 0) {
    RC_TRY(rotate(d_in, s.d_big));
    timed_begin(c, s, 1, st);
    RC_TRY(launch_ks(c, s, s.d_big, rows, d_out, st));
    timed_end(c, s, 1, st);
  } else {
    timed_begin(c, s, 1, st);
    RC_TRY(launch_ks(c, s, d_in, B, s.d_big, st));
    timed_end(c, s, 1, st);
    if (c->ms_count) {
      timed_begin(c, s, 2, st);
      HIP_TRY(launch_ms(c, s, s.d_big, B, nullptr, st));
      timed_end(c, s, 2, st);
    }
    RC_TRY(rotate(s.d_big, d_out));
  }
  return 0;
}

// n_fn functions at degrees f * stride of an N-coefficient accumulator, B inputs
int check_many(const tfhe_ctx* c, const char* what, size_t B, uint32_t n_fn, uint32_t stride) {
  if (n_fn < 1 || stride < 1) return fail(TFHE_HIP_EINVAL, "%s: n_fn = %u, stride = %u (both must be >= 1)", what, n_fn, stride);
  if ((uint64_t)(n_fn - 1) * stride >= c->p.N)
    return fail(TFHE_HIP_EINVAL, "%s: degree (n_fn - 1) * stride = %llu >= N = %u", what,
                (unsigned long long)(n_fn - 1) * stride, c->p.N);
  if (B > 0x7FFFFFFF || B * (uint64_t)n_fn > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "%s: B * n_fn too large", what);
  return 0;
}

// The single-shard host entry points: staged_run (host_common.h) on shard 0 under the engine lock.  The *_async
// entry points share async_call below.
template <class F>
int staged_call(tfhe_ctx* c, staged_in in, size_t out_bytes, std::initializer_list<copy_back> back, F&& launch) {
  std::lock_guard<std::mutex> lk(c->mu);
  shard& s = c->sh[0];
  DeviceGuard g(s.device);
  return staged_run(s, in, out_bytes, back, launch);
}

// Host -> device copy through a pinned staging ring (2 x 16 MB): the CPU fills one slot while the DMA
// engine drains the other.  Pageable sources would otherwise go through the runtime's own bounce buffer
// one synchronous piece at a time.
int upload_pinned(shard& s, void* dst, const void* src, size_t bytes) {
  const size_t slot = 16u << 20;
  void* ring[2] = {nullptr, nullptr};
  hipEvent_t done[2] = {nullptr, nullptr};
  int rc = 0;
  auto cleanup = [&]() {
    for (int i = 0; i < 2; i++) {
      if (done[i]) (void)hipEventDestroy(done[i]);
      if (ring[i]) (void)hipHostFree(ring[i]);
    }
  };
  for (int i = 0; i < 2 && !rc; i++) {
    if (hipHostMalloc(&ring[i], slot, hipHostMallocDefault) != hipSuccess) rc = fail(TFHE_HIP_ENOMEM, "pinned staging alloc");
    else if (hipEventCreateWithFlags(&done[i], hipEventDisableTiming) != hipSuccess) rc = fail(TFHE_HIP_EDEVICE, "event");
  }
  bool used[2] = {false, false};
  for (size_t off = 0, k = 0; off < bytes && !rc; off += slot, k ^= 1) {
    const size_t n = std::min(slot, bytes - off);
    if (used[k] && hipEventSynchronize(done[k]) != hipSuccess) rc = fail(TFHE_HIP_EDEVICE, "staging sync");
    if (rc) break;
    memcpy(ring[k], (const char*)src + off, n);
    if (hipMemcpyAsync((char*)dst + off, ring[k], n, hipMemcpyHostToDevice, s.stream) != hipSuccess ||
        hipEventRecord(done[k], s.stream) != hipSuccess)
      rc = fail(TFHE_HIP_EDEVICE, "staged upload failed");
    used[k] = true;
  }
  if (hipStreamSynchronize(s.stream) != hipSuccess && !rc) rc = fail(TFHE_HIP_EDEVICE, "staged upload sync");
  cleanup();
  return rc;
}

bool ordinals_distinct(const int* devices, int ndev) {
  for (int i = 0; i < ndev; i++)
    for (int j = i + 1; j < ndev; j++)
      if (devices[i] == devices[j]) return false;
  return true;
}

// Broadcast planner (tfhe_hip_bcast_plan): which replication the key load takes and the per-rank call list
// (`distinct`: ordinals_distinct of the ndev device ordinals).
//   policy "rccl": RCCL even for one device (the plumbing test); "copy": device / peer copies; NULL or "" = auto:
//   RCCL when the ordinals are distinct and librccl loads, device / peer copies otherwise (a repeated ordinal, or
//   no RCCL: hipMemcpyPeerAsync reaches every xGMI peer without it).
//   mode 2: calls[i] = rank i's ncclBroadcast inside ONE ncclGroupStart / ncclGroupEnd, root 0 (sends in place)
//   first, every rank on its own communicator member and stream; mode 1: calls[i - 1] = destination shard i of
//   copy i from shard 0; mode 0: nothing to do.  Returns the call count or a negative error.
int bcast_plan(int ndev, bool distinct, const char* policy, bool rccl_ok, int* mode, int* calls, int max_calls,
               std::string* why) {
  const bool forced = policy && strcmp(policy, "rccl") == 0;
  const bool copy = policy && strcmp(policy, "copy") == 0;
  if (policy && *policy && !forced && !copy) {
    if (why) *why = std::string("unknown broadcast policy '") + policy + "' (rccl | copy)";
    return TFHE_HIP_EINVAL;
  }
  *mode = 0;
  if (ndev < 2 && !forced) return 0;
  if (forced) {
    if (!distinct) {
      if (why) *why = "RCCL broadcast needs distinct device ordinals";
      return TFHE_HIP_EINVAL;
    }
    if (!rccl_ok) {
      if (why) *why = "RCCL forced but unavailable";
      return TFHE_HIP_EDEVICE;
    }
  }
  const bool use_rccl = forced || (!copy && distinct && rccl_ok);
  const int n = use_rccl ? ndev : ndev - 1;
  if (calls && n > max_calls) {
    if (why) *why = "call list too small";
    return TFHE_HIP_EINVAL;
  }
  for (int i = 0; calls && i < n; i++) calls[i] = use_rccl ? i : i + 1;
  *mode = use_rccl ? 2 : 1;
  return n;
}

// Broadcast `count` u64 from src (on shard 0's device) into dst[i] of every shard i >= 1, as planned above.
int broadcast(tfhe_ctx* c, const u64* src, const std::vector<u64*>& dst, size_t count) {
  const int nd = (int)c->sh.size();
  const char* env = getenv("TFHE_HIP_BCAST");
  std::vector<int> devs(nd), calls(nd);
  for (int i = 0; i < nd; i++) devs[i] = c->sh[i].device;
  const bool distinct = ordinals_distinct(devs.data(), nd);
  // librccl is only probed when the plan could use it
  const bool want = (env && strcmp(env, "rccl") == 0) || (nd > 1 && distinct && !(env && strcmp(env, "copy") == 0));
  Rccl* R = want ? &rccl() : nullptr;
  int mode = 0;
  std::string why;
  const int ncalls = bcast_plan(nd, distinct, env, R && R->ok, &mode, calls.data(), nd, &why);
  if (ncalls < 0)
    return fail(ncalls, "key broadcast: %s%s%s", why.c_str(), R && !R->ok ? ": " : "", R && !R->ok ? R->why.c_str() : "");
  if (mode == 2) {
    if (c->comms.empty()) {
      c->comms.assign(nd, nullptr);
      const ncclResult_t r = R->comm_init_all(c->comms.data(), nd, devs.data());
      if (r != ncclSuccess) {
        c->comms.clear();
        return fail(TFHE_HIP_EDEVICE, "ncclCommInitAll: %s", R->err(r));
      }
    }
    R->group_start();
    ncclResult_t r = ncclSuccess;
    for (int k = 0; k < ncalls && r == ncclSuccess; k++) {
      const int i = calls[k];
      DeviceGuard g(c->sh[i].device);
      r = R->bcast(i == 0 ? (const void*)src : (const void*)dst[i], i == 0 ? (void*)src : (void*)dst[i], count,
                   ncclUint64, 0, c->comms[i], c->sh[i].stream);
    }
    const ncclResult_t r2 = R->group_end();
    if (r != ncclSuccess || r2 != ncclSuccess)
      return fail(TFHE_HIP_EDEVICE, "ncclBroadcast: %s", R->err(r != ncclSuccess ? r : r2));
    for (int i = 0; i < nd; i++) {
      DeviceGuard g(c->sh[i].device);
      HIP_TRY(hipStreamSynchronize(c->sh[i].stream));
    }
    c->bcast_mode = 2;
    return 0;
  }
  if (mode == 0) return 0;
  for (int k = 0; k < ncalls; k++) {
    shard& s = c->sh[calls[k]];
    DeviceGuard g(s.device);
    if (s.device == c->sh[0].device)
      HIP_TRY(hipMemcpyAsync(dst[calls[k]], src, count * 8, hipMemcpyDeviceToDevice, s.stream));
    else
      HIP_TRY(hipMemcpyPeerAsync(dst[calls[k]], s.device, src, c->sh[0].device, count * 8, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
  }
  c->bcast_mode = 1;
  return 0;
}

// Convert a standard-domain BSK at `std_bsk` (on the shard's device) to the transform domain and, with_ksk, the
// KSK at s.d_ksk to byte planes.
int convert_keys(tfhe_ctx* c, shard& s, const u64* std_bsk, size_t bsk_len, bool with_ksk) {
  const size_t polys = bsk_len / c->p.N;
  DeviceGuard g(s.device);
  if (with_ksk && !c->ks_valu) {
    const int big_dim = (int)(c->p.k * c->p.N);
    if (!s.d_ks_planes)
      HIP_TRY(hipMalloc(&s.d_ks_planes, tfhe::ks_planes_bytes(big_dim, (int)c->p.ks_level, (int)c->p.n)));
    HIP_TRY(tfhe::launch_ksk_planes(s.d_ksk, big_dim, (int)c->p.ks_level, (int)c->p.n, s.d_ks_planes, s.stream));
  }
  HIP_TRY(c->eng->convert_bsk(std_bsk, s.d_bsk, polys, s.d_tw, s.stream));
  HIP_TRY(hipStreamSynchronize(s.stream));
  return 0;
}

int shard_init(tfhe_ctx* c, shard& s) {
  DeviceGuard g(s.device);
  RC_TRY(slot_streams(s));
  HIP_TRY(hipDeviceGetAttribute(&s.cus, hipDeviceAttributeMultiprocessorCount, s.device));
  std::vector<u64> tw(c->eng->table_words);  // the back end's twiddle / twist tables
  if (!c->eng->make_tables(tw.data()))
    return fail(TFHE_HIP_EUNSUPPORTED, "FFT64: compile-time twist constants differ from the host tables");
  HIP_TRY(hipMalloc(&s.d_tw, tw.size() * 8));
  HIP_TRY(hipMemcpy(s.d_tw, tw.data(), tw.size() * 8, hipMemcpyHostToDevice));
  return 0;
}

void shard_free(shard& s) {
  DeviceGuard g(s.device);
  slot_close(s, {s.d_bsk, s.d_tw_mb, s.d_ksk, s.d_ks_planes, s.d_ks_dig, s.d_tw, s.d_ms_zeros, s.d_big, s.d_acc, s.d_expand, s.d_oprf,
                 s.d_lin, s.d_lin_meta});
  for (int w = 0; w < TIMING_SLOTS; w++)
    for (auto e : s.ev[w]) (void)hipEventDestroy(e);
  for (auto e : s.ev_pool) (void)hipEventDestroy(e);
  for (int i = 0; i < 2; i++) {
    if (s.h_lin_meta[i]) (void)hipHostFree(s.h_lin_meta[i]);
    if (s.lin_meta_done[i]) (void)hipEventDestroy(s.lin_meta_done[i]);
  }
}

// Run fn(shard index, lo, hi) for contiguous slices of [0, B) on every shard concurrently (one host
// thread per shard beyond the first); the first error (with its message) is returned on this thread.
template <class F>
int for_each_slice(tfhe_ctx* c, size_t B, F&& fn) {
  const size_t nd = c->sh.size();
  std::vector<int> rc(nd, 0);
  std::vector<std::string> msg(nd);
  auto run = [&](size_t i) {
    const size_t lo = B * i / nd, hi = B * (i + 1) / nd;
    if (lo == hi) return;
    DeviceGuard g(c->sh[i].device);
    rc[i] = fn(i, lo, hi);
    if (rc[i]) msg[i] = g_err;
  };
  if (nd == 1) {
    run(0);
    return rc[0];
  }
  std::vector<std::thread> th;
  for (size_t i = 1; i < nd; i++) th.emplace_back(run, i);
  run(0);
  for (auto& t : th) t.join();
  for (size_t i = 0; i < nd; i++)
    if (rc[i]) {
      g_err = "shard " + std::to_string(i) + " (device " + std::to_string(c->sh[i].device) + "): " + msg[i];
      return rc[i];
    }
  return 0;
}

// argument checks shared by the PBS entry points (`what`: the message prefix); B == 0 passes
int pbs_check(const tfhe_ctx* c, const char* what, const void* in, size_t B, const void* luts, size_t n_lut,
              const pbs_kind& kd, const void* out) {
  const many_args* m = kd.m;
  if (!c) return fail(TFHE_HIP_EINVAL, "%s: null ctx", what);
  if (kd.rotation_only ? !c->bsk : !c->keys)
    return fail(TFHE_HIP_ENOKEYS, "%s: %s not loaded", what, kd.rotation_only ? "bootstrapping key" : "keys");
  if (m) RC_TRY(check_many(c, what, B, m->n_fn, m->stride));
  if (B == 0) return 0;
  if (!in || !luts || !n_lut || !out) return fail(TFHE_HIP_EINVAL, "%s: null buffer or n_lut == 0", what);
  if (B > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "%s: batch too large", what);
  return 0;
}

// The shard that runs an *_async call: the first one whose device holds the input (caller holds c->mu).
int shard_of_input(tfhe_ctx* c, const char* what, const void* d_in, size_t* si) {
  *si = 0;
  if (c->sh.size() < 2) return 0;
  hipPointerAttribute_t a;
  HIP_TRY(hipPointerGetAttributes(&a, d_in));
  for (size_t i = 0; i < c->sh.size(); i++)
    if (c->sh[i].device == a.device) {
      *si = i;
      return 0;
    }
  return fail(TFHE_HIP_EINVAL, "%s_async: input on device %d, no shard there", what, a.device);
}

// The *_async entry points (device buffers, checked by the caller): under the engine lock, work(s, st) on the shard
// whose device holds `d_anchor` and on the caller's stream.  uses_ws: the work touches the shard's workspaces or
// keys, so it is ordered after their previous user and recorded as the latest; without it no event is taken.
template <class F>
int async_call(tfhe_ctx* c, const char* what, const void* d_anchor, void* stream, bool uses_ws, F&& work) {
  std::lock_guard<std::mutex> lk(c->mu);
  size_t si = 0;
  RC_TRY(shard_of_input(c, what, d_anchor, &si));
  shard& s = c->sh[si];
  DeviceGuard g(s.device);
  hipStream_t st = resolve_stream(stream, s.stream);
  if (!uses_ws) return work(s, st);
  RC_TRY(ws_begin(s, st));
  RC_TRY(work(s, st));
  return ws_end(s, st);
}

int host_lut_index_check(const char* what, const u32* lut_index, size_t B, size_t n_lut) {
  if (lut_index)
    for (size_t q = 0; q < B; q++)
      if (lut_index[q] >= n_lut)
        return fail(TFHE_HIP_EINVAL, "%s: lut_index[%zu] = %u >= n_lut %zu", what, q, lut_index[q], n_lut);
  return 0;
}

// a PBS entry point's work on one shard (pbs_device, or the rotation alone)
int pbs_kind_device(tfhe_ctx* c, shard& s, const u64* d_in, size_t B, const u64* d_luts, size_t n_lut,
                    const u32* d_idx, const pbs_kind& kd, u64* d_out, hipStream_t st) {
  if (kd.rotation_only) return bootstrap_device(c, s, d_in, B, d_luts, n_lut, d_idx, d_out, st);
  return pbs_device(c, s, d_in, B, d_luts, n_lut, d_idx, kd.m, d_out, st);
}

// tfhe_hip_pbs_async / tfhe_hip_pbs_many_async / tfhe_hip_bootstrap_async: device buffers, on the shard whose
// device holds the input
int pbs_async_call(tfhe_ctx* c, const char* what, const u64* d_in, size_t B, const u64* d_luts, size_t n_lut,
                   const u32* d_idx, const pbs_kind& kd, u64* d_out, void* stream) {
  RC_TRY(pbs_check(c, what, d_in, B, d_luts, n_lut, kd, d_out));
  if (B == 0) return 0;
  return async_call(c, what, d_in, stream, true, [&](shard& s, hipStream_t st) {
    return pbs_kind_device(c, s, d_in, B, d_luts, n_lut, d_idx, kd, d_out, st);
  });
}

// tfhe_hip_pbs / tfhe_hip_pbs_many / tfhe_hip_bootstrap: host buffers, sliced over the shards
int pbs_host_call(tfhe_ctx* c, const char* what, const u64* lwe_in, size_t B, const u64* luts, size_t n_lut,
                  const u32* lut_index, const pbs_kind& kd, u64* lwe_out) {
  RC_TRY(pbs_check(c, what, lwe_in, B, luts, n_lut, kd, lwe_out));
  if (B == 0) return 0;
  RC_TRY(host_lut_index_check(what, lut_index, B, n_lut));
  std::lock_guard<std::mutex> lk(c->mu);
  const size_t io = io_dim(c->p) + 1;
  const size_t dim = kd.rotation_only ? (size_t)c->p.n + 1 : io;
  const size_t out_dim = kd.rotation_only ? (size_t)c->p.k * c->p.N + 1 : (kd.m ? kd.m->n_fn : 1) * io;
  return for_each_slice(c, B, [&](size_t i, size_t lo, size_t hi) -> int {
    const size_t b = hi - lo;
    return staged_run(c->sh[i],
                      {{lwe_in + lo * dim, b * dim * 8}, {luts, n_lut * c->p.N * 8},
                       {lut_index ? lut_index + lo : nullptr, lut_index ? b * 4 : 0}},
                      b * out_dim * 8, {{lwe_out + lo * out_dim, 3, b * out_dim * 8}},
                      [&](shard& s, std::vector<void*>& d) {
                        return pbs_kind_device(c, s, (const u64*)d[0], b, (const u64*)d[1], n_lut, (const u32*)d[2],
                                               kd, (u64*)d[3], s.stream);
                      });
  });
}

// tfhe_hip_decompress*: every check that precedes device work.  The list checks need no ctx, so they come first.
int decompress_check(const tfhe_ctx* c, const tfhe_pks_params* pp, const void* packed, size_t packed_words,
                     size_t count, const void* luts, size_t n_lut, const void* out) {
  RC_TRY(tfhe_hip_pks_list_check(pp, packed_words, count, "decompress"));
  if (!c) return fail(TFHE_HIP_EINVAL, "decompress: null ctx");
  if ((uint64_t)pp->out_k * pp->out_N != c->p.n)
    return fail(TFHE_HIP_EINVAL, "decompress: out_k * out_N = %llu, the ctx rotates ciphertexts of dimension n = %u",
                (unsigned long long)pp->out_k * pp->out_N, c->p.n);
  if (!c->bsk) return fail(TFHE_HIP_ENOKEYS, "decompress: bootstrapping key not loaded");
  if (count == 0) return 0;
  if (!packed || !luts || !n_lut || !out) return fail(TFHE_HIP_EINVAL, "decompress: null buffer or n_lut == 0");
  return 0;
}

// Decompression on device buffers (caller as pbs_device): unpack / extract into the shard's d_big workspace
// (slot 3), then the rotation (slot 0).
int decompress_device(tfhe_ctx* c, shard& s, const tfhe_pks_params& pp, const u64* d_packed, size_t count,
                      const u64* d_luts, size_t n_lut, const u32* d_idx, u64* d_out, hipStream_t st) {
  RC_TRY(ws_grow(s, (void**)&s.d_big, &s.big_cap, count * ((size_t)c->p.n + 1) * sizeof(u64)));
  timed_begin(c, s, 3, st);
  HIP_TRY(tfhe::launch_unpack_extract(d_packed, count, (int)pp.out_k, (int)pp.out_N, (int)pp.lwe_per_glwe,
                                      (int)pp.storage_log, s.d_big, st));
  timed_end(c, s, 3, st);
  return bootstrap_device(c, s, s.d_big, count, d_luts, n_lut, d_idx, d_out, st);
}

constexpr uint32_t EXPAND_MIN_DIM = 8, EXPAND_MAX_DIM = 4096;  // expand.hip: one mask polynomial in 32 KB of LDS (+ 64 bytes)

bool expand_dim_ok(uint32_t d) { return d >= EXPAND_MIN_DIM && d <= EXPAND_MAX_DIM && (d & (d - 1)) == 0; }

// tfhe_hip_expand_*: the checks on the list itself, which need no ctx
int compact_list_check(const char* what, size_t list_words, uint32_t lwe_dim, size_t count, uint32_t rep, size_t rows) {
  if (lwe_dim > EXPAND_MAX_DIM && (lwe_dim & (lwe_dim - 1)) == 0)
    return fail(TFHE_HIP_EUNSUPPORTED, "%s: lwe_dim = %u, the expansion kernel covers lwe_dim <= %u", what, lwe_dim,
                EXPAND_MAX_DIM);
  if (!expand_dim_ok(lwe_dim))
    return fail(TFHE_HIP_EINVAL, "%s: lwe_dim = %u is not a power of two in %u .. %u", what, lwe_dim, EXPAND_MIN_DIM,
                EXPAND_MAX_DIM);
  if (count > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "%s: too many ciphertexts", what);
  const size_t want = tfhe_hip_compact_list_words(lwe_dim, count);
  if (list_words != want)
    return fail(TFHE_HIP_EINVAL, "%s: list_words = %zu, %zu ciphertexts of dimension %u take %zu", what, list_words, count,
                lwe_dim, want);
  if (rep == 0 || rep > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "%s: rep = %u", what, rep);
  if (rows > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "%s: rows = %zu, too many rows for one call", what, rows);
  if (rows > count * (size_t)rep)
    return fail(TFHE_HIP_EINVAL, "%s: rows = %zu, the list gives %zu x %u", what, rows, count, rep);
  return 0;
}

// tfhe_hip_expand_compact*: every check that precedes device work
int expand_check(const tfhe_ctx* c, const void* list, size_t list_words, uint32_t lwe_dim, size_t count, uint32_t rep,
                 size_t rows, const void* out) {
  RC_TRY(compact_list_check("expand_compact", list_words, lwe_dim, count, rep, rows));
  if (!c) return fail(TFHE_HIP_EINVAL, "expand_compact: null ctx");
  if (rows && (!list || !out)) return fail(TFHE_HIP_EINVAL, "expand_compact: null buffer");
  return 0;
}

// tfhe_hip_expand_cast*: the list's dimension is the ctx's io_dim, so the ctx comes first here
int expand_cast_check(const tfhe_ctx* c, const void* list, size_t list_words, size_t count, uint32_t rep, size_t rows,
                      const void* luts, size_t n_lut, const void* out) {
  if (!c) return fail(TFHE_HIP_EINVAL, "expand_cast: null ctx");
  const uint32_t dim = io_dim(c->p);
  if (!expand_dim_ok(dim))
    return fail(TFHE_HIP_EINVAL, "expand_cast: io_dim = %u is not a power of two in %u .. %u", dim, EXPAND_MIN_DIM,
                EXPAND_MAX_DIM);
  RC_TRY(compact_list_check("expand_cast", list_words, dim, count, rep, rows));
  if (!c->keys) return fail(TFHE_HIP_ENOKEYS, "expand_cast: keys not loaded");
  if (!n_lut) return fail(TFHE_HIP_EINVAL, "expand_cast: n_lut == 0");
  if (rows && (!list || !luts || !out)) return fail(TFHE_HIP_EINVAL, "expand_cast: null buffer");
  return 0;
}

// Expansion on device buffers (caller as pbs_device), timed in slot 3.
int expand_device(tfhe_ctx* c, shard& s, const u64* d_list, size_t count, uint32_t lwe_dim, uint32_t rep, size_t rows,
                  u64* d_out, hipStream_t st) {
  timed_begin(c, s, 3, st);
  HIP_TRY(tfhe::launch_expand_compact(d_list, count, (int)lwe_dim, (int)rep, rows, d_out, st));
  timed_end(c, s, 3, st);
  return 0;
}

// Expansion into the shard's d_expand workspace (d_big is pbs_device's own: the keyswitch output in order 1, the
// rotation output in order 0), then the full PBS unchanged.
int expand_cast_device(tfhe_ctx* c, shard& s, const u64* d_list, size_t count, uint32_t rep, size_t rows,
                       const u64* d_luts, size_t n_lut, const u32* d_idx, u64* d_out, hipStream_t st) {
  const uint32_t dim = io_dim(c->p);
  RC_TRY(ws_grow(s, (void**)&s.d_expand, &s.expand_cap, rows * ((size_t)dim + 1) * sizeof(u64)));
  RC_TRY(expand_device(c, s, d_list, count, dim, rep, rows, s.d_expand, st));
  return pbs_device(c, s, s.d_expand, rows, d_luts, n_lut, d_idx, nullptr, d_out, st);
}

// tfhe_hip_oprf*: every check that precedes device work
int oprf_check(const tfhe_ctx* c, const void* seeds, size_t rows, const void* luts, const void* post_adds, size_t n_lut,
               const void* out) {
  if (!c) return fail(TFHE_HIP_EINVAL, "oprf: null ctx");
  if (!c->bsk) return fail(TFHE_HIP_ENOKEYS, "oprf: bootstrapping key not loaded");
  if (c->p.order == 0 && !c->keys)
    return fail(TFHE_HIP_ENOKEYS, "oprf: a PBS -> KS parameter set keyswitches the result: keyswitching key not loaded");
  if (rows > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "oprf: rows = %zu, too many rows for one call", rows);
  if (!n_lut) return fail(TFHE_HIP_EINVAL, "oprf: n_lut == 0");
  if (rows && (!seeds || !luts || !post_adds || !out)) return fail(TFHE_HIP_EINVAL, "oprf: null buffer");
  return 0;
}

// The seeded masks (slot 3)
int csprng_device(tfhe_ctx* c, shard& s, const u64* d_seeds, size_t rows, u64 first_word, u32 dim, size_t row_stride,
                  bool zero_body, u64* d_out, hipStream_t st) {
  timed_begin(c, s, 3, st);
  HIP_TRY(tfhe::launch_csprng_rows(d_seeds, rows, first_word, dim, row_stride, zero_body, d_out, st));
  timed_end(c, s, 3, st);
  return 0;
}

// OPRF on device buffers (caller as pbs_device): the masks of the rows' seeds with body 0 into the shard's d_oprf
// workspace (d_big is pbs_device's own), the rotation alone (order 1) or the full PBS (order 0), then the post-add.
int oprf_device(tfhe_ctx* c, shard& s, const u64* d_seeds, size_t rows, const u64* d_luts, const u64* d_post,
                size_t n_lut, const u32* d_idx, u64* d_out, hipStream_t st) {
  const size_t small = (size_t)c->p.n + 1;
  RC_TRY(ws_grow(s, (void**)&s.d_oprf, &s.oprf_cap, rows * small * sizeof(u64)));
  RC_TRY(csprng_device(c, s, d_seeds, rows, 0, c->p.n, small, true, s.d_oprf, st));
  if (c->p.order == 1) RC_TRY(bootstrap_device(c, s, s.d_oprf, rows, d_luts, n_lut, d_idx, d_out, st));
  else RC_TRY(pbs_device(c, s, s.d_oprf, rows, d_luts, n_lut, d_idx, nullptr, d_out, st));
  HIP_TRY(tfhe::launch_body_add(d_out, rows, (size_t)io_dim(c->p) + 1, d_post, n_lut, d_idx, st));
  return 0;
}

// the term description of the tfhe_hip_lwe_lincomb* entry points: host arrays (include/tfhe_hip.h)
struct lin_desc {
  const u32* row_start;  // rows + 1 entries
  const u32* term_buf;   // null: every term reads buffer 0 (the host form)
  const u32* term_row;
  const u64* term_coef;
  const u64* bias;  // null: no bias
};

// tfhe_hip_lwe_lincomb*: every check of the description that precedes device work; rows == 0 passes.  After it each
// term names an existing row of an existing buffer.
int lincomb_check(const char* what, uint32_t dim, const size_t* buf_rows, size_t n_buf, const lin_desc& L, size_t rows) {
  if (dim == 0) return fail(TFHE_HIP_EINVAL, "%s: dim == 0", what);
  if (rows > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "%s: rows = %zu, too many rows for one call", what, rows);
  if (rows == 0) return 0;
  if (!L.row_start || (n_buf && !buf_rows)) return fail(TFHE_HIP_EINVAL, "%s: null buffer", what);
  if (L.row_start[0] != 0) return fail(TFHE_HIP_EINVAL, "%s: row_start[0] = %u, must be 0", what, L.row_start[0]);
  for (size_t r = 0; r < rows; r++)
    if (L.row_start[r + 1] < L.row_start[r])
      return fail(TFHE_HIP_EINVAL, "%s: row_start[%zu] = %u < row_start[%zu] = %u", what, r + 1, L.row_start[r + 1], r,
                  L.row_start[r]);
  const size_t T = L.row_start[rows];
  if (T && (!L.term_row || !L.term_coef)) return fail(TFHE_HIP_EINVAL, "%s: null buffer", what);
  for (size_t b = 0; b < n_buf; b++)
    if (buf_rows[b] > (1ull << 60) / dim) return fail(TFHE_HIP_EINVAL, "%s: buf_rows[%zu] = %zu too large", what, b, buf_rows[b]);
  for (size_t t = 0; t < T; t++) {
    const size_t b = L.term_buf ? L.term_buf[t] : 0;
    if (b >= n_buf) return fail(TFHE_HIP_EINVAL, "%s: term_buf[%zu] = %zu >= n_buf = %zu", what, t, b, n_buf);
    if (L.term_row[t] >= buf_rows[b])
      return fail(TFHE_HIP_EINVAL, "%s: term_row[%zu] = %u >= the %zu rows of buffer %zu", what, t, L.term_row[t],
                  buf_rows[b], b);
  }
  return 0;
}

// device pointers of tfhe_hip_lwe_lincomb_async / tfhe_hip_lincomb_pbs_async: no null source, and (d_out given) no
// source range that the output range rows x dim touches
int lincomb_ptr_check(const char* what, uint32_t dim, const uint64_t* const* d_bufs, const size_t* buf_rows, size_t n_buf,
                      size_t rows, const uint64_t* d_out) {
  if (n_buf && !d_bufs) return fail(TFHE_HIP_EINVAL, "%s: null buffer", what);
  const uintptr_t o_lo = (uintptr_t)d_out, o_hi = o_lo + rows * (size_t)dim * 8;
  for (size_t b = 0; b < n_buf; b++) {
    if (!buf_rows[b]) continue;
    if (!d_bufs[b]) return fail(TFHE_HIP_EINVAL, "%s: source buffer %zu is null", what, b);
    const uintptr_t lo = (uintptr_t)d_bufs[b], hi = lo + buf_rows[b] * (size_t)dim * 8;
    if (d_out && o_lo < hi && lo < o_hi) return fail(TFHE_HIP_EINVAL, "%s: the output overlaps source buffer %zu", what, b);
  }
  return 0;
}

// Resolve a checked description into the kernel's arrays.  Terms (address, coefficient), row_start and bias are packed
// into one pinned slot of the shard and go to d_lin_meta in one copy on `st`; the slot is refilled only after the
// event behind that copy (the caller's ws_begin / ws_end order d_lin_meta itself across streams).
int lincomb_stage(shard& s, uint32_t dim, const uint64_t* const* d_bufs, const lin_desc& L, size_t rows, hipStream_t st,
                  const tfhe::lin_term** d_terms, const u32** d_row_start, const u64** d_bias) {
  const size_t T = L.row_start[rows];
  const size_t rs_off = T * sizeof(tfhe::lin_term);
  const size_t bias_off = (rs_off + (rows + 1) * sizeof(u32) + 15) & ~(size_t)15;
  const size_t total = bias_off + (L.bias ? rows * sizeof(u64) : 0);
  RC_TRY(ws_grow(s, &s.d_lin_meta, &s.lin_meta_cap, total));
  const int k = s.lin_meta_next;
  s.lin_meta_next ^= 1;
  if (!s.lin_meta_done[k]) HIP_TRY(hipEventCreateWithFlags(&s.lin_meta_done[k], hipEventDisableTiming));
  if (s.lin_meta_used[k]) HIP_TRY(hipEventSynchronize(s.lin_meta_done[k]));
  if (s.h_lin_meta_cap[k] < total) {
    if (s.h_lin_meta[k]) (void)hipHostFree(s.h_lin_meta[k]);
    s.h_lin_meta[k] = nullptr;
    s.h_lin_meta_cap[k] = 0;
    HIP_TRY(hipHostMalloc(&s.h_lin_meta[k], total, hipHostMallocDefault));
    s.h_lin_meta_cap[k] = total;
  }
  char* h = (char*)s.h_lin_meta[k];
  tfhe::lin_term* ht = (tfhe::lin_term*)h;
  for (size_t t = 0; t < T; t++) {
    ht[t].src = d_bufs[L.term_buf ? L.term_buf[t] : 0] + (size_t)L.term_row[t] * dim;
    ht[t].coef = L.term_coef[t];
  }
  memcpy(h + rs_off, L.row_start, (rows + 1) * sizeof(u32));
  if (L.bias) memcpy(h + bias_off, L.bias, rows * sizeof(u64));
  HIP_TRY(hipMemcpyAsync(s.d_lin_meta, h, total, hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(s.lin_meta_done[k], st));
  s.lin_meta_used[k] = true;
  *d_terms = (const tfhe::lin_term*)s.d_lin_meta;
  *d_row_start = (const u32*)((char*)s.d_lin_meta + rs_off);
  *d_bias = L.bias ? (const u64*)((char*)s.d_lin_meta + bias_off) : nullptr;
  return 0;
}

// The linear combinations on device buffers (caller as pbs_device, description and pointers checked), timed in slot 3.
int lincomb_device(tfhe_ctx* c, shard& s, uint32_t dim, const uint64_t* const* d_bufs, const lin_desc& L, size_t rows,
                   u64* d_out, hipStream_t st) {
  const tfhe::lin_term* d_terms = nullptr;
  const u32* d_row_start = nullptr;
  const u64* d_bias = nullptr;
  RC_TRY(lincomb_stage(s, dim, d_bufs, L, rows, st, &d_terms, &d_row_start, &d_bias));
  timed_begin(c, s, 3, st);
  HIP_TRY(tfhe::launch_lincomb(d_terms, d_row_start, d_bias, rows, dim, d_out, st));
  timed_end(c, s, 3, st);
  return 0;
}

}  // namespace


// error slot shared with pks_api.cpp / sns_api.cpp
int tfhe_hip_set_error(int code, const char* msg) {
  g_err = msg;
  return code;
}

extern "C" {

const char* tfhe_hip_last_error(void) { return g_err.c_str(); }

int tfhe_hip_params_preset(int preset, tfhe_params* o) {
  if (!o) return fail(TFHE_HIP_EINVAL, "null params");
  memset(o, 0, sizeof(*o));
  for (auto& r : PRESETS)
    if (r.id == preset) {
      *o = r.p;
      return 0;
    }
  return fail(TFHE_HIP_EINVAL, "unknown preset %d", preset);
}

size_t tfhe_hip_bsk_len(const tfhe_params* p) { return p ? tfhe::client::bsk_len(*p) : 0; }
size_t tfhe_hip_ksk_len(const tfhe_params* p) { return p ? tfhe::client::ksk_len(*p) : 0; }
uint32_t tfhe_hip_io_dim(const tfhe_params* p) { return p ? io_dim(*p) : 0; }

int tfhe_hip_rng_key_entropy(tfhe_rng_key* out) {
  if (!out) return fail(TFHE_HIP_EINVAL, "rng_key_entropy: null out");
  if (!tfhe::client::rng_key_entropy(out)) return fail(TFHE_HIP_EDEVICE, "rng_key_entropy: getrandom failed");
  return 0;
}

int tfhe_hip_rng_key_from_seed(uint64_t seed, tfhe_rng_key* out) {
  if (!out) return fail(TFHE_HIP_EINVAL, "rng_key_from_seed: null out");
  *out = tfhe::client::rng_key_from_seed(seed);
  return 0;
}

int tfhe_hip_keygen_k(const tfhe_params* p, const tfhe_rng_key* rk, uint64_t* lwe_key, uint64_t* glwe_key,
                      uint64_t* bsk, uint64_t* ksk) {
  if (!params_valid(p) || !rk || !lwe_key || !glwe_key) return fail(TFHE_HIP_EINVAL, "keygen: bad arguments");
  tfhe::client::keygen(*p, *rk, lwe_key, glwe_key, bsk, ksk);
  return 0;
}

int tfhe_hip_keygen(const tfhe_params* p, uint64_t seed, uint64_t* lwe_key, uint64_t* glwe_key, uint64_t* bsk,
                    uint64_t* ksk) {
  const tfhe_rng_key rk = tfhe::client::rng_key_from_seed(seed);
  return tfhe_hip_keygen_k(p, &rk, lwe_key, glwe_key, bsk, ksk);
}

int tfhe_hip_server_keygen_k(const tfhe_params* p, const tfhe_rng_key* rk, const uint64_t* lwe_key,
                             const uint64_t* glwe_key, uint64_t* bsk, uint64_t* ksk) {
  if (!params_valid(p) || !rk || !lwe_key || !glwe_key) return fail(TFHE_HIP_EINVAL, "server_keygen: bad arguments");
  RC_TRY(check_binary(lwe_key, p->n, "server_keygen: lwe_key"));
  RC_TRY(check_binary(glwe_key, (size_t)p->k * p->N, "server_keygen: glwe_key"));
  tfhe::client::server_keygen(*p, *rk, lwe_key, glwe_key, bsk, ksk);
  return 0;
}

int tfhe_hip_server_keygen(const tfhe_params* p, uint64_t seed, const uint64_t* lwe_key, const uint64_t* glwe_key,
                           uint64_t* bsk, uint64_t* ksk) {
  const tfhe_rng_key rk = tfhe::client::rng_key_from_seed(seed);
  return tfhe_hip_server_keygen_k(p, &rk, lwe_key, glwe_key, bsk, ksk);
}

// the multi-bit scope (include/tfhe_hip.h): FFT64, k = 1, N = 2048, PBS gadget 2^23 x 1
static bool mb_scope(const tfhe_params* p) {
  return p->transform == TFHE_HIP_TRANSFORM_FFT64 && p->k == 1 && p->N == 2048 && p->pbs_base_log == 23 &&
         p->pbs_level == 1;
}

// the grouping factor of a multi-bit key: 2, 3 or 4 (include/tfhe_hip.h)
static bool grouping_valid(uint32_t g) { return g >= 2 && g <= 4; }

// the refusals of every parameter-level multi-bit call (key generation, seeded key generation, host decompression)
static int mb_params_check(const char* what, const tfhe_params* p, uint32_t g) {
  if (!grouping_valid(g)) return fail(TFHE_HIP_EINVAL, "%s: grouping factor %u, expected 2, 3 or 4", what, g);
  if (p->n % g) return fail(TFHE_HIP_EINVAL, "%s: n = %u is not divisible by the grouping factor %u", what, p->n, g);
  if (!mb_scope(p))
    return fail(TFHE_HIP_EUNSUPPORTED, "%s: multi-bit keys cover FFT64, k = 1, N = 2048, PBS 23x1; got transform %u "
                                       "k=%u N=%u pbs %ux%u", what, p->transform, p->k, p->N, p->pbs_base_log,
                p->pbs_level);
  return 0;
}

size_t tfhe_hip_mb_bsk_len(const tfhe_params* p, uint32_t g) {
  return params_valid(p) && grouping_valid(g) && p->n % g == 0 ? tfhe::client::mb_bsk_len(*p, g) : 0;
}

int tfhe_hip_mb_server_keygen_k(const tfhe_params* p, uint32_t g, const tfhe_rng_key* rk, const uint64_t* lwe_key,
                                const uint64_t* glwe_key, uint64_t* bsk_mb, uint64_t* ksk) {
  if (!params_valid(p) || !rk || !lwe_key || !glwe_key || !bsk_mb)
    return fail(TFHE_HIP_EINVAL, "mb_server_keygen: bad arguments");
  RC_TRY(mb_params_check("mb_server_keygen", p, g));
  RC_TRY(check_binary(lwe_key, p->n, "mb_server_keygen: lwe_key"));
  RC_TRY(check_binary(glwe_key, (size_t)p->k * p->N, "mb_server_keygen: glwe_key"));
  tfhe::client::mb_server_keygen(*p, g, *rk, lwe_key, glwe_key, bsk_mb, ksk);
  return 0;
}

int tfhe_hip_mb_server_keygen(const tfhe_params* p, uint32_t g, uint64_t seed, const uint64_t* lwe_key,
                              const uint64_t* glwe_key, uint64_t* bsk_mb, uint64_t* ksk) {
  const tfhe_rng_key rk = tfhe::client::rng_key_from_seed(seed);
  return tfhe_hip_mb_server_keygen_k(p, g, &rk, lwe_key, glwe_key, bsk_mb, ksk);
}

int tfhe_hip_ms_zeros_keygen_k(const tfhe_params* p, const tfhe_rng_key* rk, const uint64_t* lwe_key, uint32_t count,
                               uint64_t* zeros) {
  if (!params_valid(p) || !rk || !lwe_key || (count && !zeros))
    return fail(TFHE_HIP_EINVAL, "ms_zeros_keygen: bad arguments");
  tfhe::client::ms_zeros_keygen(*p, *rk, lwe_key, count, zeros);
  return 0;
}

// ---- compressed (seeded) server keys (seeded.cpp)
static bool native_torus(const tfhe_params* p) { return params_valid(p) && p->transform == TFHE_HIP_TRANSFORM_FFT64; }

int tfhe_hip_aes128_block(const uint8_t key[16], const uint8_t in[16], uint8_t out[16]) {
  if (!key || !in || !out) return fail(TFHE_HIP_EINVAL, "aes128_block: null argument");
  tfhe::seeded::aes128_block(key, in, out);
  return 0;
}

int tfhe_hip_csprng_words(const uint64_t seed[2], uint64_t first_word, size_t count, uint64_t* out) {
  if (!seed || (count && !out)) return fail(TFHE_HIP_EINVAL, "csprng_words: null argument");
  tfhe::seeded::csprng_words(seed, first_word, count, out);
  return 0;
}

int tfhe_hip_seeded_server_keygen_k(const tfhe_params* p, const tfhe_rng_key* rk, const uint64_t bsk_seed[2],
                                    const uint64_t ksk_seed[2], const uint64_t* lwe_key, const uint64_t* glwe_key,
                                    uint64_t* bsk_bodies, uint64_t* ksk_bodies) {
  if (!native_torus(p) || !rk || !lwe_key || !glwe_key || (bsk_bodies && !bsk_seed) || (ksk_bodies && !ksk_seed))
    return fail(TFHE_HIP_EINVAL, "seeded_server_keygen: bad arguments (FFT64 presets only)");
  RC_TRY(check_binary(lwe_key, p->n, "seeded_server_keygen: lwe_key"));
  RC_TRY(check_binary(glwe_key, (size_t)p->k * p->N, "seeded_server_keygen: glwe_key"));
  tfhe::seeded::seeded_server_keygen(*p, *rk, bsk_seed, ksk_seed, lwe_key, glwe_key, bsk_bodies, ksk_bodies);
  return 0;
}

int tfhe_hip_seeded_lwe_list_k(uint32_t dim, uint32_t count, const uint64_t* key, int32_t noise_log2,
                               const tfhe_rng_key* rk, uint64_t stream0, const uint64_t seed[2], const uint64_t* msgs,
                               uint64_t* bodies) {
  if (!dim || !key || !rk || !seed || (count && !bodies)) return fail(TFHE_HIP_EINVAL, "seeded_lwe_list: bad arguments");
  RC_TRY(check_binary(key, dim, "seeded_lwe_list: key"));
  tfhe::seeded::seeded_lwe_list(dim, count, key, noise_log2, *rk, stream0, seed, msgs, bodies);
  return 0;
}

int tfhe_hip_decompress_bsk(const tfhe_params* p, const uint64_t seed[2], const uint64_t* bodies, uint64_t* bsk) {
  if (!native_torus(p) || !seed || !bodies || !bsk)
    return fail(TFHE_HIP_EINVAL, "decompress_bsk: bad arguments (FFT64 presets only)");
  tfhe::seeded::decompress_bsk(*p, seed, bodies, bsk);
  return 0;
}

int tfhe_hip_decompress_ksk(const tfhe_params* p, const uint64_t seed[2], const uint64_t* bodies, uint64_t* ksk) {
  if (!native_torus(p) || !seed || !bodies || !ksk)
    return fail(TFHE_HIP_EINVAL, "decompress_ksk: bad arguments (FFT64 presets only)");
  tfhe::seeded::decompress_ksk(*p, seed, bodies, ksk);
  return 0;
}

int tfhe_hip_decompress_lwe_list(uint32_t dim, uint32_t count, const uint64_t seed[2], const uint64_t* bodies,
                                 uint64_t* out) {
  if (!dim || !seed || (count && (!bodies || !out))) return fail(TFHE_HIP_EINVAL, "decompress_lwe_list: bad arguments");
  tfhe::seeded::decompress_lwe_list(dim, count, seed, bodies, out);
  return 0;
}

size_t tfhe_hip_seeded_mb_bodies_len(const tfhe_params* p, uint32_t g) {
  return params_valid(p) && grouping_valid(g) && p->n % g == 0 ? tfhe::client::bsk_bodies_len(*p, g) : 0;
}

int tfhe_hip_seeded_mb_server_keygen_k(const tfhe_params* p, uint32_t g, const tfhe_rng_key* rk,
                                       const uint64_t bsk_seed[2], const uint64_t* lwe_key, const uint64_t* glwe_key,
                                       uint64_t* bsk_bodies) {
  if (!params_valid(p) || !rk || !bsk_seed || !lwe_key || !glwe_key || !bsk_bodies)
    return fail(TFHE_HIP_EINVAL, "seeded_mb_server_keygen: bad arguments");
  RC_TRY(mb_params_check("seeded_mb_server_keygen", p, g));
  RC_TRY(check_binary(lwe_key, p->n, "seeded_mb_server_keygen: lwe_key"));
  RC_TRY(check_binary(glwe_key, (size_t)p->k * p->N, "seeded_mb_server_keygen: glwe_key"));
  tfhe::seeded::seeded_mb_server_keygen(*p, g, *rk, bsk_seed, lwe_key, glwe_key, bsk_bodies);
  return 0;
}

int tfhe_hip_decompress_bsk_mb(const tfhe_params* p, uint32_t g, const uint64_t seed[2], const uint64_t* bodies,
                               uint64_t* bsk_mb) {
  if (!params_valid(p) || !seed || !bodies || !bsk_mb) return fail(TFHE_HIP_EINVAL, "decompress_bsk_mb: bad arguments");
  RC_TRY(mb_params_check("decompress_bsk_mb", p, g));
  tfhe::seeded::decompress_bsk_mb(*p, g, seed, bodies, bsk_mb);
  return 0;
}

int tfhe_hip_ms_zeros_keygen(const tfhe_params* p, uint64_t seed, const uint64_t* lwe_key, uint32_t count,
                             uint64_t* zeros) {
  const tfhe_rng_key rk = tfhe::client::rng_key_from_seed(seed);
  return tfhe_hip_ms_zeros_keygen_k(p, &rk, lwe_key, count, zeros);
}

int tfhe_hip_lwe_encrypt_k(uint32_t dim, const uint64_t* key, int32_t noise_log2, const tfhe_rng_key* rk,
                           uint64_t stream0, const uint64_t* msgs, size_t count, uint64_t* out) {
  if (!dim || !key || !rk || (count && (!msgs || !out))) return fail(TFHE_HIP_EINVAL, "lwe_encrypt: bad arguments");
  if (noise_log2 >= 0 || noise_log2 < -63) return fail(TFHE_HIP_EINVAL, "lwe_encrypt: noise_log2 out of range");
  tfhe::client::lwe_encrypt(dim, key, noise_log2, *rk, stream0, msgs, count, out);
  return 0;
}

int tfhe_hip_lwe_encrypt(uint32_t dim, const uint64_t* key, int32_t noise_log2, uint64_t seed, uint64_t stream0,
                         const uint64_t* msgs, size_t count, uint64_t* out) {
  const tfhe_rng_key rk = tfhe::client::rng_key_from_seed(seed);
  return tfhe_hip_lwe_encrypt_k(dim, key, noise_log2, &rk, stream0, msgs, count, out);
}

int tfhe_hip_lwe_phase(uint32_t dim, const uint64_t* key, const uint64_t* ct, size_t count, uint64_t* out) {
  if (!dim || !key || (count && (!ct || !out))) return fail(TFHE_HIP_EINVAL, "lwe_phase: bad arguments");
  tfhe::client::lwe_phase(dim, key, ct, count, out);
  return 0;
}

int tfhe_hip_lut_constant(uint32_t N, uint64_t v, uint64_t* lut) {
  if (!N || !lut) return fail(TFHE_HIP_EINVAL, "lut_constant: bad arguments");
  tfhe::client::lut_constant(N, v, lut);
  return 0;
}

int tfhe_hip_lut_from_table(uint32_t N, uint32_t msg_modulus, const uint64_t* table, uint64_t delta_out,
                            uint64_t* lut) {
  if (!N || !msg_modulus || msg_modulus > N || (N % msg_modulus) || !table || !lut)
    return fail(TFHE_HIP_EINVAL, "lut_from_table: bad arguments (N=%u, msg_modulus=%u)", N, msg_modulus);
  tfhe::client::lut_from_table(N, msg_modulus, table, delta_out, lut);
  return 0;
}

int tfhe_hip_create(const tfhe_params* p, const int* devices, int ndev, tfhe_ctx** out) {
  if (!out) return fail(TFHE_HIP_EINVAL, "create: null out");
  *out = nullptr;
  if (!params_valid(p)) return fail(TFHE_HIP_EINVAL, "create: invalid parameters");
  if (!params_on_device(p))
    return fail(TFHE_HIP_EUNSUPPORTED,
                "create: device kernels of this build cover P-GATE (k=1, N=1024, PBS 7x3, KS 2x8, PBS->KS; NTT or "
                "FFT64) and P-FHEVM (k=1, N=2048, PBS 23x1, KS 4x4, KS->PBS; NTT or FFT64); got "
                "k=%u N=%u pbs %ux%u ks %ux%u order %u transform %u",
                p->k, p->N, p->pbs_base_log, p->pbs_level, p->ks_base_log, p->ks_level, p->order, p->transform);
  if (!devices || ndev < 1 || ndev > 64) return fail(TFHE_HIP_EINVAL, "create: need 1..64 device ordinals, got %d", ndev);
  for (int i = 0; i < ndev; i++) RC_TRY(device_ordinal_check("create", devices[i], i));
  std::unique_ptr<tfhe_ctx> c(new tfhe_ctx());
  c->p = *p;
  c->eng = tfhe::find_engine(p->transform == TFHE_HIP_TRANSFORM_FFT64, p->N);
  if (!c->eng)
    return fail(TFHE_HIP_EUNSUPPORTED, "create: no blind-rotation back end for transform %u, N = %u", p->transform,
                p->N);
  c->eng_mb = tfhe::find_engine_mb(c->eng);
  c->lat_max = c->eng->lat_max;  // the measured latency-kernel crossover (each engine row says how)
  {
    const char* e = getenv("TFHE_HIP_KS_VALU");
    c->ks_valu = e && e[0] == '1';
  }
  c->sh.resize(ndev);
  for (int i = 0; i < ndev; i++) c->sh[i].device = devices[i];
  for (int i = 0; i < ndev; i++) {
    const int rc = shard_init(c.get(), c->sh[i]);
    if (rc) {
      std::string m = g_err;
      tfhe_hip_destroy(c.release());
      return fail(rc, "create: shard %d (device %d): %s", i, devices[i], m.c_str());
    }
  }
  *out = c.release();
  return 0;
}

void tfhe_hip_destroy(tfhe_ctx* c) {
  if (!c) return;
  for (auto& s : c->sh) shard_free(s);
  if (!c->comms.empty() && rccl().ok)
    for (auto cm : c->comms)
      if (cm) rccl().comm_destroy(cm);
  delete c;
}

int tfhe_hip_device(const tfhe_ctx* c) { return c && !c->sh.empty() ? c->sh[0].device : -1; }
int tfhe_hip_ndev(const tfhe_ctx* c) { return c ? (int)c->sh.size() : 0; }
int tfhe_hip_device_at(const tfhe_ctx* c, int i) {
  return c && i >= 0 && i < (int)c->sh.size() ? c->sh[(size_t)i].device : -1;
}
int tfhe_hip_key_bcast_mode(const tfhe_ctx* c) { return c ? c->bcast_mode : -1; }

int tfhe_hip_bcast_plan(const int* devices, int ndev, const char* policy, int rccl_available, int* mode, int* calls,
                        int max_calls) {
  if (!devices || ndev < 1 || !mode || (max_calls > 0 && !calls)) return fail(TFHE_HIP_EINVAL, "bcast_plan: bad arguments");
  std::string why;
  const int n = bcast_plan(ndev, ordinals_distinct(devices, ndev), policy, rccl_available != 0, mode,
                           max_calls > 0 ? calls : nullptr, max_calls, &why);
  return n < 0 ? fail(n, "bcast_plan: %s", why.c_str()) : n;
}

// ---- key loading: every tfhe_hip_load_keys* / tfhe_hip_load_bsk* call fills one key_load, key_load_check holds every
// refusal (all of them precede the first change of the ctx), key_load_run is the one pipeline.
enum key_source { SRC_HOST, SRC_DEVICE, SRC_SEEDED };

// What a load call asked for.  The words that travel to shard 0 and on to the other shards are the standard-domain
// keys of a host or device source and the bodies of a seeded one (include/tfhe_hip.h has the layouts).
struct key_load {
  const char* what;  // the call's name, the prefix of its messages
  key_source src;
  const uint64_t* bsk;
  size_t bsk_len;
  const uint64_t* ksk = nullptr;
  size_t ksk_len = 0;
  bool with_ksk = false;  // false: the BSK alone (ksk, ksk_len, ksk_seed unused), a rotation-only engine
  const uint64_t *bsk_seed = nullptr, *ksk_seed = nullptr;  // SRC_SEEDED only
  bool multi_bit = false;  // a multi-bit entry point: g must be a grouping factor; otherwise a classic key, g == 1
  uint32_t g = 1;
};

static size_t std_bsk_len(const tfhe_params& p, uint32_t g) {
  return g > 1 ? tfhe::client::mb_bsk_len(p, g) : tfhe::client::bsk_len(p);
}

static int native_torus_check(const tfhe_ctx* c, const char* what) {
  if (c->p.transform != TFHE_HIP_TRANSFORM_FFT64)
    return fail(TFHE_HIP_EUNSUPPORTED, "%s: seeded keys exist for the native-torus (FFT64) presets only", what);
  return 0;
}

// can this ctx hold a multi-bit key of grouping factor g
static int mb_key_check(const tfhe_ctx* c, const char* what, uint32_t g) {
  if (!c->eng_mb)
    return fail(TFHE_HIP_EUNSUPPORTED, "%s: the multi-bit back end covers the FFT64 transform at N = 2048 (PBS 23x1); "
                                       "this ctx runs transform %u, N = %u", what, c->p.transform, c->p.N);
  if (!grouping_valid(g) || g < c->eng_mb->g_min || g > c->eng_mb->g_max)
    return fail(TFHE_HIP_EINVAL, "%s: grouping factor %u, expected 2, 3 or 4", what, g);
  if (c->p.n % g) return fail(TFHE_HIP_EINVAL, "%s: n = %u is not divisible by the grouping factor %u", what, c->p.n, g);
  return 0;
}

static int key_load_check(const tfhe_ctx* c, const key_load& r) {
  const bool seeded = r.src == SRC_SEEDED;
  if (!c || !r.bsk || (r.with_ksk && !r.ksk) || (seeded && (!r.bsk_seed || (r.with_ksk && !r.ksk_seed))))
    return fail(TFHE_HIP_EINVAL, "%s: null argument", r.what);
  if (seeded) RC_TRY(native_torus_check(c, r.what));
  if (r.multi_bit) RC_TRY(mb_key_check(c, r.what, r.g));
  const size_t want_b = seeded ? tfhe::client::bsk_bodies_len(c->p, r.g) : std_bsk_len(c->p, r.g);
  const size_t want_k = seeded ? tfhe::client::ksk_bodies_len(c->p) : tfhe::client::ksk_len(c->p);
  if (r.bsk_len != want_b || (r.with_ksk && r.ksk_len != want_k))
    return fail(TFHE_HIP_EINVAL, "%s: %s %zu/%zu, expected %zu/%zu", r.what, seeded ? "body counts" : "sizes", r.bsk_len,
                r.with_ksk ? r.ksk_len : want_k, want_b, want_k);
  return 0;
}

static tfhe::seeded_shape seeded_shape_of(const tfhe_params& p, uint32_t g, uint32_t count = 0) {
  return tfhe::seeded_shape{p.n, p.k, p.N, p.pbs_level, p.ks_level, g, count};
}

// The pipeline of a checked load.  A seeded load leaves its three phases on shard 0's stream in c->seeded_ms
// (tfhe_hip_seeded_load_stats): phase 0 the upload, 1 the expansion, 2 the conversion.
static int key_load_run(tfhe_ctx* c, const key_load& r) {
  const bool seeded = r.src == SRC_SEEDED, with_ksk = r.with_ksk;
  const size_t nd = c->sh.size(), bsk_len = std_bsk_len(c->p, r.g), ksk_len = tfhe::client::ksk_len(c->p);
  // 1. prepare
  std::lock_guard<std::mutex> lk(c->mu);
  c->keys = c->bsk = false;  // after a BSK-only load an earlier KSK belongs to another key set: rotation-only
  c->grouping = 1;
  c->bcast_mode = 0;
  if (r.g > 1) {
    c->ms_count = 0;  // the noise-reduction pick is defined for the per-element switch
    std::vector<u64> tw(c->eng_mb->table_words);
    if (!c->eng_mb->make_tables(tw.data()))
      return fail(TFHE_HIP_EUNSUPPORTED, "%s: the host root table's entry 0 is not exactly 1", r.what);
    for (auto& s : c->sh) {
      if (s.d_tw_mb) continue;
      DeviceGuard gd(s.device);
      HIP_TRY(hipMalloc(&s.d_tw_mb, tw.size() * 8));
      HIP_TRY(hipMemcpy(s.d_tw_mb, tw.data(), tw.size() * 8, hipMemcpyHostToDevice));
    }
  }
  // every shard: key buffers + a standard-domain BSK staging area (its d_stage)
  for (auto& s : c->sh) {
    DeviceGuard g(s.device);
    RC_TRY(ws_host_wait(s));
    if (s.bsk_cap < bsk_len * 8) {
      HIP_TRY(hipStreamSynchronize(s.stream));
      (void)hipFree(s.d_bsk);
      s.d_bsk = nullptr;
      s.bsk_cap = 0;
      HIP_TRY(hipMalloc(&s.d_bsk, bsk_len * 8));
      s.bsk_cap = bsk_len * 8;
    }
    if (with_ksk && !s.d_ksk) HIP_TRY(hipMalloc(&s.d_ksk, ksk_len * 8));
    RC_TRY(ws_grow(s, &s.d_stage, &s.stage_cap, bsk_len * 8));
  }
  // 2. travel: onto shard 0, then to every other shard, once.  Standard keys land where the conversion reads them;
  // bodies (1 / (k + 1) and 1 / (n + 1) of the words) in temporaries, which the conversion's stream synchronise of
  // every shard precedes the release of.
  call_buffers tmp;
  std::vector<u64*> dst_b(nd), dst_k(nd);
  for (size_t i = 0; i < nd; i++) {
    shard& s = c->sh[i];
    dst_b[i] = (u64*)s.d_stage, dst_k[i] = s.d_ksk;
    if (!seeded) continue;
    RC_TRY(tmp.alloc(s.device, r.bsk_len * 8, &dst_b[i]));
    if (with_ksk) RC_TRY(tmp.alloc(s.device, r.ksk_len * 8, &dst_k[i]));
  }
  shard& s0 = c->sh[0];
  phase_timer tm(seeded ? &s0 : nullptr);
  // a device source is read in place on shard 0: the caller's BSK is broadcast and converted without a copy
  const u64* bsk0 = r.src == SRC_DEVICE ? (const u64*)r.bsk : dst_b[0];
  {
    DeviceGuard g(s0.device);
    RC_TRY(tm.tick(-1));
    if (r.src != SRC_DEVICE) {
      RC_TRY(upload_pinned(s0, dst_b[0], r.bsk, r.bsk_len * 8));
      if (with_ksk) RC_TRY(upload_pinned(s0, dst_k[0], r.ksk, r.ksk_len * 8));
    } else if (with_ksk) {
      HIP_TRY(hipMemcpyAsync(dst_k[0], r.ksk, r.ksk_len * 8, hipMemcpyDeviceToDevice, s0.stream));
      HIP_TRY(hipStreamSynchronize(s0.stream));
    }
    RC_TRY(tm.tick(0));
  }
  RC_TRY(broadcast(c, bsk0, dst_b, r.bsk_len));  // nothing to do on one shard (bcast_plan)
  if (with_ksk) RC_TRY(broadcast(c, dst_k[0], dst_k, r.ksk_len));
  const tfhe::seeded_round_keys rk_b = seeded ? round_keys_of(r.bsk_seed) : tfhe::seeded_round_keys{};
  const tfhe::seeded_round_keys rk_k = seeded && with_ksk ? round_keys_of(r.ksk_seed) : tfhe::seeded_round_keys{};
  const tfhe::seeded_shape shp = seeded_shape_of(c->p, r.g);
  for (size_t i = 0; i < nd; i++) {
    shard& s = c->sh[i];
    if (seeded) {  // 3. expand the bodies into the buffers that the other sources fill by copy
      DeviceGuard g(s.device);
      if (i == 0) RC_TRY(tm.tick(-1));
      HIP_TRY(tfhe::launch_seeded_rows(rk_b, r.g > 1 ? tfhe::SEEDED_BSK_MB : tfhe::SEEDED_BSK, shp, dst_b[i],
                                       (u64*)s.d_stage, s.stream));
      if (with_ksk) HIP_TRY(tfhe::launch_seeded_rows(rk_k, tfhe::SEEDED_KSK, shp, dst_k[i], s.d_ksk, s.stream));
      if (i == 0) RC_TRY(tm.tick(1));
    }
    // 4. convert (waits for the shard's stream)
    RC_TRY(convert_keys(c, s, i == 0 && !seeded ? bsk0 : (const u64*)s.d_stage, bsk_len, with_ksk));
    if (i == 0 && seeded) {
      RC_TRY(tm.tick(2));
      RC_TRY(tm.totals(c->seeded_ms, 3));
    }
  }
  // 5. commit
  c->bsk = true;
  c->keys = with_ksk;
  c->grouping = r.g;
  return 0;
}

static int load_from(tfhe_ctx* c, const key_load& r) {
  RC_TRY(key_load_check(c, r));
  return key_load_run(c, r);
}

int tfhe_hip_load_keys(tfhe_ctx* c, const uint64_t* bsk, size_t bsk_len, const uint64_t* ksk, size_t ksk_len) {
  return load_from(c, {"load_keys", SRC_HOST, bsk, bsk_len, ksk, ksk_len, true});
}

int tfhe_hip_load_keys_device(tfhe_ctx* c, const uint64_t* d_bsk, size_t bsk_len, const uint64_t* d_ksk,
                              size_t ksk_len) {
  return load_from(c, {"load_keys", SRC_DEVICE, d_bsk, bsk_len, d_ksk, ksk_len, true});
}

int tfhe_hip_load_bsk(tfhe_ctx* c, const uint64_t* bsk, size_t bsk_len) {
  return load_from(c, {"load_bsk", SRC_HOST, bsk, bsk_len});
}

int tfhe_hip_load_bsk_device(tfhe_ctx* c, const uint64_t* d_bsk, size_t bsk_len) {
  return load_from(c, {"load_bsk", SRC_DEVICE, d_bsk, bsk_len});
}

int tfhe_hip_load_keys_mb(tfhe_ctx* c, uint32_t g, const uint64_t* bsk_mb, size_t bsk_mb_len, const uint64_t* ksk,
                          size_t ksk_len) {
  return load_from(c, {"load_keys_mb", SRC_HOST, bsk_mb, bsk_mb_len, ksk, ksk_len, ksk != nullptr, nullptr, nullptr,
                       true, g});
}

int tfhe_hip_grouping(const tfhe_ctx* c) { return c ? (int)c->grouping : 1; }

int tfhe_hip_load_keys_seeded(tfhe_ctx* c, const uint64_t bsk_seed[2], const uint64_t* bsk_bodies, size_t bsk_bodies_len,
                              const uint64_t ksk_seed[2], const uint64_t* ksk_bodies, size_t ksk_bodies_len) {
  return load_from(c, {"load_keys_seeded", SRC_SEEDED, bsk_bodies, bsk_bodies_len, ksk_bodies, ksk_bodies_len, true,
                       bsk_seed, ksk_seed});
}

int tfhe_hip_load_bsk_seeded(tfhe_ctx* c, const uint64_t seed[2], const uint64_t* bodies, size_t bodies_len) {
  return load_from(c, {"load_bsk_seeded", SRC_SEEDED, bodies, bodies_len, nullptr, 0, false, seed});
}

int tfhe_hip_load_keys_mb_seeded(tfhe_ctx* c, uint32_t g, const uint64_t bsk_seed[2], const uint64_t* bsk_bodies,
                                 size_t bsk_bodies_len, const uint64_t ksk_seed[2], const uint64_t* ksk_bodies,
                                 size_t ksk_bodies_len) {
  return load_from(c, {"load_keys_mb_seeded", SRC_SEEDED, bsk_bodies, bsk_bodies_len, ksk_bodies, ksk_bodies_len,
                       ksk_bodies != nullptr, bsk_seed, ksk_seed, true, g});
}

int tfhe_hip_seeded_load_stats(const tfhe_ctx* c, double* upload_ms, double* expand_ms, double* convert_ms) {
  if (!c) return fail(TFHE_HIP_EINVAL, "seeded_load_stats: null ctx");
  return seeded_ms_read(c->seeded_ms, upload_ms, expand_ms, convert_ms);
}

// ---- the expansion kernels alone (test-facing): the launcher the loaders use, on shard 0, through guarded_expand
struct expand_job {
  tfhe::seeded_kind kind;
  tfhe::seeded_shape shp;
  size_t bodies_len, out_len;
};

static int seeded_expand_call(tfhe_ctx* c, const expand_job& j, const uint64_t seed[2], const uint64_t* bodies,
                              uint64_t* out_host) {
  const tfhe::seeded_round_keys rk = round_keys_of(seed);
  std::lock_guard<std::mutex> lk(c->mu);
  shard& s = c->sh[0];
  DeviceGuard gd(s.device);
  return guarded_expand(s, j.bodies_len * 8, j.out_len, out_host, [&](u64* d_bodies, u64* d_out) -> int {
    if (j.bodies_len) HIP_TRY(hipMemcpyAsync(d_bodies, bodies, j.bodies_len * 8, hipMemcpyHostToDevice, s.stream));
    HIP_TRY(tfhe::launch_seeded_rows(rk, j.kind, j.shp, d_bodies, d_out, s.stream));
    return 0;
  });
}

int tfhe_hip_seeded_expand_bsk(tfhe_ctx* c, uint32_t g, const uint64_t seed[2], const uint64_t* bodies,
                               uint64_t* out_host) {
  if (!c || !seed || !bodies) return fail(TFHE_HIP_EINVAL, "seeded_expand_bsk: null argument");
  if (g == 0) return fail(TFHE_HIP_EINVAL, "seeded_expand_bsk: grouping factor 0");
  RC_TRY(native_torus_check(c, "seeded_expand_bsk"));
  if (g > 1) RC_TRY(mb_key_check(c, "seeded_expand_bsk", g));
  if (!out_host) return fail(TFHE_HIP_EINVAL, "seeded_expand_bsk: null argument");
  return seeded_expand_call(c, {g > 1 ? tfhe::SEEDED_BSK_MB : tfhe::SEEDED_BSK, seeded_shape_of(c->p, g),
                                tfhe::client::bsk_bodies_len(c->p, g), std_bsk_len(c->p, g)},
                            seed, bodies, out_host);
}

int tfhe_hip_seeded_expand_ksk(tfhe_ctx* c, const uint64_t seed[2], const uint64_t* bodies, uint64_t* out_host) {
  if (!c || !seed || !bodies || !out_host) return fail(TFHE_HIP_EINVAL, "seeded_expand_ksk: null argument");
  RC_TRY(native_torus_check(c, "seeded_expand_ksk"));
  return seeded_expand_call(c, {tfhe::SEEDED_KSK, seeded_shape_of(c->p, 1), tfhe::client::ksk_bodies_len(c->p),
                                tfhe::client::ksk_len(c->p)},
                            seed, bodies, out_host);
}

int tfhe_hip_seeded_expand_lwe_list(tfhe_ctx* c, uint32_t dim, uint32_t count, const uint64_t seed[2],
                                    const uint64_t* bodies, uint64_t* out_host) {
  if (!c || !seed || !out_host || (count && !bodies)) return fail(TFHE_HIP_EINVAL, "seeded_expand_lwe_list: null argument");
  if (dim == 0 || dim > 0x7FFFFFFEu || count > 0x7FFFFFFFu)
    return fail(TFHE_HIP_EINVAL, "seeded_expand_lwe_list: dim = %u, count = %u out of range", dim, count);
  tfhe::seeded_shape shp{};
  shp.n = dim, shp.count = count;
  return seeded_expand_call(c, {tfhe::SEEDED_LIST, shp, count, (size_t)count * ((size_t)dim + 1)}, seed, bodies,
                            out_host);
}

// ---- the modulus-switch zeros (tfhe_hip_load_ms_key*)
struct ms_tuning {
  double bound, r_sigma, input_variance;
};

// the checks behind the argument check, shared by the host and the seeded source
static int ms_key_check(const tfhe_ctx* c, const char* what, uint32_t count, const ms_tuning& t) {
  if (c->grouping > 1)
    return fail(TFHE_HIP_EUNSUPPORTED, "%s: multi-bit keys are loaded (grouping %u); the noise-reduction pick "
                                       "is defined for the per-element modulus switch", what, c->grouping);
  if (c->p.order != 1 && count)
    return fail(TFHE_HIP_EUNSUPPORTED, "%s: the noise reduction runs between keyswitch and blind rotation "
                                       "(KS -> PBS parameter sets only)", what);
  if (count > 0x7FFFFFFF || !(t.bound >= 0) || !(t.r_sigma >= 0) || !(t.input_variance >= 0))
    return fail(TFHE_HIP_EINVAL, "%s: count %u / bound / r_sigma / variance out of range", what, count);
  // the scan addresses the element-major transpose through a buffer resource with 32-bit byte offsets
  // (ms_reduce.hip): (n + 1) x pitch x 8 must stay below 2^31, or raw loads past num_records would read zeros
  // silently.  n = 918 allows ~292 k zeros; the reference's key carries 1449.
  if ((double)(c->p.n + 1) * (double)tfhe::ms_zeros_pitch(count) * 8.0 >= 0x1p31)
    return fail(TFHE_HIP_EINVAL, "%s: %u zeros x %u elements exceed the 2 GiB scan window", what, count,
                (unsigned)(c->p.n + 1));
  return 0;
}

// Install `count` checked zeros on every shard (0: disable the reduction and free the buffer).  Two layouts in one
// allocation: rows [count][n+1] (the add of the chosen zero), which fill_rows(shard) puts at s.d_ms_zeros by a copy
// or by work on the shard's stream, then the element-major transpose [n+1][zp] that the scan reads 64 zeros per load
// from (pbs_kernels.h: ms_zeros_pitch), built from the rows on the device.
static int install_ms_zeros(tfhe_ctx* c, uint32_t count, const ms_tuning& t,
                            const std::function<int(shard&)>& fill_rows) {
  std::lock_guard<std::mutex> lk(c->mu);
  c->ms_count = 0;
  const size_t dim = c->p.n + 1, zp = tfhe::ms_zeros_pitch(count);
  for (auto& s : c->sh) {
    DeviceGuard g(s.device);
    HIP_TRY(hipStreamSynchronize(s.stream));
    RC_TRY(ws_host_wait(s));
    (void)hipFree(s.d_ms_zeros);
    s.d_ms_zeros = nullptr;
    if (!count) continue;
    HIP_TRY(hipMalloc(&s.d_ms_zeros, (count * dim + dim * zp) * 8));
    RC_TRY(fill_rows(s));
    HIP_TRY(tfhe::launch_ms_zeros_transpose(s.d_ms_zeros, count, (u32)dim, s.d_ms_zeros + count * dim, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));  // before the caller releases what fill_rows reads
  }
  c->ms_count = count;
  c->ms_bound = t.bound;
  c->ms_r_sigma = t.r_sigma;
  c->ms_var128 = t.input_variance * 0x1p128;
  return 0;
}

int tfhe_hip_load_ms_key(tfhe_ctx* c, const uint64_t* zeros, uint32_t count, double bound, double r_sigma,
                         double input_variance) {
  if (!c || (count && !zeros)) return fail(TFHE_HIP_EINVAL, "load_ms_key: bad arguments");
  const ms_tuning t{bound, r_sigma, input_variance};
  RC_TRY(ms_key_check(c, "load_ms_key", count, t));
  return install_ms_zeros(c, count, t, [&](shard& s) -> int {
    HIP_TRY(hipMemcpyAsync(s.d_ms_zeros, zeros, (size_t)count * (c->p.n + 1) * 8, hipMemcpyHostToDevice, s.stream));
    return 0;
  });
}

// The zeros from their seeded form: count body words go to every shard, which expands the rows on its own stream.
int tfhe_hip_load_ms_key_seeded(tfhe_ctx* c, const uint64_t seed[2], const uint64_t* bodies, uint32_t count,
                                double bound, double r_sigma, double input_variance) {
  if (!c || (count && (!seed || !bodies))) return fail(TFHE_HIP_EINVAL, "load_ms_key_seeded: bad arguments");
  RC_TRY(native_torus_check(c, "load_ms_key_seeded"));
  const ms_tuning t{bound, r_sigma, input_variance};
  RC_TRY(ms_key_check(c, "load_ms_key_seeded", count, t));
  const tfhe::seeded_round_keys rk = count ? round_keys_of(seed) : tfhe::seeded_round_keys{};
  tfhe::seeded_shape shp{};
  shp.n = c->p.n, shp.count = count;
  call_buffers tmp;  // every shard's bodies, released after the installer's last synchronise
  return install_ms_zeros(c, count, t, [&](shard& s) -> int {
    u64* d_bodies = nullptr;
    RC_TRY(tmp.alloc(s.device, (size_t)count * 8, &d_bodies));
    HIP_TRY(hipMemcpyAsync(d_bodies, bodies, (size_t)count * 8, hipMemcpyHostToDevice, s.stream));
    HIP_TRY(tfhe::launch_seeded_rows(rk, tfhe::SEEDED_LIST, shp, d_bodies, s.d_ms_zeros, s.stream));
    return 0;
  });
}

int tfhe_hip_ms_reduce(tfhe_ctx* c, const uint64_t* in, size_t B, uint64_t* out, int32_t* picks) {
  if (!c || (B && (!in || !out))) return fail(TFHE_HIP_EINVAL, "ms_reduce: bad arguments");
  if (c->p.order != 1) return fail(TFHE_HIP_EUNSUPPORTED, "ms_reduce: KS -> PBS parameter sets only");
  if (c->grouping > 1)
    return fail(TFHE_HIP_EUNSUPPORTED, "ms_reduce: multi-bit keys are loaded (grouping %u); the noise-reduction pick is "
                                       "defined for the per-element modulus switch", c->grouping);
  if (B == 0) return 0;
  if (B > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "ms_reduce: batch too large");
  const size_t bytes = B * ((size_t)c->p.n + 1) * 8;
  return staged_call(c, {{in, bytes}}, B * 4, {{out, 0, bytes}, {picks, 1, B * 4}},
                     [&](shard& s, std::vector<void*>& d) -> int {
                       HIP_TRY(launch_ms(c, s, (u64*)d[0], B, (int*)d[1], s.stream));
                       return 0;
                     });
}

int tfhe_hip_pbs_async(tfhe_ctx* c, const uint64_t* d_in, size_t B, const uint64_t* d_luts, size_t n_lut,
                       const uint32_t* d_idx, uint64_t* d_out, void* stream) {
  return pbs_async_call(c, "pbs", d_in, B, d_luts, n_lut, d_idx, pbs_kind{}, d_out, stream);
}

int tfhe_hip_pbs(tfhe_ctx* c, const uint64_t* lwe_in, size_t B, const uint64_t* luts, size_t n_lut,
                 const uint32_t* lut_index, uint64_t* lwe_out) {
  return pbs_host_call(c, "pbs", lwe_in, B, luts, n_lut, lut_index, pbs_kind{}, lwe_out);
}

int tfhe_hip_pbs_many_async(tfhe_ctx* c, const uint64_t* d_in, size_t B, const uint64_t* d_luts, size_t n_lut,
                            const uint32_t* d_idx, uint32_t n_fn, uint32_t stride, uint64_t* d_out, void* stream) {
  const many_args m{n_fn, stride};
  return pbs_async_call(c, "pbs_many", d_in, B, d_luts, n_lut, d_idx, pbs_kind{&m, false}, d_out, stream);
}

int tfhe_hip_pbs_many(tfhe_ctx* c, const uint64_t* lwe_in, size_t B, const uint64_t* luts, size_t n_lut,
                      const uint32_t* lut_index, uint32_t n_fn, uint32_t stride, uint64_t* lwe_out) {
  const many_args m{n_fn, stride};
  return pbs_host_call(c, "pbs_many", lwe_in, B, luts, n_lut, lut_index, pbs_kind{&m, false}, lwe_out);
}

int tfhe_hip_bootstrap_async(tfhe_ctx* c, const uint64_t* d_in, size_t B, const uint64_t* d_luts, size_t n_lut,
                             const uint32_t* d_idx, uint64_t* d_out, void* stream) {
  return pbs_async_call(c, "bootstrap", d_in, B, d_luts, n_lut, d_idx, pbs_kind{nullptr, true}, d_out, stream);
}

int tfhe_hip_bootstrap(tfhe_ctx* c, const uint64_t* lwe_in, size_t B, const uint64_t* luts, size_t n_lut,
                       const uint32_t* lut_index, uint64_t* lwe_big_out) {
  return pbs_host_call(c, "bootstrap", lwe_in, B, luts, n_lut, lut_index, pbs_kind{nullptr, true}, lwe_big_out);
}

int tfhe_hip_decompress_async(tfhe_ctx* c, const tfhe_pks_params* pp, const uint64_t* d_packed, size_t packed_words,
                              size_t count, const uint64_t* d_luts, size_t n_lut, const uint32_t* d_idx,
                              uint64_t* d_out, void* stream) {
  RC_TRY(decompress_check(c, pp, d_packed, packed_words, count, d_luts, n_lut, d_out));
  if (count == 0) return 0;
  return async_call(c, "decompress", d_packed, stream, true, [&](shard& s, hipStream_t st) {
    return decompress_device(c, s, *pp, d_packed, count, d_luts, n_lut, d_idx, d_out, st);
  });
}

int tfhe_hip_decompress(tfhe_ctx* c, const tfhe_pks_params* pp, const uint64_t* packed, size_t packed_words,
                        size_t count, const uint64_t* luts, size_t n_lut, const uint32_t* lut_index,
                        uint64_t* lwe_big_out) {
  RC_TRY(decompress_check(c, pp, packed, packed_words, count, luts, n_lut, lwe_big_out));
  if (count == 0) return 0;
  RC_TRY(host_lut_index_check("decompress", lut_index, count, n_lut));
  const size_t out_bytes = count * ((size_t)c->p.k * c->p.N + 1) * 8;
  return staged_call(c, {{packed, packed_words * 8}, {luts, n_lut * c->p.N * 8}, {lut_index, lut_index ? count * 4 : 0}},
                     out_bytes, {{lwe_big_out, 3, out_bytes}}, [&](shard& s, std::vector<void*>& d) {
                       return decompress_device(c, s, *pp, (const u64*)d[0], count, (const u64*)d[1], n_lut,
                                                (const u32*)d[2], (u64*)d[3], s.stream);
                     });
}

size_t tfhe_hip_compact_list_words(uint32_t lwe_dim, size_t count) {
  if (!expand_dim_ok(lwe_dim) || count == 0) return 0;
  return (count + lwe_dim - 1) / lwe_dim * lwe_dim + count;
}

int tfhe_hip_expand_compact_async(tfhe_ctx* c, const uint64_t* d_list, size_t list_words, uint32_t lwe_dim, size_t count,
                                  uint32_t rep, size_t rows, uint64_t* d_lwes_out, void* stream) {
  RC_TRY(expand_check(c, d_list, list_words, lwe_dim, count, rep, rows, d_lwes_out));
  if (rows == 0) return 0;
  return async_call(c, "expand_compact", d_list, stream, false, [&](shard& s, hipStream_t st) {  // no workspace
    return expand_device(c, s, d_list, count, lwe_dim, rep, rows, d_lwes_out, st);
  });
}

int tfhe_hip_expand_compact(tfhe_ctx* c, const uint64_t* list, size_t list_words, uint32_t lwe_dim, size_t count,
                            uint32_t rep, size_t rows, uint64_t* lwes_out) {
  RC_TRY(expand_check(c, list, list_words, lwe_dim, count, rep, rows, lwes_out));
  if (rows == 0) return 0;
  const size_t out_bytes = rows * ((size_t)lwe_dim + 1) * 8;
  return staged_call(c, {{list, list_words * 8}}, out_bytes, {{lwes_out, 1, out_bytes}},
                     [&](shard& s, std::vector<void*>& d) {
                       return expand_device(c, s, (const u64*)d[0], count, lwe_dim, rep, rows, (u64*)d[1], s.stream);
                     });
}

int tfhe_hip_expand_cast_async(tfhe_ctx* c, const uint64_t* d_list, size_t list_words, size_t count, uint32_t rep,
                               size_t rows, const uint64_t* d_luts, size_t n_lut, const uint32_t* d_idx,
                               uint64_t* d_out, void* stream) {
  RC_TRY(expand_cast_check(c, d_list, list_words, count, rep, rows, d_luts, n_lut, d_out));
  if (rows == 0) return 0;
  return async_call(c, "expand_cast", d_list, stream, true, [&](shard& s, hipStream_t st) {
    return expand_cast_device(c, s, d_list, count, rep, rows, d_luts, n_lut, d_idx, d_out, st);
  });
}

int tfhe_hip_expand_cast(tfhe_ctx* c, const uint64_t* list, size_t list_words, size_t count, uint32_t rep, size_t rows,
                         const uint64_t* luts, size_t n_lut, const uint32_t* lut_index, uint64_t* lwe_out) {
  RC_TRY(expand_cast_check(c, list, list_words, count, rep, rows, luts, n_lut, lwe_out));
  RC_TRY(host_lut_index_check("expand_cast", lut_index, rows, n_lut));
  if (rows == 0) return 0;
  const size_t out_bytes = rows * ((size_t)io_dim(c->p) + 1) * 8;
  return staged_call(c, {{list, list_words * 8}, {luts, n_lut * c->p.N * 8}, {lut_index, lut_index ? rows * 4 : 0}},
                     out_bytes, {{lwe_out, 3, out_bytes}}, [&](shard& s, std::vector<void*>& d) {
                       return expand_cast_device(c, s, (const u64*)d[0], count, rep, rows, (const u64*)d[1], n_lut,
                                                 (const u32*)d[2], (u64*)d[3], s.stream);
                     });
}

int tfhe_hip_lut_oprf(uint32_t N, uint32_t random_bits, uint32_t full_bits, uint64_t* lut, uint64_t* post_add) {
  if (!N || (N & (N - 1)) || !lut || !post_add) return fail(TFHE_HIP_EINVAL, "lut_oprf: bad arguments (N = %u)", N);
  if (random_bits < 1 || random_bits >= full_bits || full_bits > 63)
    return fail(TFHE_HIP_EINVAL, "lut_oprf: need 1 <= random_bits < full_bits <= 63, got %u and %u", random_bits,
                full_bits);
  const uint64_t p = 1ull << random_bits;
  if (p > 2ull * N) return fail(TFHE_HIP_EINVAL, "lut_oprf: 2^random_bits = 2^%u exceeds 2N = %u", random_bits, 2 * N);
  const uint64_t half = 1ull << (63 - full_bits), box = 2ull * N / p;  // delta / 2; x values per step
  for (uint32_t x = 0; x < N; x++) lut[x] = (2 * (x / box) + 1) * half;
  *post_add = (p - 1) * half;
  return 0;
}

// tfhe_hip_csprng_rows*: every check that precedes device work; rows == 0 passes
static int csprng_check(const tfhe_ctx* c, const void* seeds, size_t rows, uint64_t first_word, uint32_t dim,
                        size_t row_stride, const void* out) {
  if (!c) return fail(TFHE_HIP_EINVAL, "csprng_rows: null ctx");
  if (!dim) return fail(TFHE_HIP_EINVAL, "csprng_rows: dim == 0");
  if (row_stride < dim) return fail(TFHE_HIP_EINVAL, "csprng_rows: row_stride = %zu < dim = %u", row_stride, dim);
  if (first_word > (1ull << 60) || dim > (1ull << 60) - first_word)
    return fail(TFHE_HIP_EINVAL, "csprng_rows: first_word + dim exceeds 2^60");
  if (rows > 0x7FFFFFFF || rows > 0x7FFFFFFF / (((size_t)dim + 1021) / 1022))
    return fail(TFHE_HIP_EINVAL, "csprng_rows: rows = %zu x dim = %u, too large for one call", rows, dim);
  if (rows && (!seeds || !out)) return fail(TFHE_HIP_EINVAL, "csprng_rows: null buffer");
  return 0;
}

int tfhe_hip_csprng_rows_async(tfhe_ctx* c, const uint64_t* d_seeds, size_t rows, uint64_t first_word, uint32_t dim,
                               size_t row_stride, uint64_t* d_out, void* stream) {
  RC_TRY(csprng_check(c, d_seeds, rows, first_word, dim, row_stride, d_out));
  if (rows == 0) return 0;
  return async_call(c, "csprng_rows", d_seeds, stream, false, [&](shard& s, hipStream_t st) {  // no workspace
    return csprng_device(c, s, d_seeds, rows, first_word, dim, row_stride, false, d_out, st);
  });
}

int tfhe_hip_csprng_rows(tfhe_ctx* c, const uint64_t* seeds, size_t rows, uint64_t first_word, uint32_t dim,
                         uint64_t* out) {
  RC_TRY(csprng_check(c, seeds, rows, first_word, dim, dim, out));
  if (rows == 0) return 0;
  const size_t out_bytes = rows * (size_t)dim * 8;
  return staged_call(c, {{seeds, rows * 16}}, out_bytes, {{out, 1, out_bytes}}, [&](shard& s, std::vector<void*>& d) {
    return csprng_device(c, s, (const u64*)d[0], rows, first_word, dim, dim, false, (u64*)d[1], s.stream);
  });
}

int tfhe_hip_oprf_async(tfhe_ctx* c, const uint64_t* d_seeds, size_t rows, const uint64_t* d_luts,
                        const uint64_t* d_post_adds, size_t n_lut, const uint32_t* d_idx, uint64_t* d_out,
                        void* stream) {
  RC_TRY(oprf_check(c, d_seeds, rows, d_luts, d_post_adds, n_lut, d_out));
  if (rows == 0) return 0;
  return async_call(c, "oprf", d_seeds, stream, true, [&](shard& s, hipStream_t st) {
    return oprf_device(c, s, d_seeds, rows, d_luts, d_post_adds, n_lut, d_idx, d_out, st);
  });
}

int tfhe_hip_oprf(tfhe_ctx* c, const uint64_t* seeds, size_t rows, const uint64_t* luts, const uint64_t* post_adds,
                  size_t n_lut, const uint32_t* lut_index, uint64_t* lwe_out) {
  RC_TRY(oprf_check(c, seeds, rows, luts, post_adds, n_lut, lwe_out));
  if (rows == 0) return 0;
  RC_TRY(host_lut_index_check("oprf", lut_index, rows, n_lut));
  std::lock_guard<std::mutex> lk(c->mu);
  const size_t out_dim = (size_t)io_dim(c->p) + 1;
  return for_each_slice(c, rows, [&](size_t i, size_t lo, size_t hi) -> int {
    const size_t b = hi - lo;
    return staged_run(c->sh[i],
                      {{seeds + 2 * lo, b * 16}, {luts, n_lut * c->p.N * 8}, {post_adds, n_lut * 8},
                       {lut_index ? lut_index + lo : nullptr, lut_index ? b * 4 : 0}},
                      b * out_dim * 8, {{lwe_out + lo * out_dim, 4, b * out_dim * 8}},
                      [&](shard& s, std::vector<void*>& d) {
                        return oprf_device(c, s, (const u64*)d[0], b, (const u64*)d[1], (const u64*)d[2], n_lut,
                                           (const u32*)d[3], (u64*)d[4], s.stream);
                      });
  });
}

int tfhe_hip_lwe_lincomb_async(tfhe_ctx* c, uint32_t dim, const uint64_t* const* d_bufs, const size_t* buf_rows,
                               size_t n_buf, const uint32_t* row_start, const uint32_t* term_buf,
                               const uint32_t* term_row, const uint64_t* term_coef, const uint64_t* bias, size_t rows,
                               uint64_t* d_out, void* stream) {
  if (!c) return fail(TFHE_HIP_EINVAL, "lwe_lincomb: null ctx");
  const lin_desc L{row_start, term_buf, term_row, term_coef, bias};
  RC_TRY(lincomb_check("lwe_lincomb", dim, buf_rows, n_buf, L, rows));
  if (rows == 0) return 0;
  if (!d_out || (row_start[rows] && !term_buf)) return fail(TFHE_HIP_EINVAL, "lwe_lincomb: null buffer");
  RC_TRY(lincomb_ptr_check("lwe_lincomb", dim, d_bufs, buf_rows, n_buf, rows, d_out));
  return async_call(c, "lwe_lincomb", d_out, stream, true, [&](shard& s, hipStream_t st) {
    return lincomb_device(c, s, dim, d_bufs, L, rows, d_out, st);
  });
}

int tfhe_hip_lwe_lincomb(tfhe_ctx* c, uint32_t dim, const uint64_t* src, size_t src_rows, const uint32_t* row_start,
                         const uint32_t* term_row, const uint64_t* term_coef, const uint64_t* bias, size_t rows,
                         uint64_t* out) {
  if (!c) return fail(TFHE_HIP_EINVAL, "lwe_lincomb: null ctx");
  const lin_desc L{row_start, nullptr, term_row, term_coef, bias};
  RC_TRY(lincomb_check("lwe_lincomb", dim, &src_rows, 1, L, rows));
  if (rows == 0) return 0;
  if (!out || (src_rows && !src)) return fail(TFHE_HIP_EINVAL, "lwe_lincomb: null buffer");
  const size_t out_bytes = rows * (size_t)dim * 8;
  return staged_call(c, {{src, src_rows * (size_t)dim * 8}}, out_bytes, {{out, 1, out_bytes}},
                     [&](shard& s, std::vector<void*>& d) {
                       const uint64_t* bufs[1] = {(const u64*)d[0]};
                       return lincomb_device(c, s, dim, bufs, L, rows, (u64*)d[1], s.stream);
                     });
}

int tfhe_hip_lincomb_pbs_async(tfhe_ctx* c, const uint64_t* const* d_bufs, const size_t* buf_rows, size_t n_buf,
                               const uint32_t* row_start, const uint32_t* term_buf, const uint32_t* term_row,
                               const uint64_t* term_coef, const uint64_t* bias, size_t rows, const uint64_t* d_luts,
                               size_t n_lut, const uint32_t* d_idx, uint64_t* d_out, void* stream) {
  RC_TRY(pbs_check(c, "lincomb_pbs", d_out, rows, d_luts, n_lut, pbs_kind{}, d_out));
  const uint32_t dim = io_dim(c->p) + 1;
  const lin_desc L{row_start, term_buf, term_row, term_coef, bias};
  RC_TRY(lincomb_check("lincomb_pbs", dim, buf_rows, n_buf, L, rows));
  if (rows == 0) return 0;
  if (row_start[rows] && !term_buf) return fail(TFHE_HIP_EINVAL, "lincomb_pbs: null buffer");
  RC_TRY(lincomb_ptr_check("lincomb_pbs", dim, d_bufs, buf_rows, n_buf, rows, nullptr));
  return async_call(c, "lincomb_pbs", d_out, stream, true, [&](shard& s, hipStream_t st) -> int {
    RC_TRY(ws_grow(s, (void**)&s.d_lin, &s.lin_cap, rows * (size_t)dim * sizeof(u64)));
    RC_TRY(lincomb_device(c, s, dim, d_bufs, L, rows, s.d_lin, st));
    return pbs_device(c, s, s.d_lin, rows, d_luts, n_lut, d_idx, nullptr, d_out, st);
  });
}

int tfhe_hip_blind_rotate(tfhe_ctx* c, const uint64_t* lwe_in, size_t B, const uint64_t* luts, size_t n_lut,
                          const uint32_t* lut_index, uint64_t* acc_out) {
  if (!c) return fail(TFHE_HIP_EINVAL, "blind_rotate: null ctx");
  if (!c->bsk) return fail(TFHE_HIP_ENOKEYS, "blind_rotate: keys not loaded");
  if (B == 0) return 0;
  if (!lwe_in || !luts || !n_lut || !acc_out) return fail(TFHE_HIP_EINVAL, "blind_rotate: null buffer");
  if (lut_index)
    for (size_t q = 0; q < B; q++)
      if (lut_index[q] >= n_lut) return fail(TFHE_HIP_EINVAL, "blind_rotate: lut_index[%zu] >= n_lut", q);
  const size_t din = (size_t)c->p.n + 1, acc_bytes = B * (size_t)(c->p.k + 1) * c->p.N * 8;
  return staged_call(c, {{lwe_in, B * din * 8}, {luts, n_lut * c->p.N * 8}, {lut_index, lut_index ? B * 4 : 0}},
                     acc_bytes, {{acc_out, 3, acc_bytes}}, [&](shard& s, std::vector<void*>& d) -> int {
                       HIP_TRY(launch_br(c, s, (const u64*)d[0], B, (const u64*)d[1], (const u32*)d[2], n_lut, nullptr,
                                         (u64*)d[3], s.stream));
                       return 0;
                     });
}

int tfhe_hip_sample_extract(tfhe_ctx* c, const uint64_t* acc, size_t B, uint64_t* out) {
  if (!c || (B && (!acc || !out))) return fail(TFHE_HIP_EINVAL, "sample_extract: bad arguments");
  if (B == 0) return 0;
  const size_t acc_len = (size_t)(c->p.k + 1) * c->p.N, big = (size_t)c->p.k * c->p.N + 1;
  return staged_call(c, {{acc, B * acc_len * 8}}, B * big * 8, {{out, 1, B * big * 8}},
                     [&](shard& s, std::vector<void*>& d) -> int {
                       HIP_TRY(tfhe::launch_sample_extract_many((const u64*)d[0], B, (int)c->p.k, (int)c->p.N,
                                                                !c->eng->fft, 1, 1, (u64*)d[1], s.stream));
                       return 0;
                     });
}

int tfhe_hip_sample_extract_many(tfhe_ctx* c, const uint64_t* acc, size_t B, uint32_t n_fn, uint32_t stride,
                                 uint64_t* out) {
  if (!c || (B && (!acc || !out))) return fail(TFHE_HIP_EINVAL, "sample_extract_many: bad arguments");
  RC_TRY(check_many(c, "sample_extract_many", B, n_fn, stride));
  if (B == 0) return 0;
  const size_t acc_len = (size_t)(c->p.k + 1) * c->p.N, out_bytes = B * n_fn * ((size_t)c->p.k * c->p.N + 1) * 8;
  return staged_call(c, {{acc, B * acc_len * 8}}, out_bytes, {{out, 1, out_bytes}},
                     [&](shard& s, std::vector<void*>& d) -> int {
                       HIP_TRY(tfhe::launch_sample_extract_many((const u64*)d[0], B, (int)c->p.k, (int)c->p.N,
                                                                !c->eng->fft, (int)n_fn, (int)stride, (u64*)d[1],
                                                                s.stream));
                       return 0;
                     });
}

int tfhe_hip_keyswitch(tfhe_ctx* c, const uint64_t* in, size_t B, uint64_t* out) {
  if (!c || (B && (!in || !out))) return fail(TFHE_HIP_EINVAL, "keyswitch: bad arguments");
  if (!c->keys) return fail(TFHE_HIP_ENOKEYS, "keyswitch: keys not loaded");
  if (B == 0) return 0;
  const size_t big = (size_t)c->p.k * c->p.N + 1, small = (size_t)c->p.n + 1;
  return staged_call(c, {{in, B * big * 8}}, B * small * 8, {{out, 1, B * small * 8}},
                     [&](shard& s, std::vector<void*>& d) {
                       return launch_ks(c, s, (const u64*)d[0], B, (u64*)d[1], s.stream);
                     });
}

static int ntt_impl(tfhe_ctx* c, uint64_t* polys, size_t count, bool inverse) {
  if (!c || (count && !polys)) return fail(TFHE_HIP_EINVAL, "ntt: bad arguments");
  if (c->eng->fft) return fail(TFHE_HIP_EUNSUPPORTED, "ntt: this ctx runs the FFT64 transform (tfhe_hip_fft_*)");
  if (count == 0) return 0;
  for (size_t i = 0; i < count * c->p.N; i++)
    if (polys[i] >= tfhe::GL_P) return fail(TFHE_HIP_EINVAL, "ntt: value at %zu not reduced mod p", i);
  const size_t bytes = count * c->p.N * 8;
  return staged_call(c, {{polys, bytes}}, 0, {{polys, 0, bytes}}, [&](shard& s, std::vector<void*>& d) -> int {
    HIP_TRY((inverse ? c->eng->inv : c->eng->fwd)((const u64*)d[0], count, (u64*)d[0], s.d_tw, s.stream));  // in place
    return 0;
  });
}

int tfhe_hip_ntt_fwd(tfhe_ctx* c, uint64_t* polys, size_t count) { return ntt_impl(c, polys, count, false); }
int tfhe_hip_ntt_inv(tfhe_ctx* c, uint64_t* polys, size_t count) { return ntt_impl(c, polys, count, true); }

static int fft_impl(tfhe_ctx* c, const void* in, size_t count, double* out, bool inverse) {
  if (!c || (count && (!in || !out))) return fail(TFHE_HIP_EINVAL, "fft: bad arguments");
  if (!c->eng->fft) return fail(TFHE_HIP_EUNSUPPORTED, "fft: ctx transform is not FFT64");
  if (count == 0) return 0;
  const size_t bytes = count * c->p.N * 8;
  return staged_call(c, {{in, bytes}}, bytes, {{out, 1, bytes}}, [&](shard& s, std::vector<void*>& d) -> int {
    HIP_TRY((inverse ? c->eng->inv : c->eng->fwd)((const u64*)d[0], count, (u64*)d[1], s.d_tw, s.stream));
    return 0;
  });
}

int tfhe_hip_fft_fwd(tfhe_ctx* c, const uint64_t* polys, size_t count, double* out) {
  return fft_impl(c, polys, count, out, false);
}
int tfhe_hip_fft_inv(tfhe_ctx* c, const double* in, size_t count, double* out) {
  return fft_impl(c, in, count, out, true);
}

int tfhe_hip_nand(tfhe_ctx* c, const uint64_t* c1, const uint64_t* c2, size_t B, uint64_t* out) {
  if (!c || (B && (!c1 || !c2 || !out))) return fail(TFHE_HIP_EINVAL, "nand: bad arguments");
  if (c->p.order != 0) return fail(TFHE_HIP_EUNSUPPORTED, "nand: gate bootstrapping needs a PBS->KS (small-key) parameter set");
  if (B == 0) return 0;
  const size_t dim = (size_t)c->p.n + 1;
  std::vector<u64> in(B * dim), lut(c->p.N);
  const u64 mu = 1ull << 61;  // 1/8
  for (size_t q = 0; q < B; q++) {
    for (size_t i = 0; i + 1 < dim; i++) in[q * dim + i] = 0 - c1[q * dim + i] - c2[q * dim + i];
    in[q * dim + dim - 1] = mu - c1[q * dim + dim - 1] - c2[q * dim + dim - 1];
  }
  tfhe::client::lut_constant(c->p.N, mu, lut.data());
  return tfhe_hip_pbs(c, in.data(), B, lut.data(), 1, nullptr, out);
}

int tfhe_hip_set_latency_batch(tfhe_ctx* c, size_t max_batch) {
  if (!c) return fail(TFHE_HIP_EINVAL, "set_latency_batch: null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  c->lat_max = max_batch;
  return 0;
}

const char* tfhe_hip_br_kernel(const tfhe_ctx* c, size_t B) {
  if (!c) return nullptr;
  if (c->grouping > 1) return c->eng_mb->kernel;
  return latency_batch(c, B) ? c->eng->lat_kernel : c->eng->batch_kernel;
}

int tfhe_hip_sync(tfhe_ctx* c) {
  if (!c) return fail(TFHE_HIP_EINVAL, "sync: null ctx");
  for (auto& s : c->sh) {
    DeviceGuard g(s.device);
    HIP_TRY(hipStreamSynchronize(s.stream));
    RC_TRY(ws_host_wait(s));
  }
  return 0;
}

int tfhe_hip_timing_enable(tfhe_ctx* c, int enable) {
  if (!c) return fail(TFHE_HIP_EINVAL, "timing: null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  c->timing = enable != 0;
  return 0;
}

int tfhe_hip_timing_reset(tfhe_ctx* c) {
  if (!c) return fail(TFHE_HIP_EINVAL, "timing: null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  for (auto& s : c->sh)
    for (int w = 0; w < TIMING_SLOTS; w++) {
      for (auto e : s.ev[w]) s.ev_pool.push_back(e);
      s.ev[w].clear();
    }
  return 0;
}

int tfhe_hip_timing_stats(tfhe_ctx* c, int which, double* total_ms, int* launches) {
  if (!c || which < 0 || which >= TIMING_SLOTS || !total_ms || !launches) return fail(TFHE_HIP_EINVAL, "timing: bad arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  double tot = 0;
  int cnt = 0;
  for (auto& s : c->sh) {
    DeviceGuard g(s.device);
    auto& v = s.ev[which];
    for (size_t i = 0; i + 1 < v.size(); i += 2) {
      HIP_TRY(hipEventSynchronize(v[i + 1]));
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, v[i], v[i + 1]));
      tot += ms;
      cnt++;
    }
  }
  *total_ms = tot;
  *launches = cnt;
  return 0;
}

}  // extern "C"
