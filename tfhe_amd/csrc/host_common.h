// host_common.h — plumbing shared by the C ABI translation units (api.cpp, pks_api.cpp, sns_api.cpp, sns_pks_api.cpp,
// matmul_api.cpp): error reporting, HIP call checking, the device guard, stream resolution, buffer growth, the device
// slot (the stream, the cross-stream workspace ordering and the host-call staging of every device context), and the
// key-load tools: the load skeleton of the side contexts (side_key_load) and what the seeded loads of all contexts
// share (round_keys_of, call_buffers, phase_timer, seeded_ms_read, guarded_expand, env_positive).  Host code only.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/tfhe_hip.h"
#include "client.h"
#include "pbs_kernels.h"

// the library's thread-local error slot (owned by api.cpp)
int tfhe_hip_set_error(int code, const char* msg);
// Argument check of a list of compressed GLWEs (owned by pks_api.cpp; shared with tfhe_hip_decompress): EINVAL for
// invalid parameters, count > 0x7FFFFFFF or packed_words != the words of ceil(count / lwe_per_glwe) groups,
// EUNSUPPORTED for out_N above the unpack kernel's 4096.  `what` prefixes the message.
int tfhe_hip_pks_list_check(const tfhe_pks_params* pp, size_t packed_words, size_t count, const char* what);

// What every device context (an engine shard, tfhe_pks_ctx, tfhe_sns_ctx, tfhe_sns_pks_ctx) derives from: one device
// ordinal, its own stream, the ordering state of the workspaces that all its calls share, and the staging buffer of
// its host-buffer calls.
struct device_slot {
  int device = 0;
  hipStream_t stream = nullptr;
  // workspaces and resident keys: every user waits for `ws_free` (the previous user's completion) on its own stream
  hipEvent_t ws_free = nullptr;
  hipStream_t ws_last = nullptr;
  bool ws_used = false;
  void* d_stage = nullptr;
  size_t stage_cap = 0;  // bytes
};

namespace {

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return tfhe_hip_set_error(code, buf);
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return fail(_e == hipErrorOutOfMemory ? TFHE_HIP_ENOMEM : TFHE_HIP_EDEVICE, "%s: %s (%s:%d)", #expr, \
                  hipGetErrorString(_e), __FILE__, __LINE__);                                  \
  } while (0)

#define RC_TRY(expr)      \
  do {                    \
    int _rc = (expr);     \
    if (_rc) return _rc;  \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// the stream argument of the *_async calls: TFHE_HIP_NULL_STREAM = the legacy null stream, NULL = the ctx's own
hipStream_t resolve_stream(void* user, hipStream_t own) {
  return user == TFHE_HIP_NULL_STREAM ? (hipStream_t)0 : user ? (hipStream_t)user : own;
}

// Make *p hold at least `bytes` (free, then allocate: the contents are not kept).  The caller has made sure
// that nothing on the device still uses the old buffer.
int grow_device_buffer(void** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return 0;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  HIP_TRY(hipMalloc(p, bytes));
  *cap = bytes;
  return 0;
}

// EINVAL unless `device` is an ordinal of this process (`list_index` >= 0: the entry of the caller's list it came from)
int device_ordinal_check(const char* what, int device, int list_index = -1) {
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device >= 0 && device < ndev) return 0;
  if (list_index < 0) return fail(TFHE_HIP_EINVAL, "%s: device %d of %d", what, device, ndev);
  return fail(TFHE_HIP_EINVAL, "%s: device %d of %d (devices[%d])", what, device, ndev, list_index);
}

// the slot's non-blocking stream and its ordering event (s.device is set and current)
int slot_streams(device_slot& s) {
  HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&s.ws_free, hipEventDisableTiming));
  return 0;
}

// Open a side context's slot: the ordinal check under the caller's `what`, then stream and event (EDEVICE,
// "<what>: <setup_failed>").  After a failure slot_close still applies.
int slot_open(device_slot& s, int device, const char* what, const char* setup_failed) {
  RC_TRY(device_ordinal_check(what, device));
  s.device = device;
  DeviceGuard g(device);
  if (slot_streams(s)) return fail(TFHE_HIP_EDEVICE, "%s: %s", what, setup_failed);
  return 0;
}

// Close a slot, half-opened ones included: wait for its stream and for the last user of the workspaces (a caller's
// stream may still run on them), then free `bufs` and the staging buffer and destroy event and stream.
void slot_close(device_slot& s, std::initializer_list<void*> bufs) {
  DeviceGuard g(s.device);
  if (s.stream) (void)hipStreamSynchronize(s.stream);
  if (s.ws_used) (void)hipEventSynchronize(s.ws_free);
  for (void* p : bufs) (void)hipFree(p);
  (void)hipFree(s.d_stage);
  if (s.ws_free) (void)hipEventDestroy(s.ws_free);
  if (s.stream) (void)hipStreamDestroy(s.stream);
}

// Workspace ordering across streams (the *_async calls may be given any stream): the stream that uses a slot's
// workspaces or resident keys next waits for the event recorded after the previous use; the host waits for it before
// it frees or rewrites a buffer that enqueued kernels may still read.  The entry points order: ws_begin before the
// *_device worker, ws_end after it; the workers only call ws_grow / ws_host_wait where they regrow or rewrite.
int ws_begin(device_slot& s, hipStream_t st) {
  if (s.ws_used && s.ws_last != st) HIP_TRY(hipStreamWaitEvent(st, s.ws_free, 0));
  return 0;
}
int ws_end(device_slot& s, hipStream_t st) {
  HIP_TRY(hipEventRecord(s.ws_free, st));
  s.ws_last = st;
  s.ws_used = true;
  return 0;
}
int ws_host_wait(device_slot& s) {
  if (s.ws_used) HIP_TRY(hipEventSynchronize(s.ws_free));
  return 0;
}
int ws_grow(device_slot& s, void** ptr, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return 0;
  RC_TRY(ws_host_wait(s));  // no launch may still read the old buffer
  return grow_device_buffer(ptr, cap, bytes);
}

using staged_in = std::initializer_list<std::pair<const void*, size_t>>;  // (host pointer or null, bytes)

// Stage host buffers into the slot's staging allocation (on the slot's stream).  Returns device pointers
// in order, plus one for `extra_out_bytes` of output.
int stage(device_slot& s, staged_in in, std::vector<void*>& dptr, size_t extra_out_bytes) {
  size_t total = 0;
  std::vector<size_t> off;
  for (auto& x : in) {
    off.push_back(total);
    total += (x.second + 255) & ~(size_t)255;
  }
  const size_t out_off = total;
  total += (extra_out_bytes + 255) & ~(size_t)255;
  RC_TRY(ws_grow(s, &s.d_stage, &s.stage_cap, total ? total : 256));
  size_t i = 0;
  dptr.clear();
  for (auto& x : in) {
    void* d = (char*)s.d_stage + off[i++];
    if (x.first && x.second) HIP_TRY(hipMemcpyAsync(d, x.first, x.second, hipMemcpyHostToDevice, s.stream));
    dptr.push_back(x.first ? d : nullptr);
  }
  dptr.push_back((char*)s.d_stage + out_off);
  return 0;
}

struct copy_back {  // after the launch: host dst (skipped when null) <- staged pointer d[src], bytes
  void* dst;
  size_t src, bytes;
};

// One host-buffer call on a slot's own stream (caller holds the context's lock and has set the slot's device): order
// the workspaces after their previous user, stage `in` plus out_bytes of output, launch(s, d) on the staged pointers,
// copy `back` to the host, mark the workspaces used and wait.  S: the context type that derives from device_slot.
template <class S, class F>
int staged_run(S& s, staged_in in, size_t out_bytes, std::initializer_list<copy_back> back, F&& launch) {
  RC_TRY(ws_begin(s, s.stream));
  std::vector<void*> d;
  RC_TRY(stage(s, in, d, out_bytes));
  RC_TRY(launch(s, d));
  for (auto& b : back)
    if (b.dst) HIP_TRY(hipMemcpyAsync(b.dst, d[b.src], b.bytes, hipMemcpyDeviceToHost, s.stream));
  RC_TRY(ws_end(s, s.stream));
  HIP_TRY(hipStreamSynchronize(s.stream));
  return 0;
}

// a tuning variable that counts something: its value where it is a positive number, `dflt` otherwise
size_t env_positive(const char* name, size_t dflt) {
  const char* e = getenv(name);
  const long x = e ? atol(e) : 0;
  return x > 0 ? (size_t)x : dflt;
}

// the AES key schedule of a compression seed, once per seed on the host: the 44 words travel as a launch argument
tfhe::seeded_round_keys round_keys_of(const uint64_t seed[2]) {
  tfhe::seeded_round_keys rk;
  tfhe::seeded::aes_round_keys(seed, rk.w);
  return rk;
}

// Device buffers that live for one call (the uploaded bodies of a seeded load, the output of an expand aid), on any
// devices: each is freed under a guard for its own device on every path out of the scope.
struct call_buffers {
  std::vector<std::pair<int, void*>> v;  // (device, pointer)
  template <class T>
  int alloc(int device, size_t bytes, T** out) {
    DeviceGuard g(device);
    *out = nullptr;
    HIP_TRY(hipMalloc(out, bytes ? bytes : 8));
    v.emplace_back(device, *out);
    return 0;
  }
  ~call_buffers() {
    for (auto& x : v) {
      DeviceGuard g(x.first);
      (void)hipFree(x.second);
    }
  }
};

// Device-time split of a seeded load on one slot's stream: tick(phase) books the time since the previous tick under
// `phase` (tick(-1) only opens an interval); totals() waits for the last tick.  Without a slot (a load from another
// source) tick() does nothing.  Events are destroyed with the scope.
struct phase_timer {
  const device_slot* s;
  std::vector<std::pair<hipEvent_t, int>> ev;
  explicit phase_timer(const device_slot* slot) : s(slot) {}
  int tick(int phase) {
    if (!s) return 0;
    DeviceGuard g(s->device);
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    ev.emplace_back(e, phase);
    HIP_TRY(hipEventRecord(e, s->stream));
    return 0;
  }
  int totals(double* ms, int phases) {
    for (int i = 0; i < phases; i++) ms[i] = 0;
    if (ev.empty()) return 0;
    DeviceGuard g(s->device);
    HIP_TRY(hipEventSynchronize(ev.back().first));
    for (size_t i = 1; i < ev.size(); i++) {
      if (ev[i].second < 0 || ev[i].second >= phases) continue;
      float t = 0;
      HIP_TRY(hipEventElapsedTime(&t, ev[i - 1].first, ev[i].first));
      ms[ev[i].second] += t;
    }
    return 0;
  }
  ~phase_timer() {
    for (auto& x : ev) (void)hipEventDestroy(x.first);
  }
};

// the *_seeded_load_stats read-out: a context's seeded_ms (upload, expansion, conversion or correction of its last
// seeded load, device ms) into the out-pointers that are set
int seeded_ms_read(const double ms[3], double* upload_ms, double* expand_ms, double* third_ms) {
  if (upload_ms) *upload_ms = ms[0];
  if (expand_ms) *expand_ms = ms[1];
  if (third_ms) *third_ms = ms[2];
  return 0;
}

// The key load of a side context (C: tfhe_pks_ctx, tfhe_sns_ctx, tfhe_sns_pks_ctx), after the caller's argument and
// length checks.  prepare() holds every allocation and every ws_grow, fill() enqueues the copies and kernels on
// c->stream.  Every refusal and every allocation comes before the resident key is touched: a refused load, or one that
// cannot allocate, leaves the previous key usable; from fill() on the ctx has no key until the load has completed.
template <class C, class P, class F>
int side_key_load(C* c, P&& prepare, F&& fill) {
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  RC_TRY(ws_host_wait(*c));  // a call in flight on a caller's stream still reads the resident key
  RC_TRY(prepare());
  c->key = false;
  RC_TRY(fill());
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->key = true;
  return 0;
}

// The test aid behind the *_seeded_expand_* entry points (the caller holds the context's lock and has set the slot's
// device): a buffer of body_bytes and a fresh output of out_len + TFHE_HIP_SEEDED_GUARD_WORDS words filled with 0xA5
// bytes, step(d_bodies, d_out) enqueues the uploads and the loader's launches on the slot's stream, and all of the
// output is copied back, guard words included.
template <class F>
int guarded_expand(device_slot& s, size_t body_bytes, size_t out_len, uint64_t* out_host, F&& step) {
  call_buffers tmp;
  uint64_t *d_bodies = nullptr, *d_out = nullptr;
  const size_t out_bytes = (out_len + TFHE_HIP_SEEDED_GUARD_WORDS) * 8;
  RC_TRY(tmp.alloc(s.device, body_bytes, &d_bodies));
  RC_TRY(tmp.alloc(s.device, out_bytes, &d_out));
  HIP_TRY(hipMemsetAsync(d_out, 0xA5, out_bytes, s.stream));
  RC_TRY(step(d_bodies, d_out));
  HIP_TRY(hipMemcpyAsync(out_host, d_out, out_bytes, hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(hipStreamSynchronize(s.stream));
  return 0;
}

int check_binary(const uint64_t* key, size_t len, const char* what) {
  for (size_t i = 0; i < len; i++)
    if (key[i] > 1) return fail(TFHE_HIP_EINVAL, "%s[%zu] is not binary", what, i);
  return 0;
}

}  // namespace
