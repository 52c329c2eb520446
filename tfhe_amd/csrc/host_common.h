// host_common.h — plumbing shared by the C ABI translation units (api.cpp, pks_api.cpp, sns_api.cpp, sns_pks_api.cpp):
// error reporting, HIP call checking, the device guard, stream resolution, buffer growth.  Host code only.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/tfhe_hip.h"

// the library's thread-local error slot (owned by api.cpp)
int tfhe_hip_set_error(int code, const char* msg);
// Argument check of a list of compressed GLWEs (owned by pks_api.cpp; shared with tfhe_hip_decompress): EINVAL for
// invalid parameters, count > 0x7FFFFFFF or packed_words != the words of ceil(count / lwe_per_glwe) groups,
// EUNSUPPORTED for out_N above the unpack kernel's 4096.  `what` prefixes the message.
int tfhe_hip_pks_list_check(const tfhe_pks_params* pp, size_t packed_words, size_t count, const char* what);

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

int check_binary(const uint64_t* key, size_t len, const char* what) {
  for (size_t i = 0; i < len; i++)
    if (key[i] > 1) return fail(TFHE_HIP_EINVAL, "%s[%zu] is not binary", what, i);
  return 0;
}

}  // namespace
