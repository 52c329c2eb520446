// matmul_api.cpp — C ABI of the encrypted matrix x clear matrix product (include/tfhe_hip.h, tfhe_hip_matmul_*):
// parameter checks, the resident clear matrices, the device context.  Kernels: matmul.hip; client and CPU side:
// seeded.cpp.
#include <hip/hip_runtime_api.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../include/tfhe_hip.h"
#include "client.h"
#include "host_common.h"
#include "pbs_kernels.h"

using tfhe::u32;
using tfhe::u64;

namespace {

bool matmul_valid(const tfhe_matmul_params* mp) {
  return mp && mp->N >= 64 && mp->N <= 4096 && (mp->N & (mp->N - 1)) == 0 && mp->bits_reserved >= 1 &&
         mp->bits_reserved <= 63 && mp->in_storage_log >= 1 && mp->in_storage_log <= 64 && mp->noise_log2 < 0 &&
         mp->noise_log2 > -64;
}

constexpr size_t MM_MAX_DIM = 1u << 22;  // K and C: Cpad / 64 stays a grid dimension, indices stay in an int

}  // namespace

// the resident matrices and the input / output buffers of the calls belong to the callers; the slot's event orders the
// calls so that destroy (of the ctx or of a matrix) can wait for the ones in flight
struct tfhe_matmul_ctx : device_slot {
  tfhe_matmul_params mp{};
  std::mutex mu;
};

struct tfhe_matmul_matrix {
  tfhe_matmul_ctx* ctx = nullptr;
  u32* d_w = nullptr;  // Kb * N x Cpad, value + 2^31
  size_t K = 0, C = 0, Kb = 0, Cpad = 0;
};

namespace {

int expand_device(tfhe_matmul_ctx* c, const u64* d_seeds, const u64* d_packed, size_t G, u64* d_glwes, hipStream_t s) {
  HIP_TRY(tfhe::launch_matmul_expand(d_seeds, d_packed, G, (int)c->mp.N, (int)c->mp.in_storage_log, d_glwes, s));
  return 0;
}

int dot_device(tfhe_matmul_ctx* c, const tfhe_matmul_matrix* m, const u64* d_glwes, size_t R, size_t col_stride,
               u64* d_out, hipStream_t s) {
  HIP_TRY(tfhe::launch_matmul_dot(d_glwes, m->d_w, R, (int)c->mp.N, (int)m->Kb, (int)m->Cpad, (int)m->C, col_stride, d_out, s));
  return 0;
}

int dot_check(tfhe_matmul_ctx* c, const tfhe_matmul_matrix* m, size_t R, size_t col_stride) {
  if (!c || !m) return fail(TFHE_HIP_EINVAL, "matmul_dot: null ctx or matrix");
  if (m->ctx != c) return fail(TFHE_HIP_EINVAL, "matmul_dot: the matrix belongs to another ctx");
  if (col_stride < m->C) return fail(TFHE_HIP_EINVAL, "matmul_dot: col_stride %zu < C = %zu", col_stride, m->C);
  if (R > 0x7FFFFFFF || col_stride > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "matmul_dot: too many rows or columns");
  return 0;
}

}  // namespace

extern "C" {

int tfhe_hip_matmul_params_preset(int preset, tfhe_matmul_params* o) {
  if (!o) return fail(TFHE_HIP_EINVAL, "matmul_params_preset: null out");
  if (preset != TFHE_HIP_MATMUL_PRESET_ML2048) return fail(TFHE_HIP_EINVAL, "unknown matmul preset %d", preset);
  *o = tfhe_matmul_params{2048, 27, 39, -48};
  return 0;
}

size_t tfhe_hip_matmul_body_words(const tfhe_matmul_params* mp) {
  return matmul_valid(mp) ? tfhe::seeded::matmul_body_words(*mp) : 0;
}

int tfhe_hip_matmul_keygen_k(const tfhe_matmul_params* mp, const tfhe_rng_key* rk, uint64_t* glwe_key) {
  if (!matmul_valid(mp) || !rk || !glwe_key) return fail(TFHE_HIP_EINVAL, "matmul_keygen: bad arguments");
  tfhe::client::binary_key(*rk, 7, mp->N, glwe_key);
  return 0;
}

int tfhe_hip_matmul_encrypt_k(const tfhe_matmul_params* mp, const uint64_t* glwe_key, const tfhe_rng_key* rk,
                              uint64_t stream0, const uint64_t* seeds, const int64_t* values, size_t G,
                              uint64_t* packed_out) {
  if (!matmul_valid(mp) || !glwe_key || !rk || (G && (!seeds || !values || !packed_out)))
    return fail(TFHE_HIP_EINVAL, "matmul_encrypt: bad arguments");
  RC_TRY(check_binary(glwe_key, mp->N, "matmul_encrypt: glwe_key"));
  tfhe::seeded::matmul_encrypt(*mp, glwe_key, *rk, stream0, seeds, values, G, packed_out);
  return 0;
}

int tfhe_hip_matmul_expand_host(const tfhe_matmul_params* mp, const uint64_t* seeds, const uint64_t* packed, size_t G,
                                uint64_t* glwes_out) {
  if (!matmul_valid(mp) || (G && (!seeds || !packed || !glwes_out)))
    return fail(TFHE_HIP_EINVAL, "matmul_expand_host: bad arguments");
  tfhe::seeded::matmul_expand(*mp, seeds, packed, G, glwes_out);
  return 0;
}

int tfhe_hip_matmul_dot_host(const tfhe_matmul_params* mp, const int32_t* w, size_t K, size_t C, const uint64_t* glwes,
                             size_t R, size_t col_stride, uint64_t* lwes_out) {
  if (!matmul_valid(mp) || !w || K == 0 || C == 0 || K > MM_MAX_DIM || C > MM_MAX_DIM || col_stride < C ||
      (R && (!glwes || !lwes_out)))
    return fail(TFHE_HIP_EINVAL, "matmul_dot_host: bad arguments");
  tfhe::seeded::matmul_dot(*mp, w, K, C, glwes, R, col_stride, lwes_out);
  return 0;
}

int tfhe_hip_matmul_decode(const tfhe_matmul_params* mp, const uint64_t* phases, size_t count, int64_t* out) {
  if (!matmul_valid(mp) || (count && (!phases || !out))) return fail(TFHE_HIP_EINVAL, "matmul_decode: bad arguments");
  tfhe::seeded::matmul_decode(*mp, phases, count, out);
  return 0;
}

int tfhe_hip_matmul_create(const tfhe_matmul_params* mp, int device, tfhe_matmul_ctx** out) {
  if (!out) return fail(TFHE_HIP_EINVAL, "matmul_create: null out");
  *out = nullptr;
  if (!matmul_valid(mp)) return fail(TFHE_HIP_EINVAL, "matmul_create: invalid parameters");
  tfhe_matmul_ctx* c = new tfhe_matmul_ctx();
  c->mp = *mp;
  const int rc = slot_open(*c, device, "matmul_create", "hipStreamCreate failed");
  if (rc) {
    tfhe_hip_matmul_destroy(c);
    return rc;
  }
  *out = c;
  return 0;
}

void tfhe_hip_matmul_destroy(tfhe_matmul_ctx* c) {
  if (!c) return;
  slot_close(*c, {});
  delete c;
}

int tfhe_hip_matmul_matrix_create(tfhe_matmul_ctx* c, const int32_t* w, size_t K, size_t C, tfhe_matmul_matrix** out) {
  if (!out) return fail(TFHE_HIP_EINVAL, "matmul_matrix_create: null out");
  *out = nullptr;
  if (!c || !w) return fail(TFHE_HIP_EINVAL, "matmul_matrix_create: null argument");
  if (K == 0 || C == 0 || K > MM_MAX_DIM || C > MM_MAX_DIM)
    return fail(TFHE_HIP_EINVAL, "matmul_matrix_create: K = %zu, C = %zu, both must be in 1 .. %zu", K, C, MM_MAX_DIM);
  const size_t N = c->mp.N, Kb = (K + N - 1) / N, Cpad = (C + 63) / 64 * 64;
  // value + 2^31; the padding is the value zero
  std::vector<u32> h;
  try {
    h.assign(Kb * N * Cpad, 0x80000000u);
  } catch (const std::bad_alloc&) {
    return fail(TFHE_HIP_ENOMEM, "matmul_matrix_create: host staging of %zu x %zu words", Kb * N, Cpad);
  }
  for (size_t t = 0; t < K; t++)
    for (size_t j = 0; j < C; j++) h[t * Cpad + j] = (u32)w[t * C + j] ^ 0x80000000u;
  tfhe_matmul_matrix* m = new tfhe_matmul_matrix();
  m->ctx = c;
  m->K = K;
  m->C = C;
  m->Kb = Kb;
  m->Cpad = Cpad;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  auto upload = [&]() -> int {
    HIP_TRY(hipMalloc(&m->d_w, h.size() * sizeof(u32)));
    HIP_TRY(hipMemcpyAsync(m->d_w, h.data(), h.size() * sizeof(u32), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
  };
  const int rc = upload();
  if (rc) {
    (void)hipFree(m->d_w);
    delete m;
    return rc;
  }
  *out = m;
  return 0;
}

void tfhe_hip_matmul_matrix_destroy(tfhe_matmul_matrix* m) {
  if (!m) return;
  {
    std::lock_guard<std::mutex> lk(m->ctx->mu);
    DeviceGuard g(m->ctx->device);
    (void)ws_host_wait(*m->ctx);  // a dot in flight on a caller's stream still reads the matrix
    (void)hipFree(m->d_w);
  }
  delete m;
}

int tfhe_hip_matmul_expand_async(tfhe_matmul_ctx* c, const uint64_t* d_seeds, const uint64_t* d_packed, size_t G,
                                 uint64_t* d_glwes, void* stream) {
  if (!c) return fail(TFHE_HIP_EINVAL, "matmul_expand: null ctx");
  if (G == 0) return 0;
  if (!d_seeds || !d_packed || !d_glwes) return fail(TFHE_HIP_EINVAL, "matmul_expand: null buffer");
  if (G > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "matmul_expand: too many ciphertexts");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  hipStream_t st = resolve_stream(stream, c->stream);
  RC_TRY(ws_begin(*c, st));
  RC_TRY(expand_device(c, d_seeds, d_packed, G, d_glwes, st));
  return ws_end(*c, st);
}

int tfhe_hip_matmul_expand(tfhe_matmul_ctx* c, const uint64_t* seeds, const uint64_t* packed, size_t G,
                           uint64_t* glwes_out) {
  if (!c) return fail(TFHE_HIP_EINVAL, "matmul_expand: null ctx");
  if (G == 0) return 0;
  if (!seeds || !packed || !glwes_out) return fail(TFHE_HIP_EINVAL, "matmul_expand: null buffer");
  if (G > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "matmul_expand: too many ciphertexts");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const size_t out_bytes = G * 2 * (size_t)c->mp.N * 8;
  return staged_run(*c, {{seeds, G * 16}, {packed, G * tfhe::seeded::matmul_body_words(c->mp) * 8}}, out_bytes,
                    {{glwes_out, 2, out_bytes}}, [&](tfhe_matmul_ctx& s, std::vector<void*>& d) {
                      return expand_device(&s, (const u64*)d[0], (const u64*)d[1], G, (u64*)d[2], s.stream);
                    });
}

int tfhe_hip_matmul_dot_async(tfhe_matmul_ctx* c, const tfhe_matmul_matrix* m, const uint64_t* d_glwes, size_t R,
                              size_t col_stride, uint64_t* d_lwes_out, void* stream) {
  RC_TRY(dot_check(c, m, R, col_stride));
  if (R == 0) return 0;
  if (!d_glwes || !d_lwes_out) return fail(TFHE_HIP_EINVAL, "matmul_dot: null buffer");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  hipStream_t st = resolve_stream(stream, c->stream);
  RC_TRY(ws_begin(*c, st));
  RC_TRY(dot_device(c, m, d_glwes, R, col_stride, d_lwes_out, st));
  return ws_end(*c, st);
}

int tfhe_hip_matmul_dot(tfhe_matmul_ctx* c, const tfhe_matmul_matrix* m, const uint64_t* glwes, size_t R,
                        size_t col_stride, uint64_t* lwes_out) {
  RC_TRY(dot_check(c, m, R, col_stride));
  if (R == 0) return 0;
  if (!glwes || !lwes_out) return fail(TFHE_HIP_EINVAL, "matmul_dot: null buffer");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const size_t N = c->mp.N, in_bytes = R * m->Kb * 2 * N * 8, out_bytes = R * col_stride * (N + 1) * 8;
  // the output goes up first: the LWEs C .. col_stride - 1 of a row keep the caller's words
  return staged_run(*c, {{glwes, in_bytes}, {lwes_out, out_bytes}}, 0, {{lwes_out, 1, out_bytes}},
                    [&](tfhe_matmul_ctx& s, std::vector<void*>& d) {
                      return dot_device(&s, m, (const u64*)d[0], R, col_stride, (u64*)d[1], s.stream);
                    });
}

}  // extern "C"
