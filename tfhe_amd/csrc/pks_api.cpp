// pks_api.cpp — C ABI of the packing keyswitch / compression (include/tfhe_hip.h, tfhe_hip_pks_*):
// key residency, workspace, chunked launches.  Kernels: pks.hip; host key material: client.cpp.
#include <hip/hip_runtime_api.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "../../include/tfhe_hip.h"
#include "client.h"
#include "host_common.h"
#include "pbs_kernels.h"

using tfhe::u32;
using tfhe::u64;

namespace {

bool pks_valid(const tfhe_pks_params* pp) {
  return pp && pp->in_dim > 0 && pp->in_dim % 16 == 0 && pp->out_k > 0 && pp->out_N >= 32 &&
         (pp->out_N & (pp->out_N - 1)) == 0 && ((pp->out_k + 1) * pp->out_N) % 64 == 0 && pp->base_log >= 2 &&
         pp->level > 0 && pp->base_log * pp->level < 64 && pp->base_log <= 31 && pp->lwe_per_glwe > 0 &&
         pp->lwe_per_glwe <= pp->out_N && pp->storage_log > 0 && pp->storage_log < 64 && pp->noise_log2 < 0 &&
         pp->noise_log2 > -64;
}

constexpr size_t PKS_T_BUDGET = 512ull << 20;  // T workspace per chunk of groups
constexpr uint32_t UNPACK_MAX_N = 4096;          // decompress.hip: one mask polynomial in 32 KB of LDS

}  // namespace

int tfhe_hip_pks_list_check(const tfhe_pks_params* pp, size_t packed_words, size_t count, const char* what) {
  if (!pks_valid(pp)) return fail(TFHE_HIP_EINVAL, "%s: invalid packing parameters", what);
  if (pp->out_N > UNPACK_MAX_N)
    return fail(TFHE_HIP_EUNSUPPORTED, "%s: out_N = %u, the unpack kernel covers out_N <= %u", what, pp->out_N, UNPACK_MAX_N);
  if (count > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "%s: too many ciphertexts", what);
  const size_t lpg = pp->lwe_per_glwe, rest = count % lpg;
  const size_t want = (count / lpg) * tfhe::client::pks_packed_words(*pp, (uint32_t)lpg) +
                      (rest ? tfhe::client::pks_packed_words(*pp, (uint32_t)rest) : 0);
  if (packed_words != want)
    return fail(TFHE_HIP_EINVAL, "%s: packed_words = %zu, %zu ciphertexts in groups of %zu take %zu", what, packed_words,
                count, lpg, want);
  return 0;
}

// d_A / d_A0 / d_A1 / d_T and the key are shared by every call: ordered across streams by the slot's ws_begin / ws_end
struct tfhe_pks_ctx : device_slot {
  tfhe_pks_params pp{};
  u64* d_pksk = nullptr;
  u64* d_corr = nullptr;
  bool key = false;
  u32* d_A = nullptr;
  u64* d_T = nullptr;
  size_t rows_cap = 0;  // LWEs the A / T workspaces hold
  // matrix-core path (default; TFHE_HIP_PKS_VALU=1 keeps the VALU GEMM): the key's byte planes and the
  // two digit-byte operands
  bool valu = false;
  void* d_planes = nullptr;
  void* d_A0 = nullptr;
  void* d_A1 = nullptr;
  std::mutex mu;
};

namespace {

int ensure_rows(tfhe_pks_ctx* c, size_t rows) {
  if (c->rows_cap >= rows) return 0;
  RC_TRY(ws_host_wait(*c));  // no launch may still use the old buffers
  for (void* p : {(void*)c->d_A, (void*)c->d_T, c->d_A0, c->d_A1}) (void)hipFree(p);
  c->d_A = nullptr;
  c->d_T = nullptr;
  c->d_A0 = c->d_A1 = nullptr;
  c->rows_cap = 0;
  const size_t K = (size_t)c->pp.in_dim * c->pp.level, Nc = (size_t)(c->pp.out_k + 1) * c->pp.out_N;
  if (c->valu) {
    HIP_TRY(hipMalloc(&c->d_A, rows * K * sizeof(u32)));
  } else {
    const size_t r = tfhe::pks_mfma_rows(rows);
    HIP_TRY(hipMalloc(&c->d_A0, r * K));
    HIP_TRY(hipMalloc(&c->d_A1, r * K));
  }
  HIP_TRY(hipMalloc(&c->d_T, rows * Nc * sizeof(u64)));
  c->rows_cap = rows;
  return 0;
}

// chunks of whole groups under the T budget (the caller orders the workspaces: ws_begin / ws_end)
int pack_device(tfhe_pks_ctx* c, const u64* d_lwes, size_t count, u64* d_out, hipStream_t s) {
  const tfhe_pks_params& p = c->pp;
  const size_t Nc = (size_t)(p.out_k + 1) * p.out_N, lpg = p.lwe_per_glwe;
  const size_t groups_per_chunk = std::max<size_t>(1, PKS_T_BUDGET / (lpg * Nc * 8));
  const size_t rows = std::min(count, groups_per_chunk * lpg);
  RC_TRY(ensure_rows(c, rows));
  for (size_t first = 0; first < count; first += rows) {
    const size_t n = std::min(rows, count - first);
    if (c->valu)
      HIP_TRY(tfhe::launch_pks_pack(d_lwes + first * (p.in_dim + 1), n, (int)p.in_dim, (int)p.base_log, (int)p.level,
                                    (int)p.out_k, (int)p.out_N, (int)lpg, c->d_pksk, c->d_corr, c->d_A, c->d_T,
                                    d_out + (first / lpg) * Nc, s));
    else
      HIP_TRY(tfhe::launch_pks_pack_mfma(d_lwes + first * (p.in_dim + 1), n, (int)p.in_dim, (int)p.base_log,
                                         (int)p.level, (int)p.out_k, (int)p.out_N, (int)lpg, c->d_planes, c->d_A0,
                                         c->d_A1, c->d_T, d_out + (first / lpg) * Nc, s));
  }
  return 0;
}

}  // namespace

extern "C" {

int tfhe_hip_pks_params_preset(int preset, tfhe_pks_params* o) {
  if (!o) return fail(TFHE_HIP_EINVAL, "pks_params_preset: null out");
  if (preset != TFHE_HIP_PKS_PRESET_ML2048) return fail(TFHE_HIP_EINVAL, "unknown packing preset %d", preset);
  *o = tfhe_pks_params{2048, 1, 2048, 14, 2, 2048, 26, -48};
  return 0;
}

size_t tfhe_hip_pksk_len(const tfhe_pks_params* pp) { return pp ? tfhe::client::pksk_len(*pp) : 0; }

int tfhe_hip_pks_keygen_k(const tfhe_pks_params* pp, const tfhe_rng_key* rk, const uint64_t* in_key,
                          uint64_t* out_key, uint64_t* pksk) {
  if (!pks_valid(pp) || !rk || !in_key || !out_key) return fail(TFHE_HIP_EINVAL, "pks_keygen: bad arguments");
  RC_TRY(check_binary(in_key, pp->in_dim, "pks_keygen: in_key"));
  tfhe::client::pks_keygen(*pp, *rk, in_key, out_key, pksk);
  return 0;
}

int tfhe_hip_pks_keygen(const tfhe_pks_params* pp, uint64_t seed, const uint64_t* in_key, uint64_t* out_key,
                        uint64_t* pksk) {
  const tfhe_rng_key rk = tfhe::client::rng_key_from_seed(seed);
  return tfhe_hip_pks_keygen_k(pp, &rk, in_key, out_key, pksk);
}

int tfhe_hip_pks_create(const tfhe_pks_params* pp, int device, tfhe_pks_ctx** out) {
  if (!out) return fail(TFHE_HIP_EINVAL, "pks_create: null out");
  *out = nullptr;
  if (!pks_valid(pp)) return fail(TFHE_HIP_EINVAL, "pks_create: invalid parameters");
  tfhe_pks_ctx* c = new tfhe_pks_ctx();
  c->pp = *pp;
  {
    const char* e = getenv("TFHE_HIP_PKS_VALU");
    // the matrix-core GEMM needs two int8 bytes per digit (base <= 2^15: a balanced digit reaches +2^(B-1), and
    // +2^15 would need a high byte of +128), the key planes' level limit (<= 8) and 64-deep k steps
    c->valu = (e && e[0] == '1') || pp->base_log > 15 || pp->level > 8 || (pp->in_dim * pp->level) % 64 != 0;
  }
  const int rc = slot_open(*c, device, "pks_create", "hipStreamCreate failed");
  if (rc) {
    tfhe_hip_pks_destroy(c);
    return rc;
  }
  *out = c;
  return 0;
}

void tfhe_hip_pks_destroy(tfhe_pks_ctx* c) {
  if (!c) return;
  slot_close(*c, {c->d_pksk, c->d_corr, c->d_A, c->d_T, c->d_planes, c->d_A0, c->d_A1});
  delete c;
}

int tfhe_hip_pks_load_key(tfhe_pks_ctx* c, const uint64_t* pksk, size_t len) {
  if (!c || !pksk) return fail(TFHE_HIP_EINVAL, "pks_load_key: null argument");
  if (len != tfhe::client::pksk_len(c->pp))
    return fail(TFHE_HIP_EINVAL, "pks_load_key: length %zu, expected %zu", len, tfhe::client::pksk_len(c->pp));
  const size_t Nc = (size_t)(c->pp.out_k + 1) * c->pp.out_N;
  return side_key_load(
      c,
      [&]() -> int {
        if (!c->d_pksk) HIP_TRY(hipMalloc(&c->d_pksk, len * 8));
        if (!c->d_corr) HIP_TRY(hipMalloc(&c->d_corr, Nc * 8));
        if (!c->valu && !c->d_planes)
          HIP_TRY(hipMalloc(&c->d_planes, tfhe::ks_planes_bytes((int)c->pp.in_dim, (int)c->pp.level, (int)Nc - 1)));
        return 0;
      },
      [&]() -> int {
        HIP_TRY(hipMemcpyAsync(c->d_pksk, pksk, len * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(tfhe::launch_pks_corr(c->d_pksk, (int)(c->pp.in_dim * c->pp.level), (int)Nc, (int)c->pp.base_log,
                                      c->d_corr, c->stream));
        if (!c->valu)  // balanced byte planes of the key (ks_mfma.hip's recoding, Nc columns)
          HIP_TRY(tfhe::launch_ksk_planes(c->d_pksk, (int)c->pp.in_dim, (int)c->pp.level, (int)Nc - 1, c->d_planes,
                                          c->stream));
        return 0;
      });
}

int tfhe_hip_pks_pack_async(tfhe_pks_ctx* c, const uint64_t* d_lwes, size_t count, uint64_t* d_glwes, void* stream) {
  if (!c) return fail(TFHE_HIP_EINVAL, "pks_pack: null ctx");
  if (!c->key) return fail(TFHE_HIP_ENOKEYS, "pks_pack: key not loaded");
  if (count == 0) return 0;
  if (!d_lwes || !d_glwes) return fail(TFHE_HIP_EINVAL, "pks_pack: null buffer");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  hipStream_t st = resolve_stream(stream, c->stream);
  RC_TRY(ws_begin(*c, st));
  RC_TRY(pack_device(c, d_lwes, count, d_glwes, st));
  return ws_end(*c, st);
}

int tfhe_hip_pks_pack(tfhe_pks_ctx* c, const uint64_t* lwes, size_t count, uint64_t* glwes) {
  if (!c) return fail(TFHE_HIP_EINVAL, "pks_pack: null ctx");
  if (!c->key) return fail(TFHE_HIP_ENOKEYS, "pks_pack: key not loaded");
  if (count == 0) return 0;
  if (!lwes || !glwes) return fail(TFHE_HIP_EINVAL, "pks_pack: null buffer");
  if (count > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "pks_pack: too many ciphertexts");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const tfhe_pks_params& p = c->pp;
  const size_t in_bytes = count * (p.in_dim + 1) * 8, groups = (count + p.lwe_per_glwe - 1) / p.lwe_per_glwe;
  const size_t out_bytes = groups * (p.out_k + 1) * p.out_N * 8;
  return staged_run(*c, {{lwes, in_bytes}}, out_bytes, {{glwes, 1, out_bytes}},
                    [&](tfhe_pks_ctx& s, std::vector<void*>& d) {
                      return pack_device(&s, (const u64*)d[0], count, (u64*)d[1], s.stream);
                    });
}

size_t tfhe_hip_pks_packed_words(const tfhe_pks_params* pp, uint32_t bodies) {
  return pp ? tfhe::client::pks_packed_words(*pp, bodies) : 0;
}

int tfhe_hip_pks_compress(const tfhe_pks_params* pp, const uint64_t* glwe, uint32_t bodies, uint64_t* packed) {
  if (!pks_valid(pp) || !glwe || !packed || bodies > pp->out_N) return fail(TFHE_HIP_EINVAL, "pks_compress: bad arguments");
  tfhe::client::pks_compress(*pp, glwe, bodies, packed);
  return 0;
}

int tfhe_hip_pks_extract(const tfhe_pks_params* pp, const uint64_t* packed, uint32_t bodies, uint64_t* glwe) {
  if (!pks_valid(pp) || !glwe || !packed || bodies > pp->out_N) return fail(TFHE_HIP_EINVAL, "pks_extract: bad arguments");
  tfhe::client::pks_extract(*pp, packed, bodies, glwe);
  return 0;
}

static hipError_t unpack_extract_device(const tfhe_pks_params& p, const u64* d_packed, size_t count, u64* d_out,
                                        hipStream_t s) {
  return tfhe::launch_unpack_extract(d_packed, count, (int)p.out_k, (int)p.out_N, (int)p.lwe_per_glwe,
                                     (int)p.storage_log, d_out, s);
}

int tfhe_hip_pks_unpack_extract_async(tfhe_pks_ctx* c, const uint64_t* d_packed, size_t packed_words, size_t count,
                                      uint64_t* d_lwes_out, void* stream) {
  if (!c) return fail(TFHE_HIP_EINVAL, "pks_unpack_extract: null ctx");
  RC_TRY(tfhe_hip_pks_list_check(&c->pp, packed_words, count, "pks_unpack_extract"));
  if (count == 0) return 0;
  if (!d_packed || !d_lwes_out) return fail(TFHE_HIP_EINVAL, "pks_unpack_extract: null buffer");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HIP_TRY(unpack_extract_device(c->pp, d_packed, count, d_lwes_out, resolve_stream(stream, c->stream)));
  return 0;
}

int tfhe_hip_pks_unpack_extract(tfhe_pks_ctx* c, const uint64_t* packed, size_t packed_words, size_t count,
                                uint64_t* lwes_out) {
  if (!c) return fail(TFHE_HIP_EINVAL, "pks_unpack_extract: null ctx");
  RC_TRY(tfhe_hip_pks_list_check(&c->pp, packed_words, count, "pks_unpack_extract"));
  if (count == 0) return 0;
  if (!packed || !lwes_out) return fail(TFHE_HIP_EINVAL, "pks_unpack_extract: null buffer");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const size_t out_bytes = count * ((size_t)c->pp.out_k * c->pp.out_N + 1) * 8;
  return staged_run(*c, {{packed, packed_words * 8}}, out_bytes, {{lwes_out, 1, out_bytes}},
                    [&](tfhe_pks_ctx& s, std::vector<void*>& d) -> int {
                      HIP_TRY(unpack_extract_device(s.pp, (const u64*)d[0], count, (u64*)d[1], s.stream));
                      return 0;
                    });
}

int tfhe_hip_glwe_phase(uint32_t k, uint32_t N, const uint64_t* key, const uint64_t* glwe, uint64_t* out) {
  if (!k || !N || !key || !glwe || !out) return fail(TFHE_HIP_EINVAL, "glwe_phase: bad arguments");
  tfhe::client::glwe_phase_native(k, N, key, glwe, out);
  return 0;
}

}  // extern "C"
