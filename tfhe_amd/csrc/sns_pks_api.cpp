// sns_pks_api.cpp — C ABI of the compression of squashed ciphertexts (include/tfhe_hip.h, tfhe_hip_sns_pks_*):
// key residency, workspaces, chunked launches.  Kernels: sns_pks.hip; host key material and the CPU pack: client.cpp.
#include <hip/hip_runtime_api.h>
#include <string.h>

#include <algorithm>
#include <mutex>

#include "../../include/tfhe_hip.h"
#include "client.h"
#include "host_common.h"
#include "pbs_kernels.h"

using tfhe::u64;

namespace {

bool spk_valid(const tfhe_sns_pks_params* pp) {
  return pp && pp->in_dim > 0 && pp->in_dim % 16 == 0 && pp->out_k > 0 && pp->out_N >= 32 &&
         (pp->out_N & (pp->out_N - 1)) == 0 && ((uint64_t)(pp->out_k + 1) * pp->out_N) % 64 == 0 &&
         pp->base_log >= 2 && pp->base_log <= 63 && pp->level >= 1 && (uint64_t)pp->base_log * pp->level <= 127 &&
         pp->lwe_per_glwe >= 1 && pp->lwe_per_glwe <= pp->out_N && pp->storage_log >= 2 && pp->storage_log <= 128 &&
         pp->noise_log2 < 0 && pp->noise_log2 > -64;
}

constexpr size_t SPK_T_BUDGET = 512ull << 20;    // T workspace per chunk of groups
constexpr size_t SPK_MAX_ROWS = 65535ull * 64;   // the GEMM grid's row tiles (sns_pks.hip)

}  // namespace

// d_A, d_T and the key are shared by every call: ordered across streams by the slot's ws_begin / ws_end
struct tfhe_sns_pks_ctx : device_slot {
  tfhe_sns_pks_params pp{};
  size_t chunk_groups = 0;  // TFHE_HIP_SNS_PKS_CHUNK at create; 0: by the T budget
  u64* d_pksk = nullptr;
  u64* d_corr = nullptr;
  bool key = false;
  u64* d_A = nullptr;
  u64* d_T = nullptr;
  size_t rows_cap = 0;  // LWEs the A / T workspaces hold
  double seeded_ms[3] = {0, 0, 0};  // the last seeded load: upload, expansion, correction (device ms)
  std::mutex mu;
};

namespace {

int ensure_rows(tfhe_sns_pks_ctx* c, size_t rows) {
  if (c->rows_cap >= rows) return 0;
  RC_TRY(ws_host_wait(*c));  // no launch may still use the old buffers
  (void)hipFree(c->d_A);
  (void)hipFree(c->d_T);
  c->d_A = c->d_T = nullptr;
  c->rows_cap = 0;
  const size_t K = (size_t)c->pp.in_dim * c->pp.level, Nc = (size_t)(c->pp.out_k + 1) * c->pp.out_N;
  HIP_TRY(hipMalloc(&c->d_A, rows * K * sizeof(u64)));
  HIP_TRY(hipMalloc(&c->d_T, rows * Nc * 16));
  c->rows_cap = rows;
  return 0;
}

// chunks of whole groups: the T workspace stays under its budget (or holds chunk_groups groups); the caller orders
// the workspaces (ws_begin / ws_end)
int pack_device(tfhe_sns_pks_ctx* c, const u64* d_lwes, size_t count, u64* d_out, hipStream_t s) {
  const tfhe_sns_pks_params& p = c->pp;
  const size_t Nc = (size_t)(p.out_k + 1) * p.out_N, lpg = p.lwe_per_glwe, ct_words = 2 * ((size_t)p.in_dim + 1);
  size_t groups = c->chunk_groups ? c->chunk_groups : std::max<size_t>(1, SPK_T_BUDGET / (lpg * Nc * 16));
  groups = std::max<size_t>(1, std::min(groups, SPK_MAX_ROWS / lpg));
  const size_t rows = std::min(count, groups * lpg);
  RC_TRY(ensure_rows(c, rows));
  for (size_t first = 0; first < count; first += rows) {
    const size_t n = std::min(rows, count - first);
    HIP_TRY(tfhe::launch_sns_pks_pack(d_lwes + first * ct_words, n, (int)p.in_dim, (int)p.base_log, (int)p.level,
                                      (int)p.out_k, (int)p.out_N, (int)lpg, c->d_pksk, c->d_corr, c->d_A, c->d_T,
                                      d_out + (first / lpg) * 2 * Nc, s));
  }
  return 0;
}

int pack_checks(tfhe_sns_pks_ctx* c, const void* in, size_t count, const void* out) {
  if (!c) return fail(TFHE_HIP_EINVAL, "sns_pks_pack: null ctx");
  if (!c->key) return fail(TFHE_HIP_ENOKEYS, "sns_pks_pack: key not loaded");
  if (count == 0) return 0;
  if (!in || !out) return fail(TFHE_HIP_EINVAL, "sns_pks_pack: null buffer");
  if (count > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "sns_pks_pack: too many ciphertexts");
  return 0;
}

// what both loaders allocate on first use: the resident key and its correction row
int key_buffers(tfhe_sns_pks_ctx* c) {
  if (!c->d_pksk) HIP_TRY(hipMalloc(&c->d_pksk, tfhe::client::sns_pksk_len(c->pp) * 8));
  if (!c->d_corr) HIP_TRY(hipMalloc(&c->d_corr, (size_t)(c->pp.out_k + 1) * c->pp.out_N * 16));
  return 0;
}

// the correction row of the key words in d_pksk, the last step of both loaders
hipError_t launch_corr(tfhe_sns_pks_ctx* c) {
  return tfhe::launch_sns_pks_corr(c->d_pksk, (int)(c->pp.in_dim * c->pp.level), (int)((c->pp.out_k + 1) * c->pp.out_N),
                                   (int)c->pp.out_N, (int)c->pp.base_log, c->d_corr, c->stream);
}

// the seeded loader's expansion of the whole key in one launch, into the resident key or the expand aid's output
hipError_t launch_rows(tfhe_sns_pks_ctx* c, const tfhe::seeded_round_keys& rk, const u64* d_bodies, u64* dst) {
  return tfhe::launch_seeded_rows128(rk, tfhe::SEEDED128_SNS_PKSK, {c->pp.out_k, c->pp.out_N, c->pp.level}, 0,
                                     (u64)c->pp.in_dim * c->pp.level, d_bodies, dst, c->stream);
}

}  // namespace

extern "C" {

int tfhe_hip_sns_pks_params_preset(int preset, tfhe_sns_pks_params* o) {
  if (!o) return fail(TFHE_HIP_EINVAL, "sns_pks_params_preset: null out");
  if (preset != TFHE_HIP_SNS_PKS_PRESET_FHEVM) return fail(TFHE_HIP_EINVAL, "unknown squashed-packing preset %d", preset);
  *o = tfhe_sns_pks_params{4096, 6, 1024, 61, 1, 128, 128, -62};
  return 0;
}

size_t tfhe_hip_sns_pksk_len(const tfhe_sns_pks_params* pp) { return pp ? tfhe::client::sns_pksk_len(*pp) : 0; }

int tfhe_hip_sns_pks_keygen_k(const tfhe_sns_pks_params* pp, const tfhe_rng_key* rk, const uint64_t* in_key,
                              uint64_t* out_key, uint64_t* pksk) {
  if (!spk_valid(pp) || !rk || !in_key || !out_key) return fail(TFHE_HIP_EINVAL, "sns_pks_keygen: bad arguments");
  RC_TRY(check_binary(in_key, pp->in_dim, "sns_pks_keygen: in_key"));
  tfhe::client::sns_pks_keygen(*pp, *rk, in_key, out_key, pksk);
  return 0;
}

int tfhe_hip_sns_pks_keygen(const tfhe_sns_pks_params* pp, uint64_t seed, const uint64_t* in_key, uint64_t* out_key,
                            uint64_t* pksk) {
  const tfhe_rng_key rk = tfhe::client::rng_key_from_seed(seed);
  return tfhe_hip_sns_pks_keygen_k(pp, &rk, in_key, out_key, pksk);
}

int tfhe_hip_sns_pks_create(const tfhe_sns_pks_params* pp, int device, tfhe_sns_pks_ctx** out) {
  if (!out) return fail(TFHE_HIP_EINVAL, "sns_pks_create: null out");
  *out = nullptr;
  if (!spk_valid(pp)) return fail(TFHE_HIP_EINVAL, "sns_pks_create: invalid parameters");
  tfhe_sns_pks_ctx* c = new tfhe_sns_pks_ctx();
  c->pp = *pp;
  c->chunk_groups = env_positive("TFHE_HIP_SNS_PKS_CHUNK", 0);
  const int rc = slot_open(*c, device, "sns_pks_create", "device setup failed");
  if (rc) {
    tfhe_hip_sns_pks_destroy(c);
    return rc;
  }
  *out = c;
  return 0;
}

void tfhe_hip_sns_pks_destroy(tfhe_sns_pks_ctx* c) {
  if (!c) return;
  slot_close(*c, {c->d_pksk, c->d_corr, c->d_A, c->d_T});
  delete c;
}

int tfhe_hip_sns_pks_load_key(tfhe_sns_pks_ctx* c, const uint64_t* pksk, size_t len) {
  if (!c || !pksk) return fail(TFHE_HIP_EINVAL, "sns_pks_load_key: null argument");
  if (len != tfhe::client::sns_pksk_len(c->pp))
    return fail(TFHE_HIP_EINVAL, "sns_pks_load_key: length %zu, expected %zu", len, tfhe::client::sns_pksk_len(c->pp));
  return side_key_load(c, [&] { return key_buffers(c); }, [&]() -> int {
    HIP_TRY(hipMemcpyAsync(c->d_pksk, pksk, len * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_corr(c));
    return 0;
  });
}

size_t tfhe_hip_sns_pks_seeded_bodies_len(const tfhe_sns_pks_params* pp) {
  return spk_valid(pp) ? tfhe::seeded::sns_pks_bodies_len(*pp) : 0;
}

int tfhe_hip_sns_pks_seeded_keygen_k(const tfhe_sns_pks_params* pp, const tfhe_rng_key* rk, const uint64_t seed[2],
                                     const uint64_t* in_key, uint64_t* out_key, uint64_t* bodies) {
  if (!spk_valid(pp) || !rk || !seed || !in_key || !out_key)
    return fail(TFHE_HIP_EINVAL, "sns_pks_seeded_keygen: bad arguments");
  RC_TRY(check_binary(in_key, pp->in_dim, "sns_pks_seeded_keygen: in_key"));
  tfhe::seeded::sns_pks_seeded_keygen(*pp, *rk, seed, in_key, out_key, bodies);
  return 0;
}

int tfhe_hip_sns_pks_seeded_keygen(const tfhe_sns_pks_params* pp, uint64_t rng_seed, const uint64_t seed[2],
                                   const uint64_t* in_key, uint64_t* out_key, uint64_t* bodies) {
  const tfhe_rng_key rk = tfhe::client::rng_key_from_seed(rng_seed);
  return tfhe_hip_sns_pks_seeded_keygen_k(pp, &rk, seed, in_key, out_key, bodies);
}

int tfhe_hip_sns_pks_decompress_key(const tfhe_sns_pks_params* pp, const uint64_t seed[2], const uint64_t* bodies,
                                    uint64_t* pksk) {
  if (!spk_valid(pp) || !seed || !bodies || !pksk)
    return fail(TFHE_HIP_EINVAL, "sns_pks_decompress_key: bad arguments");
  tfhe::seeded::sns_pks_decompress_key(*pp, seed, bodies, pksk);
  return 0;
}

// tfhe_hip_sns_pks_load_key from the seeded source: the bodies go up into a buffer of this call and the rows are
// expanded straight into the resident key
int tfhe_hip_sns_pks_load_key_seeded(tfhe_sns_pks_ctx* c, const uint64_t seed[2], const uint64_t* bodies, size_t len) {
  if (!c || !seed || !bodies) return fail(TFHE_HIP_EINVAL, "sns_pks_load_key_seeded: null argument");
  if (len != tfhe::seeded::sns_pks_bodies_len(c->pp))
    return fail(TFHE_HIP_EINVAL, "sns_pks_load_key_seeded: length %zu, expected %zu", len,
                tfhe::seeded::sns_pks_bodies_len(c->pp));
  const tfhe::seeded_round_keys rk = round_keys_of(seed);
  call_buffers tmp;
  u64* d_bodies = nullptr;
  phase_timer tm(c);
  return side_key_load(
      c,
      [&] {
        RC_TRY(tmp.alloc(c->device, len * 8, &d_bodies));
        return key_buffers(c);
      },
      [&] {
        RC_TRY(tm.tick(-1));
        HIP_TRY(hipMemcpyAsync(d_bodies, bodies, len * 8, hipMemcpyHostToDevice, c->stream));
        RC_TRY(tm.tick(0));
        HIP_TRY(launch_rows(c, rk, d_bodies, c->d_pksk));
        RC_TRY(tm.tick(1));
        HIP_TRY(launch_corr(c));
        RC_TRY(tm.tick(2));
        return tm.totals(c->seeded_ms, 3);
      });
}

int tfhe_hip_sns_pks_seeded_load_stats(const tfhe_sns_pks_ctx* c, double* upload_ms, double* expand_ms,
                                       double* corr_ms) {
  if (!c) return fail(TFHE_HIP_EINVAL, "sns_pks_seeded_load_stats: null ctx");
  return seeded_ms_read(c->seeded_ms, upload_ms, expand_ms, corr_ms);
}

// test-facing: the seeded loader's upload and launch into guarded_expand's output in place of the resident key
int tfhe_hip_sns_pks_seeded_expand_key(tfhe_sns_pks_ctx* c, const uint64_t seed[2], const uint64_t* bodies,
                                       uint64_t* out_host) {
  if (!c || !seed || !bodies || !out_host) return fail(TFHE_HIP_EINVAL, "sns_pks_seeded_expand_key: null argument");
  const tfhe::seeded_round_keys rk = round_keys_of(seed);
  const size_t body_bytes = tfhe::seeded::sns_pks_bodies_len(c->pp) * 8;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  return guarded_expand(*c, body_bytes, tfhe::client::sns_pksk_len(c->pp), out_host,
                        [&](u64* d_bodies, u64* d_out) -> int {
                          HIP_TRY(hipMemcpyAsync(d_bodies, bodies, body_bytes, hipMemcpyHostToDevice, c->stream));
                          HIP_TRY(launch_rows(c, rk, d_bodies, d_out));
                          return 0;
                        });
}

int tfhe_hip_sns_pks_pack_async(tfhe_sns_pks_ctx* c, const uint64_t* d_lwes, size_t count, uint64_t* d_glwes,
                                void* stream) {
  RC_TRY(pack_checks(c, d_lwes, count, d_glwes));
  if (count == 0) return 0;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  hipStream_t st = resolve_stream(stream, c->stream);
  RC_TRY(ws_begin(*c, st));
  RC_TRY(pack_device(c, d_lwes, count, d_glwes, st));
  return ws_end(*c, st);
}

int tfhe_hip_sns_pks_pack(tfhe_sns_pks_ctx* c, const uint64_t* lwes, size_t count, uint64_t* glwes) {
  RC_TRY(pack_checks(c, lwes, count, glwes));
  if (count == 0) return 0;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const tfhe_sns_pks_params& p = c->pp;
  const size_t in_bytes = count * 2 * ((size_t)p.in_dim + 1) * 8;
  const size_t groups = (count + p.lwe_per_glwe - 1) / p.lwe_per_glwe;
  const size_t out_bytes = groups * (p.out_k + 1) * 2 * p.out_N * 8;
  return staged_run(*c, {{lwes, in_bytes}}, out_bytes, {{glwes, 1, out_bytes}},
                    [&](tfhe_sns_pks_ctx& s, std::vector<void*>& d) {
                      return pack_device(&s, (const u64*)d[0], count, (u64*)d[1], s.stream);
                    });
}

int tfhe_hip_sns_pks_pack_host(const tfhe_sns_pks_params* pp, const uint64_t* pksk, const uint64_t* lwes, size_t count,
                               uint64_t* glwes) {
  if (!spk_valid(pp)) return fail(TFHE_HIP_EINVAL, "sns_pks_pack_host: invalid parameters");
  if (count == 0) return 0;
  if (!pksk || !lwes || !glwes) return fail(TFHE_HIP_EINVAL, "sns_pks_pack_host: null buffer");
  if (count > 0x7FFFFFFF) return fail(TFHE_HIP_EINVAL, "sns_pks_pack_host: too many ciphertexts");
  tfhe::client::sns_pks_pack_host(*pp, pksk, lwes, count, glwes);
  return 0;
}

size_t tfhe_hip_sns_pks_packed_words(const tfhe_sns_pks_params* pp, uint32_t bodies) {
  return pp ? tfhe::client::sns_pks_packed_words(*pp, bodies) : 0;
}

int tfhe_hip_sns_pks_compress(const tfhe_sns_pks_params* pp, const uint64_t* glwe, uint32_t bodies, uint64_t* packed) {
  if (!spk_valid(pp) || !glwe || !packed || bodies > pp->out_N)
    return fail(TFHE_HIP_EINVAL, "sns_pks_compress: bad arguments");
  tfhe::client::sns_pks_compress(*pp, glwe, bodies, packed);
  return 0;
}

int tfhe_hip_sns_pks_extract(const tfhe_sns_pks_params* pp, const uint64_t* packed, uint32_t bodies, uint64_t* glwe) {
  if (!spk_valid(pp) || !glwe || !packed || bodies > pp->out_N)
    return fail(TFHE_HIP_EINVAL, "sns_pks_extract: bad arguments");
  tfhe::client::sns_pks_extract(*pp, packed, bodies, glwe);
  return 0;
}

int tfhe_hip_glwe_phase128(uint32_t k, uint32_t N, const uint64_t* key, const uint64_t* glwe, uint64_t* out) {
  if (!k || !N || !key || !glwe || !out) return fail(TFHE_HIP_EINVAL, "glwe_phase128: bad arguments");
  tfhe::client::glwe_phase128(k, N, key, glwe, out);
  return 0;
}

}  // extern "C"
