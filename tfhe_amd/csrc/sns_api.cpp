// sns_api.cpp — C ABI of noise squashing (include/tfhe_hip.h, tfhe_hip_sns_*): key residency,
// workspaces, chunked launches.  Kernels: sns.hip; host key material: client.cpp.
#include <hip/hip_runtime_api.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/tfhe_hip.h"
#include "client.h"
#include "host_common.h"
#include "pbs_kernels.h"

using tfhe::u64;

namespace {

// the device kernels of this build: k = 2, N = 2048, 2^24 x 3 (any n), words over Z_2^128
bool sns_valid(const tfhe_sns_params* sp) {
  return sp && sp->n > 0 && sp->k == 2 && sp->N == 2048 && sp->base_log == 24 && sp->level == 3 &&
         sp->noise_log2 < 0 && sp->noise_log2 > -64;
}

// ciphertexts per pass (acc 96 KB + digit spectra 147 KB + MAC products 246 KB each); TFHE_HIP_SNS_CHUNK overrides.
// 512 since round 6: a 1024 batch as two 512 chunks measured 4,819 vs 4,556 squashes/s (256: 4,455) on one box
// (profiles/r06c_sns_chunk.txt; round 5: 4,687 vs 4,568): the inverse gains more from the smaller per-CMUX working set
// than the MAC and step 1 lose to the half-size grids
size_t sns_chunk() {
  static const size_t v = env_positive("TFHE_HIP_SNS_CHUNK", 512);
  return v;
}

constexpr size_t LOAD_CHUNK_POLYS = 2048;  // polynomials per chunk of tfhe_hip_sns_load_key

// GGSWs per chunk of a seeded load: the staging buffer takes whole rows, and a GGSW is L (k + 1) rows = 27
// polynomials, so the 2048 polynomials of tfhe_hip_sns_load_key become 75 GGSWs = 2025.  TFHE_HIP_SNS_SEEDED_CHUNK
// (GGSWs, read at every load) overrides: the tests cross chunk boundaries at n = 3
size_t seeded_units(const tfhe_sns_params& sp) {
  const size_t unit_polys = (size_t)sp.level * (sp.k + 1) * (sp.k + 1);
  const size_t u = env_positive("TFHE_HIP_SNS_SEEDED_CHUNK", std::max<size_t>(1, LOAD_CHUNK_POLYS / unit_polys));
  return std::min<size_t>(u, sp.n);
}
size_t seeded_chunk_polys(const tfhe_sns_params& sp) { return seeded_units(sp) * sp.level * (sp.k + 1) * (sp.k + 1); }

}  // namespace

// d_acc, d_D, d_O, d_lut and the key are shared by every call: ordered across streams by the slot's ws_begin / ws_end
struct tfhe_sns_ctx : device_slot {
  tfhe_sns_params sp{};
  void* d_fconst = nullptr;
  void* d_bskf = nullptr;  // key limb spectra (n x 9 x 3 x 5 x 1024 complex f64)
  bool key = false;
  u64* d_acc = nullptr;    // chunk x 3 x (lo, hi) x N
  void* d_D = nullptr;     // digit spectra (chunk x 9 x 1024 complex)
  void* d_O = nullptr;     // MAC products (chunk x 15 x 1024 complex)
  u64* d_lut = nullptr;
  uint32_t lut_mm = 0;
  size_t ws_cap = 0;
  double seeded_ms[3] = {0, 0, 0};  // the last seeded load: upload, expansion, conversion (device ms)
  std::mutex mu;
};

namespace {

int ensure_ws(tfhe_sns_ctx* c, size_t B) {
  if (c->ws_cap >= B) return 0;
  RC_TRY(ws_host_wait(*c));  // no launch may still use the old buffers
  (void)hipFree(c->d_acc);
  (void)hipFree(c->d_D);
  (void)hipFree(c->d_O);
  c->d_acc = nullptr;
  c->d_D = c->d_O = nullptr;
  c->ws_cap = 0;
  const size_t poly = 2 * (size_t)c->sp.N;
  HIP_TRY(hipMalloc(&c->d_acc, B * (c->sp.k + 1) * poly * 8));
  HIP_TRY(hipMalloc(&c->d_D, tfhe::sns_digit_len(B) * 16));
  HIP_TRY(hipMalloc(&c->d_O, tfhe::sns_fft_prod_len(B) * 16));
  c->ws_cap = B;
  return 0;
}

int ensure_lut(tfhe_sns_ctx* c, uint32_t mm) {
  if (c->d_lut && c->lut_mm == mm) return 0;
  std::vector<u64> lut(2 * (size_t)c->sp.N);
  tfhe::client::sns_lut_identity(c->sp, mm, lut.data());
  RC_TRY(ws_host_wait(*c));  // a call in flight on another stream still reads the previous modulus' LUT
  if (!c->d_lut) HIP_TRY(hipMalloc(&c->d_lut, lut.size() * 8));
  HIP_TRY(hipMemcpy(c->d_lut, lut.data(), lut.size() * 8, hipMemcpyHostToDevice));
  c->lut_mm = mm;
  return 0;
}

// squash (out != null) or blind rotate only (acc_out != null) of B device ciphertexts (the caller orders the
// workspaces: ws_begin / ws_end)
int run_device(tfhe_sns_ctx* c, const u64* d_in, size_t B, u64* d_out, u64* d_acc_out, hipStream_t s) {
  const size_t chunk = std::min(B, sns_chunk());
  RC_TRY(ensure_ws(c, chunk));
  const size_t in_dim = c->sp.n + 1, out_dim = 2 * ((size_t)c->sp.k * c->sp.N + 1);
  const size_t acc_len = (size_t)(c->sp.k + 1) * 2 * c->sp.N;
  for (size_t f = 0; f < B; f += chunk) {
    const size_t nb = std::min(chunk, B - f);
    HIP_TRY(tfhe::launch_sns_blind_rotate(d_in + f * in_dim, nb, (int)c->sp.n, c->d_lut, c->d_bskf, c->d_acc, c->d_D,
                                          c->d_O, c->d_fconst, s));
    if (d_out) HIP_TRY(tfhe::launch_sns_extract(c->d_acc, nb, d_out + f * out_dim, s));
    if (d_acc_out)
      HIP_TRY(hipMemcpyAsync(d_acc_out + f * acc_len, c->d_acc, nb * acc_len * 8, hipMemcpyDeviceToDevice, s));
  }
  return 0;
}

// the argument checks of the host and the async calls (B == 0 passes: the caller returns before it touches the device)
int squash_checks(tfhe_sns_ctx* c, const void* in, size_t B, uint32_t mm, const void* out) {
  if (!c) return fail(TFHE_HIP_EINVAL, "sns: null ctx");
  if (!c->key) return fail(TFHE_HIP_ENOKEYS, "sns: key not loaded");
  if (B == 0) return 0;
  if (!in || !out || !mm || mm > c->sp.N || (c->sp.N % mm)) return fail(TFHE_HIP_EINVAL, "sns: bad arguments");
  return 0;
}

int host_call(tfhe_sns_ctx* c, const u64* in, size_t B, uint32_t mm, u64* out, bool acc_only) {
  RC_TRY(squash_checks(c, in, B, mm, out));
  if (B == 0) return 0;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  RC_TRY(ensure_lut(c, mm));
  const size_t in_bytes = B * (c->sp.n + 1) * 8;
  const size_t out_bytes = acc_only ? B * (c->sp.k + 1) * 2 * c->sp.N * 8 : B * 2 * ((size_t)c->sp.k * c->sp.N + 1) * 8;
  return staged_run(*c, {{in, in_bytes}}, out_bytes, {{out, 1, out_bytes}}, [&](tfhe_sns_ctx& s, std::vector<void*>& d) {
    u64* d_out = (u64*)d[1];
    return run_device(&s, (const u64*)d[0], B, acc_only ? nullptr : d_out, acc_only ? d_out : nullptr, s.stream);
  });
}

// what a load of chunks of `per` polynomials needs on the device: the staging buffer of one chunk and, on first use,
// the spectra
int key_buffers(tfhe_sns_ctx* c, size_t per) {
  RC_TRY(ws_grow(*c, &c->d_stage, &c->stage_cap, per * 2 * (size_t)c->sp.N * 8));
  if (!c->d_bskf) HIP_TRY(hipMalloc(&c->d_bskf, tfhe::sns_fft_key_len(c->sp.n) * 16));
  return 0;
}

// Walk the key in chunks of `per` polynomials ((lo, hi) planes) on the ctx's stream.  source(first, np, dst) puts the
// standard-domain words of polynomials first .. first + np - 1 at dst.  The loaders (d_out == null) stage every chunk
// in d_stage, which the next chunk's source reuses (same stream: ordered), and convert it to limb spectra at its offset
// in d_bskf; tm books the conversion as phase 2.  The expand aid gives d_out: the chunks land side by side in it and
// nothing follows.
template <class Src>
int key_chunks(tfhe_sns_ctx* c, size_t per, u64* d_out, phase_timer& tm, Src&& source) {
  const size_t poly_words = 2 * (size_t)c->sp.N, polys = tfhe::client::sns_bsk_len(c->sp) / poly_words;
  for (size_t f = 0; f < polys; f += per) {
    const size_t np = std::min(per, polys - f);
    u64* dst = d_out ? d_out + f * poly_words : (u64*)c->d_stage;
    RC_TRY(source(f, np, dst));
    if (d_out) continue;
    HIP_TRY(tfhe::launch_sns_bsk_to_fft(dst, (char*)c->d_bskf + f * tfhe::SNS_FFT_POLY_BYTES, np, c->d_fconst,
                                        c->stream));
    RC_TRY(tm.tick(2));
  }
  return 0;
}

// The seeded source of key_chunks, for chunks of whole GGSWs (seeded_units): a row of k + 1 polynomials has one body
// polynomial, so the bodies of the chunk's rows go up into d_bodies (one chunk's worth, reused by the next chunk) and
// launch_seeded_rows128 expands them from the chunk's first stream row.  tm books phases 0 and 1.
struct seeded_source {
  tfhe_sns_ctx* c;
  tfhe::seeded_round_keys rk;
  const u64* bodies;
  u64* d_bodies;
  phase_timer& tm;
  size_t body_bytes(size_t polys) const { return polys / (c->sp.k + 1) * 2 * c->sp.N * 8; }
  int operator()(size_t first, size_t np, u64* dst) const {
    const size_t row0 = first / (c->sp.k + 1), rows = np / (c->sp.k + 1);
    RC_TRY(tm.tick(-1));
    HIP_TRY(hipMemcpyAsync(d_bodies, bodies + row0 * 2 * c->sp.N, body_bytes(np), hipMemcpyHostToDevice, c->stream));
    RC_TRY(tm.tick(0));
    HIP_TRY(tfhe::launch_seeded_rows128(rk, tfhe::SEEDED128_SNS_BSK, {c->sp.k, c->sp.N, c->sp.level}, row0, rows,
                                        d_bodies, dst, c->stream));
    return tm.tick(1);
  }
};

}  // namespace

extern "C" {

int tfhe_hip_sns_params_preset(int preset, tfhe_sns_params* o) {
  if (!o) return fail(TFHE_HIP_EINVAL, "sns_params_preset: null out");
  if (preset != TFHE_HIP_SNS_PRESET_FHEVM) return fail(TFHE_HIP_EINVAL, "unknown squashing preset %d", preset);
  *o = tfhe_sns_params{918, 2, 2048, 24, 3, -34};
  return 0;
}

size_t tfhe_hip_sns_bsk_len(const tfhe_sns_params* sp) { return sp ? tfhe::client::sns_bsk_len(*sp) : 0; }

int tfhe_hip_sns_keygen_k(const tfhe_sns_params* sp, const tfhe_rng_key* rk, const uint64_t* lwe_key,
                          uint64_t* glwe_key, uint64_t* bsk) {
  if (!sns_valid(sp) || !rk || !lwe_key || !glwe_key) return fail(TFHE_HIP_EINVAL, "sns_keygen: bad arguments");
  RC_TRY(check_binary(lwe_key, sp->n, "sns_keygen: lwe_key"));
  tfhe::client::sns_keygen(*sp, *rk, lwe_key, glwe_key, bsk);
  return 0;
}

int tfhe_hip_sns_keygen(const tfhe_sns_params* sp, uint64_t seed, const uint64_t* lwe_key, uint64_t* glwe_key,
                        uint64_t* bsk) {
  const tfhe_rng_key rk = tfhe::client::rng_key_from_seed(seed);
  return tfhe_hip_sns_keygen_k(sp, &rk, lwe_key, glwe_key, bsk);
}

int tfhe_hip_sns_create(const tfhe_sns_params* sp, int device, tfhe_sns_ctx** out) {
  if (!out) return fail(TFHE_HIP_EINVAL, "sns_create: null out");
  *out = nullptr;
  if (!sns_valid(sp))
    return fail(TFHE_HIP_EUNSUPPORTED, "sns_create: the device kernels cover k = 2, N = 2048, 2^24 x 3");
  tfhe_sns_ctx* c = new tfhe_sns_ctx();
  c->sp = *sp;
  int rc = slot_open(*c, device, "sns_create", "device setup failed");
  if (!rc) {
    DeviceGuard g(device);
    std::vector<unsigned char> F(tfhe::sns_fft_const_bytes());
    tfhe::make_sns_fft_const(F.data());
    if (hipMalloc(&c->d_fconst, F.size()) != hipSuccess ||
        hipMemcpy(c->d_fconst, F.data(), F.size(), hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(TFHE_HIP_EDEVICE, "sns_create: device setup failed");
  }
  if (rc) {
    tfhe_hip_sns_destroy(c);
    return rc;
  }
  *out = c;
  return 0;
}

void tfhe_hip_sns_destroy(tfhe_sns_ctx* c) {
  if (!c) return;
  slot_close(*c, {c->d_fconst, c->d_bskf, c->d_acc, c->d_D, c->d_O, c->d_lut});
  delete c;
}

int tfhe_hip_sns_load_key(tfhe_sns_ctx* c, const uint64_t* bsk, size_t len) {
  if (!c || !bsk) return fail(TFHE_HIP_EINVAL, "sns_load_key: null argument");
  if (len != tfhe::client::sns_bsk_len(c->sp))
    return fail(TFHE_HIP_EINVAL, "sns_load_key: length %zu, expected %zu", len, tfhe::client::sns_bsk_len(c->sp));
  const size_t poly_words = 2 * (size_t)c->sp.N;
  phase_timer none(nullptr);
  return side_key_load(
      c, [&] { return key_buffers(c, LOAD_CHUNK_POLYS); },
      [&] {
        return key_chunks(c, LOAD_CHUNK_POLYS, nullptr, none, [&](size_t first, size_t np, u64* dst) -> int {
          HIP_TRY(hipMemcpyAsync(dst, bsk + first * poly_words, np * poly_words * 8, hipMemcpyHostToDevice, c->stream));
          return 0;
        });
      });
}

size_t tfhe_hip_sns_seeded_bodies_len(const tfhe_sns_params* sp) {
  return sns_valid(sp) ? tfhe::seeded::sns_bodies_len(*sp) : 0;
}

int tfhe_hip_sns_seeded_keygen_k(const tfhe_sns_params* sp, const tfhe_rng_key* rk, const uint64_t seed[2],
                                 const uint64_t* lwe_key, uint64_t* glwe_key, uint64_t* bodies) {
  if (!sns_valid(sp) || !rk || !seed || !lwe_key || !glwe_key)
    return fail(TFHE_HIP_EINVAL, "sns_seeded_keygen: bad arguments");
  RC_TRY(check_binary(lwe_key, sp->n, "sns_seeded_keygen: lwe_key"));
  tfhe::seeded::sns_seeded_keygen(*sp, *rk, seed, lwe_key, glwe_key, bodies);
  return 0;
}

int tfhe_hip_sns_seeded_keygen(const tfhe_sns_params* sp, uint64_t rng_seed, const uint64_t seed[2],
                               const uint64_t* lwe_key, uint64_t* glwe_key, uint64_t* bodies) {
  const tfhe_rng_key rk = tfhe::client::rng_key_from_seed(rng_seed);
  return tfhe_hip_sns_seeded_keygen_k(sp, &rk, seed, lwe_key, glwe_key, bodies);
}

int tfhe_hip_sns_decompress_bsk(const tfhe_sns_params* sp, const uint64_t seed[2], const uint64_t* bodies,
                                uint64_t* bsk) {
  if (!sns_valid(sp) || !seed || !bodies || !bsk) return fail(TFHE_HIP_EINVAL, "sns_decompress_bsk: bad arguments");
  tfhe::seeded::sns_decompress_bsk(*sp, seed, bodies, bsk);
  return 0;
}

int tfhe_hip_csprng_words128(const uint64_t seed[2], uint64_t first_word, size_t count, uint64_t* out_pairs) {
  if (!seed || (count && !out_pairs)) return fail(TFHE_HIP_EINVAL, "csprng_words128: null argument");
  if (first_word > (1ull << 59) || count > (1ull << 59)) return fail(TFHE_HIP_EINVAL, "csprng_words128: out of range");
  tfhe::seeded::csprng_words128(seed, first_word, count, out_pairs);
  return 0;
}

// tfhe_hip_sns_load_key from the seeded source: a body buffer of one chunk beside the loader's buffers
int tfhe_hip_sns_load_key_seeded(tfhe_sns_ctx* c, const uint64_t seed[2], const uint64_t* bodies, size_t len) {
  if (!c || !seed || !bodies) return fail(TFHE_HIP_EINVAL, "sns_load_key_seeded: null argument");
  if (len != tfhe::seeded::sns_bodies_len(c->sp))
    return fail(TFHE_HIP_EINVAL, "sns_load_key_seeded: length %zu, expected %zu", len,
                tfhe::seeded::sns_bodies_len(c->sp));
  const size_t per = seeded_chunk_polys(c->sp);
  call_buffers tmp;
  phase_timer tm(c);
  seeded_source src{c, round_keys_of(seed), bodies, nullptr, tm};
  return side_key_load(
      c,
      [&] {
        RC_TRY(tmp.alloc(c->device, src.body_bytes(per), &src.d_bodies));
        return key_buffers(c, per);
      },
      [&] {
        RC_TRY(key_chunks(c, per, nullptr, tm, src));
        return tm.totals(c->seeded_ms, 3);
      });
}

int tfhe_hip_sns_seeded_load_stats(const tfhe_sns_ctx* c, double* upload_ms, double* expand_ms, double* convert_ms) {
  if (!c) return fail(TFHE_HIP_EINVAL, "sns_seeded_load_stats: null ctx");
  return seeded_ms_read(c->seeded_ms, upload_ms, expand_ms, convert_ms);
}

// test-facing: the chunks of the seeded loader, launch by launch, into guarded_expand's output in place of the
// staging buffer
int tfhe_hip_sns_seeded_expand_bsk(tfhe_sns_ctx* c, const uint64_t seed[2], const uint64_t* bodies,
                                   uint64_t* out_host) {
  if (!c || !seed || !bodies || !out_host) return fail(TFHE_HIP_EINVAL, "sns_seeded_expand_bsk: null argument");
  const size_t per = seeded_chunk_polys(c->sp);
  phase_timer none(nullptr);
  seeded_source src{c, round_keys_of(seed), bodies, nullptr, none};
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  return guarded_expand(*c, src.body_bytes(per), tfhe::client::sns_bsk_len(c->sp), out_host,
                        [&](u64* d_bodies, u64* d_out) {
                          src.d_bodies = d_bodies;
                          return key_chunks(c, per, d_out, none, src);
                        });
}

int tfhe_hip_sns_squash(tfhe_sns_ctx* c, const uint64_t* in, size_t B, uint32_t mm, uint64_t* out) {
  return host_call(c, in, B, mm, out, false);
}

int tfhe_hip_sns_blind_rotate(tfhe_sns_ctx* c, const uint64_t* in, size_t B, uint32_t mm, uint64_t* acc_out) {
  return host_call(c, in, B, mm, acc_out, true);
}

int tfhe_hip_sns_squash_async(tfhe_sns_ctx* c, const uint64_t* d_in, size_t B, uint32_t mm, uint64_t* d_out,
                              void* stream) {
  RC_TRY(squash_checks(c, d_in, B, mm, d_out));
  if (B == 0) return 0;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  RC_TRY(ensure_lut(c, mm));
  hipStream_t st = resolve_stream(stream, c->stream);
  RC_TRY(ws_begin(*c, st));
  RC_TRY(run_device(c, d_in, B, d_out, nullptr, st));
  return ws_end(*c, st);
}

int tfhe_hip_sns_phase(const tfhe_sns_params* sp, const uint64_t* glwe_key, const uint64_t* cts, size_t count,
                       uint64_t* out) {
  if (!sp || !glwe_key || (count && (!cts || !out))) return fail(TFHE_HIP_EINVAL, "sns_phase: bad arguments");
  tfhe::client::sns_phase(*sp, glwe_key, cts, count, out);
  return 0;
}

}  // extern "C"
