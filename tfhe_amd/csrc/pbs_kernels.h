// pbs_kernels.h — what the host API layer calls in the kernel files: the table of blind-rotation back ends
// (br_engine, one row per .hip file) and the launchers of the other kernels, grouped by source file.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <initializer_list>
#include <type_traits>

#include "gl64.h"

namespace tfhe {
// ---- the blind-rotation back ends: pbs_kernels.hip, pbs_n2048.hip, pbs_fft.hip, pbs_fft2k.hip ----------------------
// One back end = one ring and polynomial size.  Keys, tables and spectra travel as u64 words (the FFT64 rows hold
// doubles in them); every launcher returns hipSuccess for an empty batch.
struct br_engine {
  bool fft;        // FFT64 over the 2^64 torus; false: Goldilocks NTT over Z_p
  unsigned N;
  size_t lat_max;  // default latency crossover: batches (per shard) up to this size run the latency kernel
  const char *lat_kernel, *batch_kernel;  // what tfhe_hip_br_kernel reports
  size_t table_words;                     // device twiddle tables, 8-byte words
  // fills `table_words` words; false = the kernels' compile-time twist constants differ from these host tables
  bool (*make_tables)(u64* tw);
  // standard-domain BSK (`polys` polynomials of N words) -> the transform domain
  hipError_t (*convert_bsk)(const u64* bsk_std, u64* bsk, size_t polys, const u64* tw, hipStream_t s);
  // exactly one of out_big (B x (N + 1) extracted samples) and out_acc (B x 2N accumulators); hipErrorInvalidValue
  // otherwise.  latency: one ciphertext (N = 2048 FFT64: two) per workgroup; n_cus: the device's compute-unit
  // count (the P-GATE FFT64 batch kernel's priority split and start stagger, pbs_fft.hip dispatch_half; <= 0 = 256)
  hipError_t (*blind_rotate)(const u64* lwe_in, size_t B, int n, const u64* luts, const u32* lut_index, int n_lut,
                             const u64* bsk, const u64* tw, u64* out_big, u64* out_acc, bool latency, int n_cus,
                             hipStream_t s);
  // natural-order transforms of `count` polynomials (the parity tests): the NTT rows work in place (in == out), the
  // FFT64 rows N torus words -> N / 2 complex and back to N doubles (no 1 / M, no rounding)
  hipError_t (*fwd)(const u64* in, size_t count, u64* out, const u64* tw, hipStream_t s);
  hipError_t (*inv)(const u64* in, size_t count, u64* out, const u64* tw, hipStream_t s);
};
extern const br_engine ENGINE_NTT1K, ENGINE_NTT2K, ENGINE_FFT1K, ENGINE_FFT2K;

inline const br_engine* find_engine(bool fft, unsigned N) {
  for (const br_engine* e : {&ENGINE_NTT1K, &ENGINE_NTT2K, &ENGINE_FFT1K, &ENGINE_FFT2K})
    if (e->fft == fft && e->N == N) return e;
  return nullptr;
}

// ---- the multi-bit back ends: pbs_fft2k_mb.hip ----------------------------------------------------------------------
// A second lookup beside find_engine: a row serves the keys of grouping factor g_min .. g_max on the ring of `base`
// (whose tables, convert_bsk and transforms it shares; the converted key is (n / g)(2^g - 1) GGSWs in base's layout).
struct br_engine_mb {
  const br_engine* base;
  unsigned g_min, g_max;
  const char* kernel;      // what tfhe_hip_br_kernel reports (one kernel shape for every batch size)
  size_t table_words;      // the back end's own device tables, 8-byte words
  bool (*make_tables)(u64* tw_mb);
  // as br_engine::blind_rotate; n % g == 0, tw = base's tables, tw_mb = this row's
  hipError_t (*blind_rotate)(const u64* lwe_in, size_t B, int n, int g, const u64* luts, const u32* lut_index,
                             int n_lut, const u64* bsk, const u64* tw, const u64* tw_mb, u64* out_big, u64* out_acc,
                             hipStream_t s);
};
extern const br_engine_mb ENGINE_FFT2K_MB;

inline const br_engine_mb* find_engine_mb(const br_engine* base) {
  for (const br_engine_mb* e : {&ENGINE_FFT2K_MB})
    if (e->base == base) return e;
  return nullptr;
}

// The output mode of a blind rotation as compile-time flags: f(WRITE_ACC, WRITE_BIG) launches the kernel
// instantiated for `acc only` or `big only` (f's arguments are std::bool_constant values).
template <class F>
hipError_t launch_out_mode(const u64* out_acc, const u64* out_big, F&& f) {
  if (out_acc && !out_big) f(std::true_type{}, std::false_type{});
  else if (out_big && !out_acc) f(std::false_type{}, std::true_type{});
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---- pbs_kernels.hip ---------------------------------------------------------------------------------------------
// canonical psi: primitive 2N-th root of unity with psi^(2N/64) = 8 (generator 7)
u64 canonical_psi(unsigned N);
// 4 x 1024 twiddle tables of the device NTT layout
void make_ntt_tables(u64 psi, u64* tw);
hipError_t launch_keyswitch(const u64* in_big, size_t B, int big_dim, const u64* ksk, int n, int base_log, int levels,
                           u64* out, hipStream_t s);
// ---- ks_mfma.hip: keyswitch as eight int8 GEMMs on the matrix cores: KSK byte planes built once per key load,
// digits staged in a workspace of ks_digits_bytes(B, ...) bytes
size_t ks_planes_bytes(int big_dim, int levels, int n);
size_t ks_digits_bytes(size_t B, int big_dim, int levels);
hipError_t launch_ksk_planes(const u64* ksk, int big_dim, int levels, int n, void* planes, hipStream_t s);
hipError_t launch_keyswitch_mfma(const u64* in_big, size_t B, int big_dim, const void* planes, int n, int base_log,
                                 int levels, void* digits, u64* out, hipStream_t s);
// packing keyswitch on the matrix cores: the GEMM, then pks.hip's shift-and-sum
size_t pks_mfma_rows(size_t count);
hipError_t launch_pks_gemm_mfma(const u64* lwes, size_t count, int in_dim, int base_log, int LV, int Nc,
                                const void* planes, void* A0, void* A1, u64* T, hipStream_t s);
hipError_t launch_pks_pack_mfma(const u64* lwes, size_t count, int in_dim, int base_log, int L, int k, int N, int lpg,
                                const void* planes, void* A0, void* A1, u64* T, u64* out, hipStream_t s);
// ---- pks.hip: packing keyswitch
hipError_t launch_pks_corr(const u64* pksk, int K, int Nc, int base_log, u64* corr, hipStream_t s);
hipError_t launch_pks_pack(const u64* lwes, size_t count, int in_dim, int base_log, int L, int k, int N, int lpg,
                           const u64* pksk, const u64* corr, u32* A, u64* T, u64* out, hipStream_t s);
// ---- sns.hip (sns_fft.h): noise squashing on the native 2^128 torus: d_fconst = device copy of
// make_sns_fft_const(); words as (lo, hi) planes per polynomial
size_t sns_fft_const_bytes();
void make_sns_fft_const(void* out);
size_t sns_fft_key_len(size_t n);  // key limb spectra, in 16-byte complex
size_t sns_digit_len(size_t B);    // digit spectra workspace, in 16-byte complex
size_t sns_fft_prod_len(size_t B);  // MAC product workspace, in 16-byte complex
constexpr size_t SNS_FFT_POLY_BYTES = 5 * 1024 * 16;  // limb spectra of one (i, r, j) key polynomial (sns_fft.h SF_LIMBS)
hipError_t launch_sns_bsk_to_fft(const u64* bsk_std, void* bsk_fft, size_t polys, const void* d_fconst,
                                 hipStream_t s);
hipError_t launch_sns_blind_rotate(const u64* lwe, size_t B, int n, const u64* lut, const void* bsk_fft, u64* acc,
                                   void* D, void* Oprod, const void* d_fconst, hipStream_t s);
hipError_t launch_sns_extract(const u64* acc, size_t B, u64* out, hipStream_t s);
// ---- sns_pks.hip: packing keyswitch over the 2^128 torus (squashed LWEs -> GLWE planes).  corr: Nc x 16 bytes,
// built once per key; A: count x in_dim*L u64 of digits; T: count x Nc x 16 bytes.  hipErrorInvalidValue for a
// count beyond the grids (more than 65535 row tiles)
hipError_t launch_sns_pks_corr(const u64* pksk, int K, int Nc, int N, int base_log, u64* corr, hipStream_t s);
hipError_t launch_sns_pks_pack(const u64* lwes, size_t count, int in_dim, int base_log, int L, int k, int N, int lpg,
                               const u64* pksk, const u64* corr, u64* A, u64* T, u64* out, hipStream_t s);
// ---- ms_reduce.hip: modulus-switch noise reduction, in place on B x (n+1); picks (device, nullable).
// `zeros` holds the rows [count][n+1] followed by their element-major transpose [n+1][ms_zeros_pitch(count)]
// (padding columns zero).
inline size_t ms_zeros_pitch(size_t count) { return (count + 63) / 64 * 64; }
hipError_t launch_ms_reduce(u64* lwe, size_t B, int n, const u64* zeros, int count, int log2_2N, double bound,
                            double r_sigma, double var128, int* picks, hipStream_t s);
// ---- sample_extract_many.hip: row b * n_fn + f of `out` is the sample of accumulator b at degree f * stride, for
// either ring (zp: Z_p accumulators, converted to 2^64) and N <= 2048; acc 16-byte aligned.  n_fn = stride = 1 is
// the plain degree-0 extraction
hipError_t launch_sample_extract_many(const u64* acc, size_t B, int k, int N, bool zp, int n_fn, int stride, u64* out,
                                      hipStream_t s);
// ---- decompress.hip: decompression, steps 1 and 2: `packed` = ceil(count / lpg) compressed GLWEs (k, N, storage w
// bits) back to back as tfhe_hip_pks_compress writes them -> count x (kN + 1) LWEs, row g * lpg + i = the sample
// at degree i of group g.  N <= 4096 (hipErrorInvalidValue above), count <= 0x7FFFFFFF
hipError_t launch_unpack_extract(const u64* packed, size_t count, int k, int N, int lpg, int w, u64* lwes_out,
                                 hipStream_t s);
// ---- expand.hip: compact-list expansion: `list` = ceil(count / lwe_dim) x lwe_dim mask words, then count body
// words -> rows x (lwe_dim + 1) LWEs, row r = list entry r / rep (rep >= 1 copies of every entry; rows <= count *
// rep).  lwe_dim a power of two in 8 .. 4096, count and rows <= 0x7FFFFFFF (hipErrorInvalidValue otherwise);
// rows == 0 launches nothing
hipError_t launch_expand_compact(const u64* list, size_t count, int lwe_dim, int rep, size_t rows, u64* out,
                                 hipStream_t s);
// ---- csprng.hip: the seeded mask stream (seeded.cpp csprng_words) on the device.  Row r of `out` (at
// out + r * row_stride) gets words first_word .. first_word + dim - 1 of the stream of seed (seeds[2r], seeds[2r+1]);
// zero_body also sets word dim to 0.  first_word + dim <= 2^60, row_stride >= dim (+ 1 with zero_body) and
// rows * ceil(dim / 1022) <= 0x7FFFFFFF (hipErrorInvalidValue otherwise); rows == 0 or dim == 0 launches nothing
hipError_t launch_csprng_rows(const u64* seeds, size_t rows, u64 first_word, u32 dim, size_t row_stride,
                              bool zero_body, u64* out, hipStream_t s);
// ---- seeded_keys.hip: seeded (compressed) server keys expanded on the device, into the standard-domain layouts that
// the conversion kernels read (seeded.cpp decompress_* are the host references).  rk: the 44 round-key words of the
// key's seed (seeded::aes_round_keys, once per seed on the host).  Shape fields read per kind:
//   SEEDED_LIST    n (the dimension), count: bodies [count]                       -> out [count][n + 1]
//   SEEDED_KSK     n, k, N, LV:              bodies [k N][LV]                      -> out [k N][LV - 1 - s][n + 1]
//   SEEDED_BSK     n, k, N, L:               bodies [n][L][k + 1][N]               -> out [n][c L + l][(k + 1) N]
//   SEEDED_BSK_MB  n, k, N, L, g:            bodies [n / g][2^g][L][k + 1][N]      -> out [n / g][sigma - 1][l][c][(k + 1) N],
//                                            sigma = 0 neither read nor written, its stream words stepped over
// hipErrorInvalidValue for a null buffer, a zero level count, g outside 2..4, n % g != 0 or a grid past 2^31 - 1
// workgroups; zero rows launch nothing.
struct seeded_round_keys {
  u32 w[44];
};
enum seeded_kind { SEEDED_LIST = 0, SEEDED_KSK = 1, SEEDED_BSK = 2, SEEDED_BSK_MB = 3 };
struct seeded_shape {
  u32 n, k, N, L, LV, g, count;
};
hipError_t launch_seeded_rows(const seeded_round_keys& rk, seeded_kind kind, const seeded_shape& sh, const u64* bodies,
                              u64* out, hipStream_t s);
// ---- seeded_keys128.hip: seeded 128-bit keys (u128 words as (lo, hi) u64 pairs in the bodies, as [lo][N], [hi][N]
// planes in the output; seeded.cpp sns_decompress_bsk / sns_pks_decompress_key are the host references).  `rows`
// stream rows from row0 on, both whole units (SNS_BSK: the L (k + 1) rows of a GGSW; SNS_PKSK: the L rows of an input
// element); `bodies` holds the body pairs of those rows ([rows][N][2]) and `out` receives their destination rows
// ([rows][k + 1][2][N], the unit's own order: SNS_BSK [i][c L + l], SNS_PKSK [j][L - 1 - s]), so a key may be
// expanded in chunks of units through one staging buffer.  hipErrorInvalidValue for N not a power of two >= 32, a
// zero k or L, a partial unit, a null or not 16-byte-aligned buffer or a grid past 2^31 - 1 workgroups; zero rows
// launch nothing.
enum seeded128_kind { SEEDED128_SNS_BSK = 0, SEEDED128_SNS_PKSK = 1 };
struct seeded128_shape {
  u32 k, N, L;  // mask polynomials of a row, polynomial size, levels
};
hipError_t launch_seeded_rows128(const seeded_round_keys& rk, seeded128_kind kind, const seeded128_shape& sh, u64 row0,
                                 u64 rows, const u64* bodies, u64* out, hipStream_t s);
// rows [count][dim] -> the element-major transpose [dim][ms_zeros_pitch(count)] behind them (ms_reduce.hip)
hipError_t launch_ms_zeros_transpose(const u64* rows, u32 count, u32 dim, u64* tr, hipStream_t s);
// ---- matmul.hip: encrypted matrix x clear matrix.  expand: G seeded GLWEs (seeds G x 2, packed G x ceil(N w / 64)
// words of w-bit body values) -> glwes G x 2 x N.  dot: glwes R x Kb x 2 x N times the resident matrix W (Kb N x Cpad
// u32, value + 2^31, zero = 2^31 past K and past C) -> LWE c < C of row r at out + (r * col_stride + c) * (N + 1).
// N and Cpad multiples of 64, Cpad / 64 <= 65535, C <= Cpad, col_stride >= C (hipErrorInvalidValue otherwise)
hipError_t launch_matmul_expand(const u64* seeds, const u64* packed, size_t G, int N, int w, u64* glwes, hipStream_t s);
hipError_t launch_matmul_dot(const u64* glwes, const u32* W, size_t R, int N, int Kb, int Cpad, int C, size_t col_stride,
                             u64* out, hipStream_t s);
// body (last word) of row r of rows x row_len += post_add[idx ? idx[r] : 0]
hipError_t launch_body_add(u64* lwes, size_t rows, size_t row_len, const u64* post_add, size_t n_lut, const u32* idx,
                           hipStream_t s);
// ---- lincomb.hip: out[r] = sum of terms[t].coef * terms[t].src[0 .. dim - 1] over t in row_start[r] ..
// row_start[r + 1] - 1, body += bias[r] (bias may be null), mod 2^64.  Every terms[t].src is a device row of dim
// words that the caller has checked and that `out` does not overlap; rows == 0 launches nothing
struct lin_term {
  const u64* src;
  u64 coef;
};
hipError_t launch_lincomb(const lin_term* terms, const u32* row_start, const u64* bias, size_t rows, u32 dim, u64* out,
                          hipStream_t s);
}  // namespace tfhe
