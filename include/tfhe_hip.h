/*
 * tfhe_hip.h — C ABI of libtfhe_hip.so, the MI355X-native TFHE programmable-bootstrap engine.
 *
 * This is the drop-in boundary for the reference's PBS path.  In the reference, JS callers reach
 * the TFHE core through packages/wasm (tfhe-rs 0.8.7 compiled to WASM/N-API, an empty submodule
 * here: .gitmodules:4, packages/pnpm-lock.yaml:1988-1995) and through the FHE server's
 * /evaluate endpoint (e2e/test/fhe.test.ts:105-175).  Each entry point below names the reference
 * interface it replaces.  Plain C: pointers + sizes, no torch / HIP types in signatures
 * (streams are passed as void*).
 *
 * Conventions
 *   - LWE ciphertexts: u64[dim + 1] = (a_0 .. a_{dim-1}, b), native torus Z_{2^64}.
 *   - GLWE / BSK values: Z_p, p = 2^64 - 2^32 + 1, canonical in [0, p) (transform 0, the NTT engine);
 *     native torus Z_{2^64} (transform 1, the FFT64 engine: tfhe-rs's own f64-FFT arithmetic).
 *   - BSK (standard domain): u64[n][(k+1)*l][k+1][N]; row index = c*l + lvl (c = component that
 *     carries s_i * 2^(64 - base_log*(lvl+1))), column = GLWE component (0..k-1 mask, k body).
 *   - KSK: u64[k*N][ks_level][n + 1], KSK[j][r] = LWE_s(s'_j * 2^(64 - ks_base_log*(r+1))).
 *   - LUT ("accumulator"): u64[N] in Z_p (see tfhe_hip_lut_*) for both transforms; the FFT64 engine
 *     maps each value back to the torus (x + round(x / 2^32), exact for Delta * m, Delta >= 2^32).
 *   - Every function returns 0 on success or a negative TFHE_HIP_E* code; it never aborts.
 *     tfhe_hip_last_error() returns the message of the last failure on the calling thread.
 *   - Ownership: the caller owns every host buffer; calls read/write them synchronously (the
 *     *_async variants take DEVICE pointers and enqueue on the given HIP stream).  The library
 *     owns device keys and workspaces (freed by tfhe_hip_destroy).
 *   - Threading: a ctx is not re-entrant; calls on one ctx are serialized by an internal mutex.
 */
#ifndef TFHE_HIP_H
#define TFHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFHE_HIP_OK 0
#define TFHE_HIP_EINVAL (-1)      /* bad argument / size mismatch */
#define TFHE_HIP_ENOMEM (-2)      /* host or device allocation failed */
#define TFHE_HIP_EDEVICE (-3)     /* HIP runtime error */
#define TFHE_HIP_ENOKEYS (-4)     /* keys not loaded */
#define TFHE_HIP_EUNSUPPORTED (-5) /* parameter set not supported by the device kernels */

#define TFHE_HIP_PRESET_GATE 0   /* n=630 k=1 N=1024, PBS 7x3, KS 2x8 (TFHE 128-bit default) */
#define TFHE_HIP_PRESET_FHEVM 1  /* n=918 k=1 N=2048, PBS 23x1, KS 4x4 (PARAM_MESSAGE_2_CARRY_2_KS_PBS) */
#define TFHE_HIP_PRESET_GATE_FFT 2 /* P-GATE on the FFT64 transform (native-torus BSK, f64 FFT) */
#define TFHE_HIP_PRESET_FHEVM_FFT 3 /* P-FHEVM on the FFT64 transform (N = 2048 as two 512-point halves) */
#define TFHE_HIP_PRESET_FHEVM_MB_FFT 4 /* preset 3 with n = 924 (divisible by 2, 3 and 4): multi-bit PBS keys */

#define TFHE_HIP_TRANSFORM_NTT 0   /* GLWE/BSK over Z_p, Goldilocks NTT (exact integer arithmetic) */
#define TFHE_HIP_TRANSFORM_FFT64 1 /* GLWE/BSK over Z_2^64, f64 FFT (tfhe-rs FFT64; oracle/fft_oracle.c) */

typedef struct tfhe_params {
  uint32_t n, k, N;
  uint32_t pbs_base_log, pbs_level;
  uint32_t ks_base_log, ks_level;
  int32_t lwe_noise_log2;  /* stddev as log2 of a torus fraction */
  int32_t glwe_noise_log2;
  uint32_t order;          /* 0 = PBS then KS (ciphertexts under the small key), 1 = KS then PBS */
  uint32_t transform;      /* TFHE_HIP_TRANSFORM_*: external-product arithmetic (and BSK domain) */
} tfhe_params;

typedef struct tfhe_ctx tfhe_ctx;

/* ---- parameters & sizes ------------------------------------------------------------------
 * Replaces the tfhe-rs parameter constants selected by name in sdk/relayer/src/tfhe.ts:14-19. */
int tfhe_hip_params_preset(int preset, tfhe_params* out);
size_t tfhe_hip_bsk_len(const tfhe_params* p);
size_t tfhe_hip_ksk_len(const tfhe_params* p);
/* LWE dimension of PBS inputs/outputs (n for order 0, k*N for order 1). */
uint32_t tfhe_hip_io_dim(const tfhe_params* p);

/* ---- client-side key material (host) ------------------------------------------------------
 * Replaces TfheClientKey.generate / ServerKey generation (sdk/relayer/src/tfhe.ts:20-28,
 * generateKeys.js:20-31).  All randomness is ChaCha20 keyed by a 192-bit rng key plus a stream index
 * (LWE key 1, GLWE key 2, BSK_i 0x1000+i, KSK_j 0x100000+j, MS zero z 0x200000+z, multi-bit GGSW (q, sigma)
 * 0x600000 + 16 q + sigma, seeded multi-bit GGSW (q, sigma) 0x700000 + 16 q + sigma, ciphertext q stream0+q;
 * further down: packing key 4 and 0x300000+j, squashing key 5 and 0x400000+i, ct128 packing key 6 and 0x500000+j,
 * seeded squashing GGSW i 0x800000+i, seeded ct128 packing row j 0x900000+j).
 *   - tfhe_hip_rng_key_entropy: 192 bits from the OS (getrandom) -- production keys and encryptions;
 *   - tfhe_hip_rng_key_from_seed: (seed, a public tag) -- REPRODUCIBLE streams for tests, golden vectors
 *     and the oracle.  A seeded key set is public knowledge: never use one for real data.
 * The uint64_t-seed entry points below are the seeded (test) forms of the *_k functions. */
typedef struct tfhe_rng_key {
  uint32_t w[6];
} tfhe_rng_key;
int tfhe_hip_rng_key_entropy(tfhe_rng_key* out);
int tfhe_hip_rng_key_from_seed(uint64_t seed, tfhe_rng_key* out);
int tfhe_hip_keygen_k(const tfhe_params* p, const tfhe_rng_key* rk, uint64_t* lwe_key, uint64_t* glwe_key,
                      uint64_t* bsk /* nullable */, uint64_t* ksk /* nullable */);
int tfhe_hip_keygen(const tfhe_params* p, uint64_t seed, uint64_t* lwe_key, uint64_t* glwe_key,
                    uint64_t* bsk /* nullable */, uint64_t* ksk /* nullable */);
/* BSK / KSK (standard domain) for GIVEN binary secret keys — the server-key half of keygen, for key
 * material ingested from tfhe-rs (the packages/kms loader role, SURVEY §8f f3: the ClientKey of
 * sdk/relayer/src/test/keys/privateKey.bin; tfhe_amd/keyio.py parses it).  EINVAL if a key word is not 0/1. */
int tfhe_hip_server_keygen_k(const tfhe_params* p, const tfhe_rng_key* rk, const uint64_t* lwe_key,
                             const uint64_t* glwe_key, uint64_t* bsk /* nullable */, uint64_t* ksk /* nullable */);
int tfhe_hip_server_keygen(const tfhe_params* p, uint64_t seed, const uint64_t* lwe_key, const uint64_t* glwe_key,
                           uint64_t* bsk /* nullable */, uint64_t* ksk /* nullable */);
/* ---- multi-bit PBS keys (tfhe-rs LweMultiBitBootstrapKey; PARITY UNPINNED at the byte level) ------------------
 * The grouping factor g in {2, 3, 4} belongs to the key, not to tfhe_params; n % g == 0.  Scope: the FFT64
 * transform, k = 1, N = 2048, PBS gadget 2^23 x 1 (the shape of presets 3 and 4); every other shape returns
 * EUNSUPPORTED, a wrong g or n % g != 0 EINVAL.
 *   key     for group q (elements s_{gq} .. s_{gq+g-1}) and every sigma in 1 .. 2^g - 1 one GGSW of the indicator
 *           [ s_{gq+i} == bit i of sigma for all i < g ], encrypted like a classic BSK row (same noise), on ChaCha
 *           stream 0x600000 + 16 q + sigma; sigma = 0 is not stored.  Layout [q][sigma - 1][level][row c][col j][N].
 *   switch  sum first, then switch: t_sigma = ms( sum_{i in sigma} a_{gq+i} mod 2^64 ), ms = the classic rounding
 *           to 2N (NOT the sum of switched values)
 *   step    acc <- acc + ExtProd( sum_sigma (X^{t_sigma} - 1) GGSW_{q,sigma}, acc ), the SignedDecomposer digits
 *           taken from acc itself; exactly one indicator (sigma = 0 included) is 1, so this is
 *           acc <- X^{<a, s>_group} acc.  Initial accumulator, sample extraction and LUT layout as the classic PBS.
 * From one rng key the secret keys and the KSK are word for word those of tfhe_hip_keygen_k / server_keygen_k.
 * tfhe_hip_mb_bsk_len: (n / g) (2^g - 1) (k+1) L (k+1) N words, 0 for invalid arguments. */
size_t tfhe_hip_mb_bsk_len(const tfhe_params* p, uint32_t g);
int tfhe_hip_mb_server_keygen_k(const tfhe_params* p, uint32_t g, const tfhe_rng_key* rk, const uint64_t* lwe_key,
                                const uint64_t* glwe_key, uint64_t* bsk_mb, uint64_t* ksk /* nullable */);
int tfhe_hip_mb_server_keygen(const tfhe_params* p, uint32_t g, uint64_t seed, const uint64_t* lwe_key,
                              const uint64_t* glwe_key, uint64_t* bsk_mb, uint64_t* ksk /* nullable */);
/* Modulus-switch noise reduction key of the P-FHEVM server key (the
 * reference's parameter block carries modulus_switch_zeros_count 1449, ms_bound 2^58,
 * ms_r_sigma_factor 13.179852282053789, ms_input_variance 2.63039184094559e-07 —
 * sdk/relayer/src/test/keys/privateKey.bin @0x5e04..0x5e30).  count LWE encryptions of 0 under
 * the small key, count x (n+1) u64. */
#define TFHE_HIP_MS_FHEVM_ZEROS 1449u
#define TFHE_HIP_MS_FHEVM_BOUND 0x1p58
#define TFHE_HIP_MS_FHEVM_R_SIGMA 13.179852282053789
#define TFHE_HIP_MS_FHEVM_INPUT_VARIANCE 2.63039184094559e-07
int tfhe_hip_ms_zeros_keygen_k(const tfhe_params* p, const tfhe_rng_key* rk, const uint64_t* lwe_key, uint32_t count,
                               uint64_t* zeros);
int tfhe_hip_ms_zeros_keygen(const tfhe_params* p, uint64_t seed, const uint64_t* lwe_key, uint32_t count,
                             uint64_t* zeros);
/* ---- compressed (seeded) server keys, SURVEY §8f f3 ---------------------------------------------
 * Replaces tfhe-rs core_crypto decompress_seeded_lwe_bootstrap_key / decompress_seeded_lwe_keyswitch_key /
 * decompress_seeded_lwe_ciphertext_list behind CompressedServerKey::decompress, the step by which the fhEVM
 * coprocessor turns a tenant's stored key into evaluation keys (tests/fhevm-suite/fhevm/docker-compose/
 * coprocessor-docker-compose.yml:96, --tenant-key-cache-size).  Masks come from the AES-128-CTR stream of a
 * 128-bit seed (seed[0] = low 64 bits) restated from tfhe-csprng (tfhe_amd/csrc/seeded.cpp has the byte order);
 * bodies are in tfhe-rs order:
 *   BSK bodies [i < n][l < L][c <= k][N]   (GGSW i, decomposition level l most significant first, GLWE row c)
 *   KSK bodies [j < k N][s < ks_level]     (input key element j, storage row s = decomposition level ks_level - s:
 *                                           least significant first, as tfhe-rs's keygen walks (1..=levels).rev();
 *                                           engine KSK row ks_level - 1 - s; P-FHEVM: big key -> small key)
 *   list bodies [z < count]                (e.g. the modulus-switch zeros)
 * Decompressed keys land in this engine's standard layouts (tfhe_hip_load_keys, tfhe_hip_load_ms_key).  FFT64
 * presets only (native 2^64 torus).  PARITY UNPINNED at the byte level: the reference holds no server-key file. */
int tfhe_hip_aes128_block(const uint8_t key[16], const uint8_t in[16], uint8_t out[16]); /* FIPS-197 check */
int tfhe_hip_csprng_words(const uint64_t seed[2], uint64_t first_word, size_t count, uint64_t* out);
int tfhe_hip_seeded_server_keygen_k(const tfhe_params* p, const tfhe_rng_key* rk, const uint64_t bsk_seed[2],
                                    const uint64_t ksk_seed[2], const uint64_t* lwe_key, const uint64_t* glwe_key,
                                    uint64_t* bsk_bodies /* nullable */, uint64_t* ksk_bodies /* nullable */);
int tfhe_hip_seeded_lwe_list_k(uint32_t dim, uint32_t count, const uint64_t* key, int32_t noise_log2,
                               const tfhe_rng_key* rk, uint64_t stream0, const uint64_t seed[2],
                               const uint64_t* msgs /* nullable: encryptions of zero */, uint64_t* bodies);
int tfhe_hip_decompress_bsk(const tfhe_params* p, const uint64_t seed[2], const uint64_t* bodies, uint64_t* bsk);
int tfhe_hip_decompress_ksk(const tfhe_params* p, const uint64_t seed[2], const uint64_t* bodies, uint64_t* ksk);
int tfhe_hip_decompress_lwe_list(uint32_t dim, uint32_t count, const uint64_t seed[2], const uint64_t* bodies,
                                 uint64_t* out /* count x (dim + 1) */);
/* Seeded multi-bit bootstrapping keys (tfhe-rs SeededLweMultiBitBootstrapKey; restated, PARITY UNPINNED at the byte
 * level like every seeded path).  Bodies [n/g][2^g][L][k+1][N]: group q holds 2^g GGSWs, sigma = 0 .. 2^g - 1 (tfhe-rs
 * stores all 2^g, this engine keeps 2^g - 1); bit i of sigma belongs to key element g q + i (the convention of
 * tfhe_hip_mb_server_keygen) and GGSW (q, sigma) encrypts the indicator [(s_{gq+i})_i = bits of sigma], its rows in
 * tfhe-rs's form as tfhe_hip_seeded_server_keygen_k writes them (row c < k: -m g_l S_c, row k: m g_l).  Stream row
 * rho = ((q 2^g + sigma) L + l)(k+1) + c owns mask words rho k N ... of the seed's stream; the noise of GGSW
 * (q, sigma) comes from ChaCha stream 0x700000 + 16 q + sigma of the rng key.  The KSK of a multi-bit set is the
 * classic seeded KSK (tfhe_hip_seeded_server_keygen_k with bsk_bodies NULL).
 * tfhe_hip_decompress_bsk_mb is the host reference of the device route: it writes this engine's layout
 * [q][sigma - 1][l][c][j][N] (level-major, unlike the classic [i][c L + l]) and SKIPS sigma = 0, whose bodies are
 * ignored and whose mask words are stepped over in the stream.  Valid because sum_sigma indicator_sigma = 1, so
 * tfhe-rs's sum_sigma X^{t_sigma} GGSW_sigma [.] acc equals this engine's acc + sum_{sigma >= 1} (X^{t_sigma} - 1)
 * GGSW_sigma [.] acc up to noise.
 * Both refuse what tfhe_hip_load_keys_mb refuses: EINVAL for g outside {2, 3, 4} or n % g != 0, EUNSUPPORTED outside
 * FFT64, k = 1, N = 2048, PBS 23x1.  tfhe_hip_seeded_mb_bodies_len: (n / g) 2^g L (k+1) N, 0 for invalid arguments. */
size_t tfhe_hip_seeded_mb_bodies_len(const tfhe_params* p, uint32_t g);
int tfhe_hip_seeded_mb_server_keygen_k(const tfhe_params* p, uint32_t g, const tfhe_rng_key* rk,
                                       const uint64_t bsk_seed[2], const uint64_t* lwe_key, const uint64_t* glwe_key,
                                       uint64_t* bsk_bodies);
int tfhe_hip_decompress_bsk_mb(const tfhe_params* p, uint32_t g, const uint64_t seed[2], const uint64_t* bodies,
                               uint64_t* bsk_mb);
/* Encrypt count torus messages; ciphertext q uses ChaCha stream (stream0 + q) of the rng key (a fresh
 * entropy key per call, or one key with non-overlapping stream ranges).
 * Replaces the encrypt path of packages/luxfhejs/src/index.ts:127-141 (server-side /encrypt). */
int tfhe_hip_lwe_encrypt_k(uint32_t dim, const uint64_t* key, int32_t noise_log2, const tfhe_rng_key* rk,
                           uint64_t stream0, const uint64_t* msgs, size_t count, uint64_t* out);
int tfhe_hip_lwe_encrypt(uint32_t dim, const uint64_t* key, int32_t noise_log2, uint64_t seed,
                         uint64_t stream0, const uint64_t* msgs, size_t count, uint64_t* out);
/* phase = b - <a, s> (decryption before decoding); replaces /decrypt
 * (packages/hardhat-plugin/src/index.ts:71-75). */
int tfhe_hip_lwe_phase(uint32_t dim, const uint64_t* key, const uint64_t* ct, size_t count, uint64_t* out);
/* LUT builders.  Replaces ServerKey::generate_accumulator (ml/biometrics/notebooks/main.rs:65-68). */
int tfhe_hip_lut_constant(uint32_t N, uint64_t torus_value, uint64_t* lut);
int tfhe_hip_lut_from_table(uint32_t N, uint32_t msg_modulus, const uint64_t* table, uint64_t delta_out,
                            uint64_t* lut);

/* ---- device engine ------------------------------------------------------------------------
 * One engine spans ndev device "shards" (SURVEY §8b/§8e).  Each shard owns a HIP stream, a copy of the
 * keys and its workspaces.  Host-buffer calls (tfhe_hip_pbs, tfhe_hip_nand) split a batch into
 * contiguous slices, one per shard, run concurrently (one host thread per shard) and return when all
 * are done; the outputs are in input order.  Keys are uploaded once to shard 0 (pinned staging) and
 * broadcast to the others: RCCL (ncclCommInitAll + ncclBroadcast over xGMI, librccl loaded on first use)
 * when the ordinals are distinct, device copies when an ordinal repeats (a one-GPU box can run
 * devices = {0, 0} to exercise the split).  TFHE_HIP_BCAST=rccl|copy overrides the choice.
 * Stage-level entry points (blind_rotate, sample_extract, keyswitch, ms_reduce, ntt_*, fft_*) run on
 * shard 0.  Replaces the CPU worker pool of the reference's FHE service
 * (coprocessor-docker-compose.yml:97 --coprocessor-fhe-threads=8). */
int tfhe_hip_create(const tfhe_params* p, const int* devices, int ndev, tfhe_ctx** out);
void tfhe_hip_destroy(tfhe_ctx* ctx);
const char* tfhe_hip_last_error(void);
int tfhe_hip_device(const tfhe_ctx* ctx);          /* device of shard 0 */
int tfhe_hip_ndev(const tfhe_ctx* ctx);            /* number of shards */
int tfhe_hip_device_at(const tfhe_ctx* ctx, int i); /* device of shard i, -1 if out of range */
/* How the last key load reached shards 1..ndev-1: 0 = single shard, 1 = device copies, 2 = RCCL. */
int tfhe_hip_key_bcast_mode(const tfhe_ctx* ctx);
/* The key-load broadcast planner behind tfhe_hip_load_keys (host logic only, no device is touched), so the
 * N-rank call structure is testable without N GPUs.  policy: "rccl", "copy" or NULL / "" = auto (RCCL when
 * the ordinals are distinct and librccl is available, device / peer copies otherwise).  *mode as
 * tfhe_hip_key_bcast_mode.  mode 2: calls[i] = the rank issuing the i-th ncclBroadcast inside one
 * ncclGroupStart / ncclGroupEnd (root 0 first); mode 1: calls[i] = destination shard of the i-th copy from
 * shard 0.  Returns the number of calls (<= max_calls) or a negative error code. */
int tfhe_hip_bcast_plan(const int* devices, int ndev, const char* policy, int rccl_available, int* mode, int* calls,
                        int max_calls);

/* Upload standard-domain BSK and KSK from host memory through a pinned staging ring to shard 0,
 * broadcast them to every other shard, and convert them on each device (BSK to the transform domain,
 * KSK to the matrix-core byte planes).  Replaces the packages/kms key-loader role (pinned-HBM key
 * residency). */
int tfhe_hip_load_keys(tfhe_ctx* ctx, const uint64_t* bsk, size_t bsk_len, const uint64_t* ksk, size_t ksk_len);
/* Same, from DEVICE buffers on shard 0's device (e.g. after a torch.distributed broadcast of the keys). */
int tfhe_hip_load_keys_device(tfhe_ctx* ctx, const uint64_t* d_bsk, size_t bsk_len, const uint64_t* d_ksk,
                              size_t ksk_len);
/* The bootstrapping key alone: upload, broadcast to every shard and convert it as tfhe_hip_load_keys does, with no
 * keyswitching key (a tfhe-rs DecompressionKey holds none; a dummy KSK at n = 2048, N = 2048 would be 134 MB).
 * Replaces the key residency behind tfhe-rs DecompressionKey / programmable_bootstrap_lwe_ciphertext.  The ctx
 * is then "rotation-only": tfhe_hip_blind_rotate, tfhe_hip_bootstrap*, tfhe_hip_decompress* and tfhe_hip_br_kernel
 * work; every call that keyswitches (tfhe_hip_pbs*, tfhe_hip_nand, tfhe_hip_keyswitch) keeps returning
 * TFHE_HIP_ENOKEYS until a tfhe_hip_load_keys makes the ctx complete.  _device: d_bsk on shard 0's device. */
int tfhe_hip_load_bsk(tfhe_ctx* ctx, const uint64_t* bsk, size_t bsk_len);
int tfhe_hip_load_bsk_device(tfhe_ctx* ctx, const uint64_t* d_bsk, size_t bsk_len);

/* Multi-bit keys (tfhe_hip_mb_server_keygen*): upload, broadcast and convert like tfhe_hip_load_keys.  ksk == NULL
 * loads a rotation-only ctx (as tfhe_hip_load_bsk).  Afterwards every entry point that blind-rotates (pbs*,
 * pbs_many*, bootstrap*, blind_rotate, oprf*, expand_cast*, decompress*, lincomb_pbs_async) runs the multi-bit
 * kernel on every shard and tfhe_hip_br_kernel reports its name; a later tfhe_hip_load_keys / load_bsk restores the
 * classic path.  A loaded modulus-switch noise-reduction key is dropped: its pick is defined for the per-element
 * switch, so tfhe_hip_load_ms_key and tfhe_hip_ms_reduce return EUNSUPPORTED on a multi-bit ctx.  EUNSUPPORTED for
 * an NTT ctx or N = 1024; EINVAL for g outside {2, 3, 4}, n % g != 0 or a wrong length. */
int tfhe_hip_load_keys_mb(tfhe_ctx* ctx, uint32_t g, const uint64_t* bsk_mb, size_t bsk_mb_len,
                          const uint64_t* ksk /* nullable */, size_t ksk_len);
/* Grouping factor of the resident bootstrapping key: 1 = classic keys (or none), 2..4 = multi-bit. */
int tfhe_hip_grouping(const tfhe_ctx* ctx);

/* Seeded (compressed) keys loaded without a host decompression (the CompressedServerKey::decompress step of the
 * fhEVM coprocessor's tenant key cache, on the device): the HOST body buffers (layouts of the seeded section above)
 * go through the pinned ring to shard 0 and by the key broadcast to the other shards -- bodies, not expanded keys:
 * 1/(k+1) of the BSK words and 1/(n+1) of the KSK words -- and every shard regenerates the masks into its own
 * standard-domain buffers (tfhe_amd/csrc/seeded_keys.hip: AES-128-CTR as tfhe_hip_csprng_words, the key schedule once
 * per seed on the host), word for word what tfhe_hip_decompress_bsk / _bsk_mb / _ksk write; the conversion kernels of
 * tfhe_hip_load_keys follow unchanged.  The device copy of the bodies is released before the call returns.  State
 * transitions are those of the unseeded loaders: _seeded and _bsk_seeded restore the classic back end, _mb_seeded
 * (ksk_bodies NULL = rotation-only, ksk_seed then unused) drops a resident noise-reduction key.  FFT64 ctx only
 * (EUNSUPPORTED otherwise); EINVAL for a null argument, a wrong body count (bsk: n L (k+1) N or
 * tfhe_hip_seeded_mb_bodies_len; ksk: k N ks_level), g outside {2, 3, 4} or n % g != 0; EUNSUPPORTED for a multi-bit
 * load at N = 1024.  Every check precedes any change of the ctx: after a refused call the resident keys still work. */
int tfhe_hip_load_keys_seeded(tfhe_ctx* ctx, const uint64_t bsk_seed[2], const uint64_t* bsk_bodies,
                              size_t bsk_bodies_len, const uint64_t ksk_seed[2], const uint64_t* ksk_bodies,
                              size_t ksk_bodies_len);
int tfhe_hip_load_bsk_seeded(tfhe_ctx* ctx, const uint64_t seed[2], const uint64_t* bodies, size_t bodies_len);
int tfhe_hip_load_keys_mb_seeded(tfhe_ctx* ctx, uint32_t g, const uint64_t bsk_seed[2], const uint64_t* bsk_bodies,
                                 size_t bsk_bodies_len, const uint64_t ksk_seed[2] /* nullable with ksk_bodies */,
                                 const uint64_t* ksk_bodies /* nullable */, size_t ksk_bodies_len);
/* Device milliseconds of the last seeded key load on shard 0: upload of the bodies, expansion kernels, conversion
 * (a measurement aid, tools/seeded_load_bench.py; any pointer may be null). */
int tfhe_hip_seeded_load_stats(const tfhe_ctx* ctx, double* upload_ms, double* expand_ms, double* convert_ms);
/* Stage-level (the parity tests): the expansion kernels alone, through the launchers the loaders use, on shard 0.
 * out_host receives the standard-domain key (tfhe_hip_bsk_len / tfhe_hip_mb_bsk_len / tfhe_hip_ksk_len / count x
 * (dim + 1) words) FOLLOWED BY TFHE_HIP_SEEDED_GUARD_WORDS words of the device buffer behind it, which were filled
 * with 0xA5 bytes before the launch: a kernel that stays in bounds leaves them as they were.  _bsk: g = 1 classic
 * bodies, g in 2..4 multi-bit bodies, shape and n of the ctx; errors as the loaders. */
#define TFHE_HIP_SEEDED_GUARD_WORDS 64u
int tfhe_hip_seeded_expand_bsk(tfhe_ctx* ctx, uint32_t g, const uint64_t seed[2], const uint64_t* bodies,
                               uint64_t* out_host);
int tfhe_hip_seeded_expand_ksk(tfhe_ctx* ctx, const uint64_t seed[2], const uint64_t* bodies, uint64_t* out_host);
int tfhe_hip_seeded_expand_lwe_list(tfhe_ctx* ctx, uint32_t dim, uint32_t count, const uint64_t seed[2],
                                    const uint64_t* bodies, uint64_t* out_host);

/* Enable the modulus-switch noise reduction between keyswitch and blind rotation (order 1 only;
 * count = 0 disables).  Before each blind rotation the ciphertext gets the one zero whose
 * measure |E[err]| + r_sigma * sd(err) of the switch to 2N is best (tfhe-rs 1.x
 * improve_lwe_ciphertext_modulus_switch_noise_for_binary_key; exact rule in oracle/tfhe_oracle.h).
 * EUNSUPPORTED for order 0 parameter sets. */
int tfhe_hip_load_ms_key(tfhe_ctx* ctx, const uint64_t* zeros, uint32_t count, double bound, double r_sigma,
                         double input_variance);
/* The same from the seeded form of the zeros (bodies [count], tfhe_hip_seeded_lwe_list_k at dim = n): the rows
 * [count][n+1] are expanded and their element-major transpose is built on every shard's device.  Checks and refusals
 * of tfhe_hip_load_ms_key (EUNSUPPORTED on a multi-bit ctx, the 2 GiB scan window), EUNSUPPORTED for an NTT ctx. */
int tfhe_hip_load_ms_key_seeded(tfhe_ctx* ctx, const uint64_t seed[2], const uint64_t* bodies, uint32_t count,
                                double bound, double r_sigma, double input_variance);
/* Stage-level: the reduction alone on B small-key ciphertexts (B x (n+1)); picks (nullable, B
 * entries) receives the chosen zero index or -1. */
int tfhe_hip_ms_reduce(tfhe_ctx* ctx, const uint64_t* lwe_small, size_t B, uint64_t* out, int32_t* picks);

/* Full PBS of B ciphertexts: order 0 = blind-rotate -> sample-extract -> keyswitch.
 * luts: n_lut LUTs of N values; lut_index (nullable, B entries) picks the LUT per ciphertext.
 * Replaces ServerKey::keyswitch_programmable_bootstrap (ml/biometrics/notebooks/main.rs:71) and
 * the compute behind POST /evaluate (e2e/test/fhe.test.ts:141-157).  Host buffers, synchronous. */
int tfhe_hip_pbs(tfhe_ctx* ctx, const uint64_t* lwe_in, size_t B, const uint64_t* luts, size_t n_lut,
                 const uint32_t* lut_index, uint64_t* lwe_out);
/* Device buffers, enqueued on `stream` (hipStream_t; NULL = the shard's stream, TFHE_HIP_NULL_STREAM = the
 * device's legacy null stream, e.g. torch's default stream).  Inputs resident in HBM, on the device of the
 * shard that runs the batch: the first shard whose device holds d_lwe_in.  Calls on different streams
 * are ordered on the shard's workspaces by an event (a later call waits for the previous one's kernels).
 * What a call touches of the caller's memory (tests/test_gpu_device_buffers.py pins it with guard rows on every
 * blind-rotation kernel, both keyswitch kernels and both forms of the many-LUT extraction; the same holds for
 * tfhe_hip_pbs_many_async and tfhe_hip_bootstrap_async): it writes exactly the B rows of d_lwe_out (B * n_fn rows for
 * the many-LUT call) and nothing else; it reads rows 0 .. B - 1 of d_lwe_in and nothing past them (a padded workgroup
 * reruns row B - 1 and stores nothing), n_lut * N words of d_luts and B entries of d_lut_index.
 * Alignment: every kernel loads d_lwe_in and d_luts and stores d_lwe_out as single 8-byte words (4-byte halves at
 * most), because rows of n + 1 or kN + 1 words leave every second row of an odd length 8-byte aligned whatever the
 * base is.  The three pointers therefore need the natural 8-byte alignment of uint64_t and no more, d_lut_index 4
 * bytes.  The 16-byte loads of the many-LUT extraction read the ctx's own accumulator workspace (its launcher refuses
 * any other alignment), never a caller's buffer.  The guard-row tests run at the 16-byte-aligned bases a fresh
 * allocation gives. */
#define TFHE_HIP_NULL_STREAM ((void*)(intptr_t)-1)
int tfhe_hip_pbs_async(tfhe_ctx* ctx, const uint64_t* d_lwe_in, size_t B, const uint64_t* d_luts, size_t n_lut,
                       const uint32_t* d_lut_index, uint64_t* d_lwe_out, void* stream);
/* Many-LUT PBS: n_fn functions of each input from ONE blind rotation.  Replaces tfhe-rs
 * ServerKey::apply_many_lookup_table.  A many-LUT lays n_fn tables side by side in one accumulator and
 * output f is the sample extracted at degree f * stride; the caller guarantees that every input uses only
 * the first 1/n_fn of the message x carry space.  No builder of its own is needed (tfhe-rs
 * generate_many_lookup_table): the many-LUT over n_fn tables of msg_modulus / n_fn entries is
 * tfhe_hip_lut_from_table applied to their concatenation, with stride = N / n_fn; the half-box rotation is
 * unchanged.  lwe_out: B x n_fn x (io_dim + 1), ciphertext-major (row b * n_fn + f).  Requires n_fn >= 1,
 * stride >= 1, (n_fn - 1) * stride < N and B * n_fn <= 0x7FFFFFFF (EINVAL otherwise, before any device work).
 * Host buffers, synchronous, sharded like tfhe_hip_pbs. */
int tfhe_hip_pbs_many(tfhe_ctx* ctx, const uint64_t* lwe_in, size_t B, const uint64_t* luts, size_t n_lut,
                      const uint32_t* lut_index, uint32_t n_fn, uint32_t stride, uint64_t* lwe_out);
/* The same on device buffers (tfhe-rs apply_many_lookup_table on resident ciphertexts); stream and workspace
 * rules of tfhe_hip_pbs_async. */
int tfhe_hip_pbs_many_async(tfhe_ctx* ctx, const uint64_t* d_lwe_in, size_t B, const uint64_t* d_luts, size_t n_lut,
                            const uint32_t* d_lut_index, uint32_t n_fn, uint32_t stride, uint64_t* d_lwe_out,
                            void* stream);

/* Programmable bootstrap WITHOUT a keyswitch: blind rotation + sample extraction of B ciphertexts under the small
 * (dimension n) key, B x (n+1) in -> B x (kN+1) out under the GLWE key, for either `order`; no modulus-switch noise
 * reduction.  Replaces tfhe-rs programmable_bootstrap_lwe_ciphertext.  Needs the BSK only (tfhe_hip_load_bsk or
 * tfhe_hip_load_keys).  Host buffers, synchronous, sharded like tfhe_hip_pbs; timed in slot 0. */
int tfhe_hip_bootstrap(tfhe_ctx* ctx, const uint64_t* lwe_in, size_t B, const uint64_t* luts, size_t n_lut,
                       const uint32_t* lut_index, uint64_t* lwe_big_out);
/* The same on device buffers; stream and workspace rules of tfhe_hip_pbs_async. */
int tfhe_hip_bootstrap_async(tfhe_ctx* ctx, const uint64_t* d_lwe_in, size_t B, const uint64_t* d_luts, size_t n_lut,
                             const uint32_t* d_lut_index, uint64_t* d_lwe_big_out, void* stream);

/* Stage-level entry points (host buffers) used by the parity tests. */
/* acc_out: B x (k+1) x N values in the GLWE ring (Z_p for NTT, torus for FFT64) after the CMUX loop. */
int tfhe_hip_blind_rotate(tfhe_ctx* ctx, const uint64_t* lwe_in, size_t B, const uint64_t* luts, size_t n_lut,
                          const uint32_t* lut_index, uint64_t* acc_out);
/* acc (Z_p, B x (k+1)N) -> LWE under the GLWE key, converted to 2^64: B x (kN + 1). */
int tfhe_hip_sample_extract(tfhe_ctx* ctx, const uint64_t* acc, size_t B, uint64_t* lwe_big_out);
/* The extraction stage of tfhe-rs apply_many_lookup_table (extract_lwe_sample_from_glwe_ciphertext at
 * MonomialDegree(f * stride)): acc as above -> B x n_fn x (kN + 1), row b * n_fn + f = the sample at degree
 * f * stride, converted to 2^64 like tfhe_hip_sample_extract. */
int tfhe_hip_sample_extract_many(tfhe_ctx* ctx, const uint64_t* acc, size_t B, uint32_t n_fn, uint32_t stride,
                                 uint64_t* lwe_big_out);
/* B x (kN+1) -> B x (n+1). */
int tfhe_hip_keyswitch(tfhe_ctx* ctx, const uint64_t* lwe_big, size_t B, uint64_t* lwe_small_out);
/* Negacyclic NTT over Z_p of count polynomials of size N, in place, natural order:
 * A[j] = a(psi^(2j+1)), psi the primitive 2N-th root with psi^(2N/64) = 8.  ntt_inv includes 1/N. */
int tfhe_hip_ntt_fwd(tfhe_ctx* ctx, uint64_t* polys, size_t count);
int tfhe_hip_ntt_inv(tfhe_ctx* ctx, uint64_t* polys, size_t count);

/* FFT64 transform (N = 1024), natural order, for parity tests of the device FFT against
 * oracle/fft_oracle.c: fwd reads count x N torus values as int64, writes count x N/2 complex (re, im
 * doubles); inv reads count x N/2 complex and writes count x N doubles (no 1/M, no rounding).
 * EUNSUPPORTED unless the ctx was created with transform = TFHE_HIP_TRANSFORM_FFT64. */
int tfhe_hip_fft_fwd(tfhe_ctx* ctx, const uint64_t* polys, size_t count, double* out);
int tfhe_hip_fft_inv(tfhe_ctx* ctx, const double* in, size_t count, double* out);

/* Gate bootstrapping (FheBool NAND): out = PBS((0, 1/8) - c1 - c2, LUT == 1/8), B gates. */
int tfhe_hip_nand(tfhe_ctx* ctx, const uint64_t* c1, const uint64_t* c2, size_t B, uint64_t* out);

/* Batches of at most max_batch ciphertexts run the latency blind-rotate kernel (one ciphertext per
 * workgroup: 4.5x (N=1024) / 2.5x (N=2048) lower PBS latency — the lockstep levels of integer
 * circuits, single /evaluate requests, packages/luxfhejs/src/index.ts:56-141 call patterns); larger
 * batches the throughput kernel.  Defaults = the measured crossovers on MI355X (tools/latency_sweep.py,
 * tools/latency_sweep_fft.sh): NTT engine 1024 for N=1024 (55 vs 61 ms at B=1024, 69 vs 62 at 1280),
 * 512 for N=2048 (42 vs 53 ms at 512, 63 vs 53 at 768); FFT64 engine 512 for both N (PBS with the
 * latency kernel: 3.9 / 7.9 ms at N=1024 for up to 256 / 512 ciphertexts, 5.7 / 11.3 ms at N=2048;
 * batch kernel 14.5-15.5 ms up to 2048 ciphertexts at N=1024, 15.3-16.0 ms up to 1024 at N=2048);
 * 0 disables the latency kernel. */
int tfhe_hip_set_latency_batch(tfhe_ctx* ctx, size_t max_batch);
/* Name of the blind-rotate kernel the dispatch launches for a per-shard batch of `batch` ciphertexts under
 * the current latency threshold (e.g. "blind_rotate_fft_pair_kernel"), or NULL for a null ctx.  No reference
 * counterpart: a measurement aid, so a profile is matched to the kernel that actually ran (bench.py). */
const char* tfhe_hip_br_kernel(const tfhe_ctx* ctx, size_t batch);
/* Wait for all work on the ctx stream. */
int tfhe_hip_sync(tfhe_ctx* ctx);
/* Per-kernel device timing (HIP events recorded on the launch stream around every blind-rotate /
 * keyswitch launch).  reset clears the record; stats waits for the recorded events and returns the
 * summed milliseconds and the launch count.  which: 0 = blind rotate (+sample extract), 1 = keyswitch,
 * 2 = modulus-switch noise reduction, 3 = the ingest stage of a call: unpack / extract of a decompression, or the
 * expansion of a compact list.
 * Used by bench.py for the roofline figure. */
int tfhe_hip_timing_enable(tfhe_ctx* ctx, int enable);
int tfhe_hip_timing_reset(tfhe_ctx* ctx);
int tfhe_hip_timing_stats(tfhe_ctx* ctx, int which, double* total_ms, int* launches);

/* ---- LWE -> GLWE packing keyswitch and ciphertext compression ---------------
 * Replaces the reference's compression of result ciphertexts (ml/extensions/rust/src/compression.rs:
 * cpu_compress_ciphertexts_into_list :246-291 / cuda_compress_ciphertexts_into_single_glwe :190-240 ->
 * tfhe-rs par_keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext, then
 * CompressedModulusSwitchedGlweCiphertext::compress; extract :134-156).  Up to lwe_per_glwe LWEs
 * (dimension in_dim, native 2^64) are keyswitched into the coefficients 0, 1, ... of one GLWE
 * (k = out_k, N = out_N) under a fresh binary GLWE key; compression switches every stored coefficient
 * to storage_log bits and bit-packs them.  Exact rule: oracle/tfhe_oracle.h (or_pks_params). */
typedef struct tfhe_pks_params {
  uint32_t in_dim, out_k, out_N, base_log, level, lwe_per_glwe, storage_log;
  int32_t noise_log2;
} tfhe_pks_params;
/* PARAMS_8B_2048_NEW (ml/extensions/rust/src/fhext_classes.rs:98-112): in 2048, pks 2 x 2^14,
 * out k=1 N=2048, lwe_per_glwe 2048, storage 26 bits, noise 2^-48 */
#define TFHE_HIP_PKS_PRESET_ML2048 0
int tfhe_hip_pks_params_preset(int preset, tfhe_pks_params* out);
size_t tfhe_hip_pksk_len(const tfhe_pks_params* pp); /* in_dim * level * (out_k+1) * out_N u64 */
/* output GLWE key (out_k*out_N bits, ChaCha stream 4) and PKSK [j][l][(k+1)N] (stream 0x300000+j) */
int tfhe_hip_pks_keygen(const tfhe_pks_params* pp, uint64_t seed, const uint64_t* in_key, uint64_t* out_key,
                        uint64_t* pksk /* nullable */);
/* the same from a 192-bit rng key (tfhe_hip_rng_key_entropy for production keys; the seeded form above
 * is tfhe_hip_rng_key_from_seed(seed) and exists for reproducible tests) */
int tfhe_hip_pks_keygen_k(const tfhe_pks_params* pp, const tfhe_rng_key* rk, const uint64_t* in_key,
                          uint64_t* out_key, uint64_t* pksk /* nullable */);
typedef struct tfhe_pks_ctx tfhe_pks_ctx;
int tfhe_hip_pks_create(const tfhe_pks_params* pp, int device, tfhe_pks_ctx** out);
/* Waits for every call still in flight on the ctx, on a caller's stream too, before it frees the ctx's buffers. */
void tfhe_hip_pks_destroy(tfhe_pks_ctx* ctx);
/* Waits for every call still in flight on the ctx before it rewrites the resident key. */
int tfhe_hip_pks_load_key(tfhe_pks_ctx* ctx, const uint64_t* pksk, size_t len);
/* count LWEs (count x (in_dim+1)) -> ceil(count / lwe_per_glwe) GLWEs ((k+1) x N each); GLWE g holds
 * LWEs g*lwe_per_glwe ... in coefficients 0, 1, ...  Host buffers, synchronous. */
int tfhe_hip_pks_pack(tfhe_pks_ctx* ctx, const uint64_t* lwes, size_t count, uint64_t* glwes);
/* Device buffers, enqueued on `stream` (NULL = the ctx stream, TFHE_HIP_NULL_STREAM = the null stream).  The digit
 * and T workspaces and the key are shared by every call on the ctx: calls on different streams, host calls included,
 * are ordered on them by an event (a later call waits for the previous one's kernels on its own stream, and the host
 * waits for them before it regrows a workspace), so a call may follow another at once, on any stream, without a
 * synchronisation by the caller. */
int tfhe_hip_pks_pack_async(tfhe_pks_ctx* ctx, const uint64_t* d_lwes, size_t count, uint64_t* d_glwes, void* stream);
size_t tfhe_hip_pks_packed_words(const tfhe_pks_params* pp, uint32_t bodies);
int tfhe_hip_pks_compress(const tfhe_pks_params* pp, const uint64_t* glwe, uint32_t bodies, uint64_t* packed);
int tfhe_hip_pks_extract(const tfhe_pks_params* pp, const uint64_t* packed, uint32_t bodies, uint64_t* glwe);
/* client-side decryption of a native GLWE: body - sum_c mask_c * S_c (N values) */
int tfhe_hip_glwe_phase(uint32_t k, uint32_t N, const uint64_t* key, const uint64_t* glwe, uint64_t* out);

/* ---- decompression: compressed GLWEs back into compute-ready LWEs -----------------------------
 * Replaces tfhe-rs CompressedCiphertextList::get / DecompressionKey::unpack (the return half of the reference's
 * compression surface, ml/extensions/rust/src/compression.rs:134-291): unpack the stored bits, sample-extract
 * coefficient i, blind-rotate under a key from the post-packing key to the compute GLWE key, sample-extract.
 * A list of `count` ciphertexts is the concatenation of G = ceil(count / lwe_per_glwe) compressed GLWEs exactly as
 * tfhe_hip_pks_compress writes them: group g holds lwe_per_glwe bodies (the last one the remainder) and is
 * tfhe_hip_pks_packed_words(pp, bodies_g) words long; spare high bits of a group's last word are ignored.
 *
 * Stage-level (tfhe-rs: unpack + extract_lwe_sample_from_glwe_ciphertext; needs no key): row q = g * lwe_per_glwe
 * + i of lwes_out (count x (out_k*out_N + 1)) is the LWE of coefficient i of group g under the post-packing key,
 * stored values moved to the top of the word (<< (64 - storage_log)).  EINVAL if packed_words is not the sum
 * above; EUNSUPPORTED for out_N > 4096; count == 0 returns OK.  _async: device pointers and a stream, rules of
 * tfhe_hip_pks_pack_async. */
int tfhe_hip_pks_unpack_extract(tfhe_pks_ctx* ctx, const uint64_t* packed, size_t packed_words, size_t count,
                                uint64_t* lwes_out);
int tfhe_hip_pks_unpack_extract_async(tfhe_pks_ctx* ctx, const uint64_t* d_packed, size_t packed_words, size_t count,
                                      uint64_t* d_lwes_out, void* stream);
/* The whole decompression on a ctx whose n = pp->out_k * pp->out_N and whose BSK (tfhe_hip_load_bsk) goes from the
 * post-packing key to the ctx GLWE key: unpack / extract into a shard workspace (timed in slot 3), then
 * tfhe_hip_bootstrap (slot 0).  lwe_big_out: count x (kN + 1); lut_index: count entries or null.  EINVAL unless pp
 * is valid, packed_words fits and pp->out_k * pp->out_N == n; ENOKEYS without a BSK; count <= 0x7FFFFFFF; all checks
 * run before any device work.  The host form runs on shard 0; a multi-shard caller hands whole groups to the
 * async form (device buffers on the shard's device; stream and workspace rules of tfhe_hip_pbs_async). */
int tfhe_hip_decompress(tfhe_ctx* ctx, const tfhe_pks_params* pp, const uint64_t* packed, size_t packed_words,
                        size_t count, const uint64_t* luts, size_t n_lut, const uint32_t* lut_index,
                        uint64_t* lwe_big_out);
int tfhe_hip_decompress_async(tfhe_ctx* ctx, const tfhe_pks_params* pp, const uint64_t* d_packed, size_t packed_words,
                              size_t count, const uint64_t* d_luts, size_t n_lut, const uint32_t* d_lut_index,
                              uint64_t* d_lwe_big_out, void* stream);

/* ---- compact ciphertext lists: expansion and casting ------------------------------------------
 * Replaces tfhe-rs CompactCiphertextList::expand and the cast that follows it (KeySwitchingKey, then one PBS per
 * radix block) on the ingest side of the fhEVM coprocessor: every user input arrives as ONE compact list under the
 * network's CompactPublicKey (sdk/relayer/src/sdk/encrypt.ts:97-148,185, build_with_proof_packed; fixtures
 * sdk/relayer/src/test/v1/ciphertext.ts:1, src/test/assets/input-proof-payload-{1,2,3}.json).  The proof is not
 * verified here.  `list` is the LWE compact list's data Vec<u64> in tfhe-rs order: bins x lwe_dim mask words,
 * bins = ceil(count / lwe_dim) (every bin of up to lwe_dim ciphertexts shares one mask polynomial M), then count
 * body words.  Output row r is list entry q = r / rep, in bin q / lwe_dim at degree i = q % lwe_dim:
 *   a[k] = M[k + i + 1 - lwe_dim] (k + i + 1 >= lwe_dim),   a[k] = -M[k + i + 1] (otherwise),   b = bodies[q]
 * rep = 1 is the plain expansion; rep = 2 gives one row per radix block of a packed list (two blocks per LWE), and
 * rows (anything in 0 .. count * rep) cuts the last entry short for an odd block count.
 * lwe_dim: a power of two in 8 .. 4096 (EUNSUPPORTED for a larger power of two, EINVAL otherwise); EINVAL if
 * list_words is not tfhe_hip_compact_list_words, rep == 0, rows > count * rep, rows > 0x7FFFFFFF, or a buffer is
 * null when rows > 0; rows == 0 returns OK; count == 0 is valid only with rows == 0 and list_words == 0.  Every
 * check runs before any device work. */
/* bins * lwe_dim + count, or 0 if lwe_dim is not a power of two in 8..4096 or count == 0 (host only) */
size_t tfhe_hip_compact_list_words(uint32_t lwe_dim, size_t count);
/* Stage-level: the expansion alone (tfhe_amd/csrc/expand.hip), needs no key; timed in slot 3.  lwes_out: rows x
 * (lwe_dim + 1).  The host form runs on shard 0; _async: device pointers, on the shard whose device holds d_list,
 * enqueued on `stream` (rules of tfhe_hip_pbs_async). */
int tfhe_hip_expand_compact(tfhe_ctx* ctx, const uint64_t* list, size_t list_words, uint32_t lwe_dim, size_t count,
                            uint32_t rep, size_t rows, uint64_t* lwes_out);
int tfhe_hip_expand_compact_async(tfhe_ctx* ctx, const uint64_t* d_list, size_t list_words, uint32_t lwe_dim,
                                  size_t count, uint32_t rep, size_t rows, uint64_t* d_lwes_out, void* stream);
/* Expansion into a shard workspace (slot 3), then the ctx's full PBS in its `order` (keyswitch with the loaded KSK --
 * for ingest, the casting key compact-PKE key -> small key -- optional MS noise reduction, blind rotation; slots 1,
 * 2, 0).  The list's dimension is tfhe_hip_io_dim(params): EINVAL if that is not an allowed lwe_dim.  luts / n_lut /
 * lut_index (rows entries or null) as tfhe_hip_pbs; lwe_out: rows x (io_dim + 1).  ENOKEYS unless a full key set is
 * loaded (a rotation-only ctx is refused like tfhe_hip_pbs); EINVAL for n_lut == 0 or a host lut_index entry >=
 * n_lut.  The host form runs on shard 0; a multi-shard caller hands whole lists to the async form (device buffers on
 * the shard's device; stream and workspace rules of tfhe_hip_pbs_async). */
int tfhe_hip_expand_cast(tfhe_ctx* ctx, const uint64_t* list, size_t list_words, size_t count, uint32_t rep,
                         size_t rows, const uint64_t* luts, size_t n_lut, const uint32_t* lut_index,
                         uint64_t* lwe_out);
int tfhe_hip_expand_cast_async(tfhe_ctx* ctx, const uint64_t* d_list, size_t list_words, size_t count, uint32_t rep,
                               size_t rows, const uint64_t* d_luts, size_t n_lut, const uint32_t* d_lut_index,
                               uint64_t* d_lwe_out, void* stream);

/* ---- oblivious pseudo-random ciphertexts from a seed (fhEVM rand / randBounded) ------------------
 * tfhe-rs ServerKey::generate_oblivious_pseudo_random* (the fheRand / fheRandBounded operators,
 * tests/fhevm-suite/e2e/test/operatorsPrices.json:439-468): a 128-bit seed expands through the AES-CTR CSPRNG into
 * the mask of an LWE ciphertext under the small key with body 0, whose phase nobody without the secret key knows;
 * a blind rotation with a staircase LUT and one plaintext addition turn that phase into an encryption of
 * random_bits uniform bits.  The masks are generated on the device (tfhe_amd/csrc/csprng.hip): a request uploads
 * 16 bytes per row.  PARITY UNPINNED at the byte level, as every seeded path here (the reference mount holds no
 * OPRF vector): the conventions are restated from tfhe-rs and are, all arithmetic mod 2^64,
 *   row mask     row seed s = (lo, hi): mask = words 0 .. n-1 of the seed's stream (tfhe_hip_csprng_words(s, 0, n)),
 *                body 0, i.e. tfhe_hip_decompress_lwe_list(n, 1, s, {0})
 *   block seeds  block j of a request with parent seed S uses (lo, hi) = words (2j, 2j + 1) of S's stream (tfhe-rs
 *                DeterministicSeeder: 16 consecutive stream bytes per seed, little endian)
 *   LUT          p = 2^random_bits, delta = 2^(64 - full_bits), 1 <= random_bits < full_bits <= 63, p <= 2N:
 *                lut[x] = (2 floor(x / (2N / p)) + 1) delta / 2 for x < N, post_add = (p - 1) delta / 2, no half-box
 *                rotation (tfhe_hip_lut_oprf)
 *   result       with x = (-sum a~_i s_i) mod 2N, a~ the standard modulus switch of the mask (no noise reduction),
 *                row r encrypts v delta: v = floor(x / (2N / p)) + p / 2 if x < N, else
 *                v = p / 2 - 1 - floor((x - N) / (2N / p))
 *   gate bits    LUT = tfhe_hip_lut_constant(N, 2^61), post_add = 0: the bit is true iff x < N
 * Pipeline: order 1 (KS -> PBS, P-FHEVM): masks -> blind rotation -> sample extraction -> post-add, no keyswitch and
 * no modulus-switch noise reduction: rows of kN + 1 words, the BSK alone suffices (a rotation-only ctx works).
 * Order 0 (PBS -> KS, P-GATE): masks -> the full PBS (rotation, extraction, keyswitch) -> post-add: rows of n + 1
 * words, both keys.  Either way a row is io_dim + 1 words.  Timing: the mask kernel in slot 3, then the slots of
 * the PBS. */
/* host: the LUT (N words) and post-add of the convention above; EINVAL for N not a power of two, random_bits == 0,
 * random_bits >= full_bits, full_bits > 63 or 2^random_bits > 2N */
int tfhe_hip_lut_oprf(uint32_t N, uint32_t random_bits, uint32_t full_bits, uint64_t* lut, uint64_t* post_add);
/* Stage-level: the mask kernel alone, host buffers, shard 0, needs no keys.  out: rows x dim, row r = words
 * first_word .. first_word + dim - 1 of the stream of seed (seeds[2r], seeds[2r + 1]).  EINVAL for a null buffer,
 * dim == 0, rows > 0x7FFFFFFF, rows * ceil(dim / 1022) > 0x7FFFFFFF or first_word + dim > 2^60; rows == 0
 * returns OK */
int tfhe_hip_csprng_rows(tfhe_ctx* ctx, const uint64_t* seeds, size_t rows, uint64_t first_word, uint32_t dim,
                         uint64_t* out);
/* _async: device pointers, on the shard whose device holds d_seeds, enqueued on `stream` (no workspace is used).
 * Row r starts at d_out + r * row_stride (row_stride >= dim, EINVAL otherwise); words dim .. row_stride - 1 of a row
 * are not written. */
int tfhe_hip_csprng_rows_async(tfhe_ctx* ctx, const uint64_t* d_seeds, size_t rows, uint64_t first_word, uint32_t dim,
                               size_t row_stride, uint64_t* d_out, void* stream);
/* seeds: rows x 2; luts: n_lut x N with post_adds[n_lut] added to the body of every row that uses the LUT;
 * lut_index (rows entries, or null = LUT 0) as tfhe_hip_pbs; lwe_out: rows x (io_dim + 1).  Every check precedes
 * device work: EINVAL for a null buffer, n_lut == 0, a host lut_index entry >= n_lut or rows > 0x7FFFFFFF; ENOKEYS
 * without a BSK, and in order 0 without the KSK; rows == 0 returns OK.  The host form slices the rows over the
 * shards (outputs in seed order); _async: device pointers, on the shard whose device holds d_seeds, enqueued on
 * `stream` (stream and workspace rules of tfhe_hip_pbs_async; a device lut_index is trusted as there). */
int tfhe_hip_oprf(tfhe_ctx* ctx, const uint64_t* seeds, size_t rows, const uint64_t* luts, const uint64_t* post_adds,
                  size_t n_lut, const uint32_t* lut_index, uint64_t* lwe_out);
int tfhe_hip_oprf_async(tfhe_ctx* ctx, const uint64_t* d_seeds, size_t rows, const uint64_t* d_luts,
                        const uint64_t* d_post_adds, size_t n_lut, const uint32_t* d_lut_index, uint64_t* d_lwe_out,
                        void* stream);

/* ---- sparse linear combinations of LWE rows: the linear part of a radix circuit level -----------------------
 * tfhe-rs lwe_ciphertext_add_assign / lwe_ciphertext_cleartext_mul_assign / lwe_ciphertext_plaintext_add_assign
 * (what shortint's unchecked_add, unchecked_scalar_mul and the bivariate 4x + y of apply_bivariate_lookup_table
 * reduce to; the reference's call site of a server-side operation is ml/extensions/rust/src/ml.rs:88), applied to
 * a whole circuit level at once (tfhe_amd/csrc/lincomb.hip).  Output row r of `dim` words is, mod 2^64,
 *   out[r][j] = sum over t in row_start[r] .. row_start[r + 1] - 1 of term_coef[t] * B_t[j],  j < dim
 *   out[r][dim - 1] += bias[r]
 * with B_t row term_row[t] of source buffer term_buf[t].  A row without terms is a trivial ciphertext (zero mask,
 * body bias[r]); a source may repeat within a row and across rows; rows of any dim are 8-byte aligned only.
 * row_start (rows + 1 entries), term_buf, term_row (u32), term_coef (u64) and bias (u64, null = none) are HOST
 * arrays in every form: the library checks them, resolves each term to an address and stages the result through
 * pinned memory of its own, so no kernel sees an address that was not checked.  Every check precedes device work:
 * EINVAL for a null ctx or buffer, dim == 0, row_start[0] != 0, a decreasing row_start, term_buf[t] >= n_buf,
 * term_row[t] >= buf_rows[term_buf[t]], rows > 0x7FFFFFFF (the term count is a u32 by construction), or an output
 * range that overlaps a source buffer; rows == 0 returns OK and launches nothing.  Needs no key.  Timing: slot 3. */
/* host form: one source buffer src of src_rows x dim words (the terms have no term_buf), out: rows x dim; shard 0 */
int tfhe_hip_lwe_lincomb(tfhe_ctx* ctx, uint32_t dim, const uint64_t* src, size_t src_rows, const uint32_t* row_start,
                         const uint32_t* term_row, const uint64_t* term_coef, const uint64_t* bias, size_t rows,
                         uint64_t* out);
/* _async: d_bufs is a HOST array of n_buf device base pointers, buffer b holding buf_rows[b] x dim words; d_out:
 * rows x dim on the device, on the shard whose device holds it; enqueued on `stream` (stream rules of
 * tfhe_hip_pbs_async; the staged description is a workspace of the shard and ordered as there). */
int tfhe_hip_lwe_lincomb_async(tfhe_ctx* ctx, uint32_t dim, const uint64_t* const* d_bufs, const size_t* buf_rows,
                               size_t n_buf, const uint32_t* row_start, const uint32_t* term_buf,
                               const uint32_t* term_row, const uint64_t* term_coef, const uint64_t* bias, size_t rows,
                               uint64_t* d_out, void* stream);
/* The same map with dim = io_dim + 1 into a workspace of the ctx, then the PBS of tfhe_hip_pbs_async on the
 * assembled rows, in one call: d_lwe_out: rows x (io_dim + 1).  Checks of both; ENOKEYS without keys.  d_lwe_out is
 * written only after the assembly has read its sources. */
int tfhe_hip_lincomb_pbs_async(tfhe_ctx* ctx, const uint64_t* const* d_bufs, const size_t* buf_rows, size_t n_buf,
                               const uint32_t* row_start, const uint32_t* term_buf, const uint32_t* term_row,
                               const uint64_t* term_coef, const uint64_t* bias, size_t rows, const uint64_t* d_luts,
                               size_t n_lut, const uint32_t* d_lut_index, uint64_t* d_lwe_out, void* stream);

/* ---- switch-and-squash: noise squashing to a 128-bit LWE ----------------------
 * fhEVM's sns-worker (coprocessor-docker-compose.yml:124-140) turns each 64-bit P-FHEVM ciphertext into
 * a Z_2^128 LWE with tiny noise for threshold decryption: keyswitch to the small key, modulus-switch
 * noise reduction (tfhe_hip_ms_reduce), then a PBS with a BSK under a 128-bit GLWE key (k=2, N=2048,
 * 2^24 x 3) and the identity LUT.  The GLWE ring is the native 2^128 torus (as tfhe-rs): a coefficient
 * is one u128 word, a polynomial two u64 planes [lo][N], [hi][N]; rule: oracle/sns_oracle.c.
 * Output: (k*N + 1) x (lo, hi) u64 per ciphertext. */
typedef struct tfhe_sns_params {
  uint32_t n, k, N, base_log, level;
  int32_t noise_log2; /* Gaussian noise round(N(0,1) * 2^(64 + x)) on the 128-bit bodies */
} tfhe_sns_params;
#define TFHE_HIP_SNS_PRESET_FHEVM 0 /* n = 918 (P-FHEVM small key), k = 2, N = 2048, 2^24 x 3, noise 2^30 */
int tfhe_hip_sns_params_preset(int preset, tfhe_sns_params* out);
size_t tfhe_hip_sns_bsk_len(const tfhe_sns_params* sp); /* n*(k+1)L*(k+1)*2*N: [i][c*L+l][j][lo, hi][N] */
/* 128-bit GLWE key (k*N bits, ChaCha stream 5) and BSK (stream 0x400000 + i) for the small LWE key */
int tfhe_hip_sns_keygen(const tfhe_sns_params* sp, uint64_t seed, const uint64_t* lwe_key, uint64_t* glwe_key,
                        uint64_t* bsk /* nullable */);
/* the same from a 192-bit rng key (OS entropy for production keys) */
int tfhe_hip_sns_keygen_k(const tfhe_sns_params* sp, const tfhe_rng_key* rk, const uint64_t* lwe_key,
                          uint64_t* glwe_key, uint64_t* bsk /* nullable */);
typedef struct tfhe_sns_ctx tfhe_sns_ctx;
int tfhe_hip_sns_create(const tfhe_sns_params* sp, int device, tfhe_sns_ctx** out);
void tfhe_hip_sns_destroy(tfhe_sns_ctx* ctx);
/* Loading rounds every key word (read as a signed 128-bit integer) to the nearest multiple of 2^16
 * (oracle: or_sns_bsk_round; ~2^20 of extra phase noise beside the key's 2^30).  The external product
 * splits the rounded key into five limbs, the balanced low 48 bits and four balanced 16-bit limbs, and
 * computes each digit x limb convolution as an f64 FFT product, exact for the 16-bit limbs
 * (n x 9 x 3 x 5 x 1024 complex of key spectra: 2.03 GB at n = 918).  Waits for every call still in
 * flight on the ctx before it rewrites the resident key. */
int tfhe_hip_sns_load_key(tfhe_sns_ctx* ctx, const uint64_t* bsk, size_t len);
/* B small-key ciphertexts (B x (n+1)) -> B x (k*N+1) x 2 u64; identity LUT over msg_modulus values
 * (a divisor of N; EINVAL otherwise, before any device work).  Host buffers, synchronous. */
int tfhe_hip_sns_squash(tfhe_sns_ctx* ctx, const uint64_t* lwe_small, size_t B, uint32_t msg_modulus, uint64_t* out);
/* Device buffers, enqueued on `stream` (NULL = the ctx's stream, TFHE_HIP_NULL_STREAM = the legacy null
 * stream), in chunks of TFHE_HIP_SNS_CHUNK (512) ciphertexts.  The accumulators, spectra and the LUT are shared
 * by every call on the ctx: calls on different streams, host calls included, are ordered on them by an event (a
 * later call waits for the previous one's kernels on its own stream, and the host waits for them before it
 * rewrites the LUT for another msg_modulus or regrows a workspace), so a call may follow another at once,
 * on any stream, without a synchronisation by the caller. */
int tfhe_hip_sns_squash_async(tfhe_sns_ctx* ctx, const uint64_t* d_lwe_small, size_t B, uint32_t msg_modulus,
                              uint64_t* d_out, void* stream);
/* stage-level (parity tests): accumulator after the CMUX loop, B x (k+1) x (lo, hi) x N words */
int tfhe_hip_sns_blind_rotate(tfhe_sns_ctx* ctx, const uint64_t* lwe_small, size_t B, uint32_t msg_modulus,
                              uint64_t* acc_out);
/* client: phase b - <a, s> mod 2^128 of count squashed ciphertexts -> (lo, hi) pairs */
int tfhe_hip_sns_phase(const tfhe_sns_params* sp, const uint64_t* glwe_key, const uint64_t* cts, size_t count,
                       uint64_t* out);

/* ---- the seeded (compressed) squashing key: bodies + a 128-bit seed, DESIGN §7h'' --------------
 * The form in which a tenant's CompressedServerKey carries the noise-squashing key (tfhe-rs
 * CompressedNoiseSquashingKey: a SeededLweBootstrapKey over u128).  PARITY UNPINNED at the byte level, as every
 * seeded path here: the stream and the order below restate tfhe-csprng / tfhe-rs, with no key file to compare with.
 *   The 128-bit mask stream: u128 mask word w of a seed is bytes 16 w + 1 .. 16 w + 16 of the seed's AES-CTR table,
 *   little endian (the start at byte 1 of tfhe_hip_csprng_words), so lo = word 2 w and hi = word 2 w + 1 of
 *   tfhe_hip_csprng_words: block w less its byte 0, plus byte 0 of block w + 1.  tfhe_hip_csprng_words128 writes
 *   words first_word .. as (lo, hi) pairs.
 *   Bodies [n][L][k+1][N] u128 words as (lo, hi) u64 pairs (the bytes of a Vec<u128>), n L (k+1) 2 N words
 *   (tfhe_hip_sns_seeded_bodies_len; 0 for parameters outside the device kernels).  Stream row rho = (i L + l)(k+1) + c,
 *   level l = 0 most significant, owns u128 mask words rho k N .. (polynomial j, then coefficient t).  Rows are in
 *   tfhe-rs's GGSW form (row c < k: -s_i g_l S_c in the body, row k: s_i g_l on body coefficient 0,
 *   g_l = 2^(128 - base_log (l + 1))); noise from the Gaussian sampler of tfhe_hip_sns_keygen, GGSW i on ChaCha
 *   stream 0x800000 + i; the GLWE key is that of tfhe_hip_sns_keygen (stream 5).
 * tfhe_hip_sns_decompress_bsk writes the loader's [i][c*L+l][j][lo, hi][N] layout on the host: the host route
 * (followed by tfhe_hip_sns_load_key) and the CPU reference, word for word, of the device expansion. */
size_t tfhe_hip_sns_seeded_bodies_len(const tfhe_sns_params* sp);
int tfhe_hip_sns_seeded_keygen(const tfhe_sns_params* sp, uint64_t rng_seed, const uint64_t seed[2],
                               const uint64_t* lwe_key, uint64_t* glwe_key, uint64_t* bodies /* nullable */);
int tfhe_hip_sns_seeded_keygen_k(const tfhe_sns_params* sp, const tfhe_rng_key* rk, const uint64_t seed[2],
                                 const uint64_t* lwe_key, uint64_t* glwe_key, uint64_t* bodies /* nullable */);
int tfhe_hip_sns_decompress_bsk(const tfhe_sns_params* sp, const uint64_t seed[2], const uint64_t* bodies,
                                uint64_t* bsk);
int tfhe_hip_csprng_words128(const uint64_t seed[2], uint64_t first_word, size_t count, uint64_t* out_pairs);
/* tfhe_hip_sns_load_key from the seeded form: the HOST bodies go up in chunks of whole GGSWs (75 = 2025 polynomials;
 * TFHE_HIP_SNS_SEEDED_CHUNK, read at every load, sets the GGSWs per chunk), a HIP kernel
 * (tfhe_amd/csrc/seeded_keys128.hip) regenerates the masks into the staging buffer in the loader's layout, and the
 * conversion of tfhe_hip_sns_load_key follows on the same stream: a third of the bytes travel and no host AES runs.
 * The resident key equals that of tfhe_hip_sns_decompress_bsk + tfhe_hip_sns_load_key bit for bit.  EINVAL for a null
 * argument or len != tfhe_hip_sns_seeded_bodies_len, before any change to the ctx; a refused load, or one that cannot
 * allocate its buffers, leaves the resident key usable.  Waits for every call still in flight on the ctx. */
int tfhe_hip_sns_load_key_seeded(tfhe_sns_ctx* ctx, const uint64_t seed[2], const uint64_t* bodies, size_t len);
/* Device milliseconds of the last seeded load: upload of the bodies, expansion kernels, conversion (a measurement
 * aid, tools/sns_seeded_load_bench.py; any pointer may be null). */
int tfhe_hip_sns_seeded_load_stats(const tfhe_sns_ctx* ctx, double* upload_ms, double* expand_ms, double* convert_ms);
/* Test-facing, in the manner of tfhe_hip_seeded_expand_bsk: the loader's chunks through the loader's launcher into a
 * fresh device buffer; out_host receives tfhe_hip_sns_bsk_len words FOLLOWED BY TFHE_HIP_SEEDED_GUARD_WORDS words of
 * the device buffer behind them, which were filled with 0xA5 bytes before the launch. */
int tfhe_hip_sns_seeded_expand_bsk(tfhe_sns_ctx* ctx, const uint64_t seed[2], const uint64_t* bodies,
                                   uint64_t* out_host);

/* ---- compression of squashed ciphertexts: packing keyswitch over the 2^128 torus ---------------
 * The stored form of fhEVM's sns-worker output (the ct128 bucket, coprocessor-docker-compose.yml:124-140;
 * tfhe-rs CompressedSquashedNoiseCiphertextList): up to lwe_per_glwe squashed LWEs (dimension in_dim, words of
 * Z_2^128) are keyswitched into the coefficients 0, 1, ... of one 128-bit GLWE under a fresh binary key
 * (NoiseSquashingCompressionKey), then the mask and one body per ciphertext are bit-packed.  This is the rule of
 * tfhe_hip_pks_* widened to Z_2^128; kernels tfhe_amd/csrc/sns_pks.hip.
 *
 * Validity (EINVAL otherwise): in_dim % 16 == 0 (> 0); out_k > 0; out_N a power of two >= 32; (out_k+1)*out_N % 64
 * == 0; 2 <= base_log <= 63; level >= 1; base_log*level <= 127; 1 <= lwe_per_glwe <= out_N; 2 <= storage_log <= 128;
 * -64 < noise_log2 < 0.
 * Layouts (those of tfhe_hip_sns_*): an LWE is (in_dim+1) pairs (lo, hi), as tfhe_hip_sns_squash writes them; a
 * polynomial is two planes [lo][N], [hi][N]; a GLWE is (out_k+1) polynomials; the key is [j][l][c][lo, hi][N],
 * in_dim*level*(out_k+1)*2*out_N words.
 * Digits of a mask word a (u128), prec = base_log*level, B = 2^base_log:
 *   state = ((a >> (128 - prec - 1)) + 1) >> 1, masked to prec bits;
 *   for l = level-1 ... 0:  res = state & (B-1);  state >>= base_log;
 *                           carry = ((((res - 1) | state) & res) >> (base_log - 1)) & 1;
 *                           state += carry;  digit_l = res - carry*B
 * Pack of the cnt <= lwe_per_glwe LWEs of one group (group g takes LWEs g*lwe_per_glwe ...):
 *   T_d = sum_{j,l} digit_{d,j,l} * PKSK[j][l]  (coefficient-wise, mod 2^128)
 *   out = sum_d X^d * ((0, ..., 0, b_d) - T_d)  (negacyclic, mod 2^128)
 * Key: the output key is out_k*out_N bits of ChaCha stream 6; row j comes from stream 0x500000 + j.  PKSK[j][l]
 * encrypts in_key[j] * 2^(128 - base_log*(l+1)) at coefficient 0: masks uniform (lo word, then hi word, per
 * coefficient), then one Gaussian integer round(N(0,1) * 2^(64 + noise_log2)) per body coefficient,
 * body = sum_c mask_c (*) S_c + e + m.
 * Stored form: out_k*out_N mask values, then `bodies` body values; for storage_log s < 128 a value is
 * ((x >> (128 - s - 1)) + 1) >> 1 mod 2^s, for s = 128 the word itself; values are packed LSB-first into
 * ceil(values * s / 64) u64 words (a value may span three words).  Extraction puts each value back at the top of
 * its word (<< (128 - s)) and zeroes the unused body coefficients. */
typedef struct tfhe_sns_pks_params {
  uint32_t in_dim, out_k, out_N, base_log, level, lwe_per_glwe, storage_log;
  int32_t noise_log2;
} tfhe_sns_pks_params;
/* PARITY UNPINNED.  in_dim 4096 (the squashing key's k*N), 2^61 x 1 level, out k = 6, N = 1024, 128 LWEs per GLWE,
 * storage 128 bits, noise 2^2: tfhe-rs NOISE_SQUASHING_COMP_PARAM_MESSAGE_2_CARRY_2_KS_PBS_TUNIFORM_2M128 restated
 * from memory (no copy to compare with); tfhe-rs draws the key noise from TUniform(3), this engine from its Gaussian
 * sampler at std 4, as for the squashing key. */
#define TFHE_HIP_SNS_PKS_PRESET_FHEVM 0
int tfhe_hip_sns_pks_params_preset(int preset, tfhe_sns_pks_params* out);
size_t tfhe_hip_sns_pksk_len(const tfhe_sns_pks_params* pp); /* 0 for a null pp */
int tfhe_hip_sns_pks_keygen(const tfhe_sns_pks_params* pp, uint64_t seed, const uint64_t* in_key, uint64_t* out_key,
                            uint64_t* pksk /* nullable */);
/* the same from a 192-bit rng key (OS entropy for production keys) */
int tfhe_hip_sns_pks_keygen_k(const tfhe_sns_pks_params* pp, const tfhe_rng_key* rk, const uint64_t* in_key,
                              uint64_t* out_key, uint64_t* pksk /* nullable */);
typedef struct tfhe_sns_pks_ctx tfhe_sns_pks_ctx;
/* The T workspace of a pack holds whole groups up to 512 MB; TFHE_HIP_SNS_PKS_CHUNK (read here, at create) sets
 * the groups per chunk instead. */
int tfhe_hip_sns_pks_create(const tfhe_sns_pks_params* pp, int device, tfhe_sns_pks_ctx** out);
void tfhe_hip_sns_pks_destroy(tfhe_sns_pks_ctx* ctx);
/* Waits for every call still in flight on the ctx before it rewrites the resident key. */
int tfhe_hip_sns_pks_load_key(tfhe_sns_pks_ctx* ctx, const uint64_t* pksk, size_t len);
/* count LWEs (count x (in_dim+1) x (lo, hi)) -> ceil(count / lwe_per_glwe) GLWEs ((out_k+1) x [lo][N], [hi][N]).
 * ENOKEYS without a key; count == 0 returns OK; EINVAL for a null buffer or count > 0x7FFFFFFF; every check runs
 * before any device work.  Host buffers, synchronous. */
int tfhe_hip_sns_pks_pack(tfhe_sns_pks_ctx* ctx, const uint64_t* lwes, size_t count, uint64_t* glwes);
/* Device buffers, enqueued on `stream` (NULL = the ctx stream, TFHE_HIP_NULL_STREAM = the null stream), as
 * tfhe_hip_pks_pack_async.  The digit and T workspaces are shared by every call on the ctx: calls on different
 * streams are ordered on them by an event, as tfhe_hip_sns_squash_async orders its own. */
int tfhe_hip_sns_pks_pack_async(tfhe_sns_pks_ctx* ctx, const uint64_t* d_lwes, size_t count, uint64_t* d_glwes,
                                void* stream);
/* The same rule on the CPU (no device, no ctx): the reference of the device path. */
int tfhe_hip_sns_pks_pack_host(const tfhe_sns_pks_params* pp, const uint64_t* pksk, const uint64_t* lwes, size_t count,
                               uint64_t* glwes);
size_t tfhe_hip_sns_pks_packed_words(const tfhe_sns_pks_params* pp, uint32_t bodies);
int tfhe_hip_sns_pks_compress(const tfhe_sns_pks_params* pp, const uint64_t* glwe, uint32_t bodies, uint64_t* packed);
int tfhe_hip_sns_pks_extract(const tfhe_sns_pks_params* pp, const uint64_t* packed, uint32_t bodies, uint64_t* glwe);
/* client-side decryption of a 128-bit GLWE: body - sum_c mask_c * S_c -> [lo][N], [hi][N] */
int tfhe_hip_glwe_phase128(uint32_t k, uint32_t N, const uint64_t* key, const uint64_t* glwe, uint64_t* out);
/* The seeded (compressed) ct128 packing key (tfhe-rs CompressedNoiseSquashingCompressionKey: a seeded packing
 * keyswitch key over u128), DESIGN §7h''; PARITY UNPINNED at the byte level.  One seeded 128-bit GLWE per (input
 * element j, storage row s), stream row rho = j level + s of the 128-bit mask stream above: out_k out_N u128 mask
 * words, then a body of [out_N] (lo, hi) pairs; bodies [in_dim][level][out_N][2], in_dim level 2 out_N words
 * (tfhe_hip_sns_pks_seeded_bodies_len, 0 for invalid parameters).  Storage row s holds decomposition level
 * `level - s` (least significant first, the keyswitching-key rule of the seeded section above) and lands in this
 * engine's row l = level - 1 - s, with in_key[j] 2^(128 - base_log (l + 1)) on body coefficient 0.  Noise of input
 * element j from ChaCha stream 0x900000 + j; the output key is that of tfhe_hip_sns_pks_keygen (stream 6).
 * tfhe_hip_sns_pks_decompress_key writes the loader's [j][l][c][lo, hi][N] layout on the host (the host route and the
 * CPU reference of the device expansion, word for word). */
size_t tfhe_hip_sns_pks_seeded_bodies_len(const tfhe_sns_pks_params* pp);
int tfhe_hip_sns_pks_seeded_keygen(const tfhe_sns_pks_params* pp, uint64_t rng_seed, const uint64_t seed[2],
                                   const uint64_t* in_key, uint64_t* out_key, uint64_t* bodies /* nullable */);
int tfhe_hip_sns_pks_seeded_keygen_k(const tfhe_sns_pks_params* pp, const tfhe_rng_key* rk, const uint64_t seed[2],
                                     const uint64_t* in_key, uint64_t* out_key, uint64_t* bodies /* nullable */);
int tfhe_hip_sns_pks_decompress_key(const tfhe_sns_pks_params* pp, const uint64_t seed[2], const uint64_t* bodies,
                                    uint64_t* pksk);
/* tfhe_hip_sns_pks_load_key from the seeded form: the bodies go up into a buffer of this call, the expansion kernel
 * writes the rows straight into the resident key and the correction kernel of tfhe_hip_sns_pks_load_key follows.  The
 * resident key equals that of the host route bit for bit.  EINVAL for a null argument or a wrong length, before any
 * change to the ctx; a refused load, or one that cannot allocate, leaves the resident key usable.  Waits for calls in
 * flight.  _load_stats: device ms of the last seeded load (upload, expansion, correction). */
int tfhe_hip_sns_pks_load_key_seeded(tfhe_sns_pks_ctx* ctx, const uint64_t seed[2], const uint64_t* bodies, size_t len);
int tfhe_hip_sns_pks_seeded_load_stats(const tfhe_sns_pks_ctx* ctx, double* upload_ms, double* expand_ms,
                                       double* corr_ms);
/* Test-facing: the loader's launcher into a fresh device buffer; out_host receives tfhe_hip_sns_pksk_len words
 * followed by TFHE_HIP_SEEDED_GUARD_WORDS pre-filled (0xA5) guard words. */
int tfhe_hip_sns_pks_seeded_expand_key(tfhe_sns_pks_ctx* ctx, const uint64_t seed[2], const uint64_t* bodies,
                                       uint64_t* out_host);

/* ---- encrypted matrix x clear matrix (the front half of the compression path) ------------------
 * Replaces the reference's GLWE x clear-matrix product (ml/extensions/rust/src: driver lib_python.rs:243-337
 * cuda_matrix_multiplication, CPU twin :340-401; ml.rs:66-90 cuda_glwe_dot_product_with_clear_one_to_many and the
 * LWE accumulate; rule computations.rs:80-132, encryption.rs:5-174, ml.rs:95-121).  All arithmetic is mod 2^64,
 * GLWE dimension 1.  Kernels tfhe_amd/csrc/matmul.hip, host client code tfhe_amd/csrc/seeded.cpp.
 *   encode   (encryption.rs:5-40)  plaintext = v * 2^(64 - bits_reserved), v a signed integer mod 2^64
 *   encrypt  (ml.rs:131-189, encryption.rs:88-133, compression.rs:59-105)  a row of the matrix is cut into chunks of
 *            N (the caller zero-pads the last); chunk g is one seeded GLWE: mask = words 0 .. N-1 of the AES-CTR
 *            stream of seed g (tfhe_hip_csprng_words(seed, 0, N)), body = A*S + e + plaintext, then the body alone
 *            is switched to in_storage_log bits, (((x >> (64-w-1)) + 1) >> 1) & (2^w - 1) (w = 64: unchanged), and
 *            bit-packed LSB first; every GLWE's body starts on a word boundary and takes
 *            tfhe_hip_matmul_body_words() words
 *   expand   (compression.rs:110-128, ml.rs:191-205)  body value << (64 - in_storage_log), mask from the seed
 *   dot      for row r, column c and K-blocks kb < Kb = ceil(K / N), w_kb[t] = W[kb N + t][c] (zero past K): the
 *            reference accumulates glwe_{r,kb} * reverse(w_kb) (negacyclic) and sample-extracts coefficient N-1;
 *            in closed form the output LWE (dimension N, under the GLWE key read as an LWE key) is
 *              mask[i] = sum_kb sum_t w_kb[t] * a'_{r,kb}[t - i],  a'[d] = a[d] (d >= 0), -a[N + d] (d < 0)
 *              body    = sum_kb sum_t w_kb[t] * b_{r,kb}[t]
 *   decode   (encryption.rs:135-174)  closest representable of the phase at bits_reserved bits, / delta, mod 2^b;
 *            values >= 2^(b-1) are negative
 * The C LWEs of one encrypted row then go through tfhe_hip_pks_pack_async (pks in_dim = N) in groups of
 * lwe_per_glwe that never straddle two rows, and tfhe_hip_pks_compress with `bodies` = the group's real count
 * (compression.rs:263-289).  PARITY UNPINNED at the byte level, as every seeded path here (the reference mount
 * holds no tfhe-rs). */
typedef struct tfhe_matmul_params {
  uint32_t N, bits_reserved, in_storage_log;
  int32_t noise_log2;
} tfhe_matmul_params;
/* N 2048, 27 bits reserved, bodies stored on 39 bits, noise 2^-48 (fhext_classes.rs:99-112, the rounding of the
 * reference's standard deviation that TFHE_HIP_PKS_PRESET_ML2048 uses) */
#define TFHE_HIP_MATMUL_PRESET_ML2048 0
int tfhe_hip_matmul_params_preset(int preset, tfhe_matmul_params* out);
/* Valid: N a power of two in 64 .. 4096, 1 <= bits_reserved <= 63, 1 <= in_storage_log <= 64, -64 < noise_log2 < 0;
 * every call below returns EINVAL otherwise, before any device work. */
size_t tfhe_hip_matmul_body_words(const tfhe_matmul_params* mp); /* ceil(N * in_storage_log / 64); 0 if invalid */
/* Host, no GPU.  keygen: N key bits from ChaCha stream 7 of the rng key.  encrypt: G GLWEs, values G x N (signed,
 * padded by the caller), seeds G x 2, packed_out G x body_words; the noise of GLWE g comes from ChaCha stream
 * stream0 + g.  expand_host: glwes_out G x 2 x N.  dot_host: the closed form above on the CPU, the layouts of
 * tfhe_hip_matmul_dot.  decode: count phases -> signed values. */
int tfhe_hip_matmul_keygen_k(const tfhe_matmul_params* mp, const tfhe_rng_key* rk, uint64_t* glwe_key);
int tfhe_hip_matmul_encrypt_k(const tfhe_matmul_params* mp, const uint64_t* glwe_key, const tfhe_rng_key* rk,
                              uint64_t stream0, const uint64_t* seeds, const int64_t* values, size_t G,
                              uint64_t* packed_out);
int tfhe_hip_matmul_expand_host(const tfhe_matmul_params* mp, const uint64_t* seeds, const uint64_t* packed, size_t G,
                                uint64_t* glwes_out);
int tfhe_hip_matmul_dot_host(const tfhe_matmul_params* mp, const int32_t* w, size_t K, size_t C, const uint64_t* glwes,
                             size_t R, size_t col_stride, uint64_t* lwes_out);
int tfhe_hip_matmul_decode(const tfhe_matmul_params* mp, const uint64_t* phases, size_t count, int64_t* out);
typedef struct tfhe_matmul_ctx tfhe_matmul_ctx;
typedef struct tfhe_matmul_matrix tfhe_matmul_matrix;
int tfhe_hip_matmul_create(const tfhe_matmul_params* mp, int device, tfhe_matmul_ctx** out);
/* Waits for every call still in flight on the ctx, on a caller's stream too.  Destroy the ctx's matrices first. */
void tfhe_hip_matmul_destroy(tfhe_matmul_ctx* ctx);
/* A clear matrix w (K x C, row-major, K >= 1, C >= 1) uploaded once and kept resident; a ctx may hold many.  destroy
 * waits for the calls in flight on the ctx before it frees the matrix. */
int tfhe_hip_matmul_matrix_create(tfhe_matmul_ctx* ctx, const int32_t* w, size_t K, size_t C, tfhe_matmul_matrix** out);
void tfhe_hip_matmul_matrix_destroy(tfhe_matmul_matrix* m);
/* Device buffers, enqueued on `stream` (NULL = the ctx stream, TFHE_HIP_NULL_STREAM = the null stream); calls on
 * different streams are ordered by an event as tfhe_hip_pks_pack_async orders its own, so a call may follow another
 * at once on any stream.  expand: d_seeds G x 2, d_packed G x body_words -> d_glwes G x 2 x N.  dot: d_glwes
 * R x Kb x 2 x N (Kb = ceil(K / N) of the matrix) -> LWE c of row r at d_lwes_out + (r * col_stride + c) * (N + 1),
 * col_stride >= C; the LWEs C .. col_stride - 1 of a row are not written (a caller that zero-fills them once can pack
 * all R rows in one tfhe_hip_pks_pack_async with col_stride a multiple of lwe_per_glwe: a zero LWE adds nothing to
 * its GLWE).  G == 0 / R == 0 return OK.  The forms without _async take host buffers and are synchronous; the host
 * dot reads lwes_out first, so the unwritten LWEs keep the caller's words. */
int tfhe_hip_matmul_expand_async(tfhe_matmul_ctx* ctx, const uint64_t* d_seeds, const uint64_t* d_packed, size_t G,
                                 uint64_t* d_glwes, void* stream);
int tfhe_hip_matmul_expand(tfhe_matmul_ctx* ctx, const uint64_t* seeds, const uint64_t* packed, size_t G,
                           uint64_t* glwes_out);
int tfhe_hip_matmul_dot_async(tfhe_matmul_ctx* ctx, const tfhe_matmul_matrix* m, const uint64_t* d_glwes, size_t R,
                              size_t col_stride, uint64_t* d_lwes_out, void* stream);
int tfhe_hip_matmul_dot(tfhe_matmul_ctx* ctx, const tfhe_matmul_matrix* m, const uint64_t* glwes, size_t R,
                        size_t col_stride, uint64_t* lwes_out);

#ifdef __cplusplus
}
#endif
#endif
