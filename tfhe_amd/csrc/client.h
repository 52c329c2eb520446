// client.h — host-side key material (see client.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/tfhe_hip.h"

namespace tfhe {
namespace client {
tfhe_rng_key rng_key_from_seed(uint64_t seed);
bool rng_key_entropy(tfhe_rng_key* k);  // getrandom(2), 192 bits
size_t bsk_len(const tfhe_params& p);
size_t ksk_len(const tfhe_params& p);
size_t bsk_bodies_len(const tfhe_params& p, uint32_t g);  // body words of a seeded BSK; g == 1: classic
size_t ksk_bodies_len(const tfhe_params& p);
void keygen(const tfhe_params& p, const tfhe_rng_key& rk, uint64_t* lwe_key, uint64_t* glwe_key, uint64_t* bsk, uint64_t* ksk);
// BSK / KSK for given binary secret keys (e.g. an ingested tfhe-rs ClientKey); same streams as keygen
void server_keygen(const tfhe_params& p, const tfhe_rng_key& rk, const uint64_t* lwe_key, const uint64_t* glwe_key,
                   uint64_t* bsk, uint64_t* ksk);
// multi-bit keys (include/tfhe_hip.h): g in {2, 3, 4}, n % g == 0 and a native-torus p are the caller's checks;
// bsk_mb [q][sigma - 1][level][row c][col j][N], the KSK that of server_keygen
size_t mb_bsk_len(const tfhe_params& p, uint32_t g);
void mb_server_keygen(const tfhe_params& p, uint32_t g, const tfhe_rng_key& rk, const uint64_t* lwe_key,
                      const uint64_t* glwe_key, uint64_t* bsk_mb, uint64_t* ksk);
// P-FHEVM modulus-switch zeros: count LWE encryptions of 0 under the small key, count x (n+1)
void ms_zeros_keygen(const tfhe_params& p, const tfhe_rng_key& rk, const uint64_t* lwe_key, uint32_t count, uint64_t* zeros);
void lwe_encrypt(uint32_t dim, const uint64_t* key, int32_t noise_log2, const tfhe_rng_key& rk, uint64_t stream0,
                 const uint64_t* msgs, size_t count, uint64_t* out);
void lwe_phase(uint32_t dim, const uint64_t* key, const uint64_t* ct, size_t count, uint64_t* out);
void noise_words(const tfhe_rng_key& rk, uint64_t stream, int32_t log2_sigma, size_t count, int64_t* out);
void lut_constant(uint32_t N, uint64_t torus_value, uint64_t* lut);
void lut_from_table(uint32_t N, uint32_t msg_modulus, const uint64_t* table, uint64_t delta, uint64_t* lut);
// packing keyswitch (LWE list -> GLWE) key and ciphertext compression
size_t pksk_len(const tfhe_pks_params& pp);
void pks_keygen(const tfhe_pks_params& pp, const tfhe_rng_key& rk, const uint64_t* in_key, uint64_t* out_key, uint64_t* pksk);
void glwe_phase_native(uint32_t k, uint32_t N, const uint64_t* key, const uint64_t* glwe, uint64_t* out);
size_t pks_packed_words(const tfhe_pks_params& pp, uint32_t bodies);
void pks_compress(const tfhe_pks_params& pp, const uint64_t* glwe, uint32_t bodies, uint64_t* packed);
void pks_extract(const tfhe_pks_params& pp, const uint64_t* packed, uint32_t bodies, uint64_t* glwe);
// noise squashing (128-bit GLWE over the native 2^128 torus, words as (lo, hi) planes)
size_t sns_bsk_len(const tfhe_sns_params& sp);
void sns_keygen(const tfhe_sns_params& sp, const tfhe_rng_key& rk, const uint64_t* lwe_key, uint64_t* glwe_key, uint64_t* bsk);
void sns_lut_identity(const tfhe_sns_params& sp, uint32_t msg_modulus, uint64_t* lut);
void sns_phase(const tfhe_sns_params& sp, const uint64_t* glwe_key, const uint64_t* cts, size_t count, uint64_t* out);
// compression of squashed ciphertexts: the packing keyswitch over Z_2^128 (include/tfhe_hip.h tfhe_hip_sns_pks_*)
size_t sns_pksk_len(const tfhe_sns_pks_params& pp);
void sns_pks_keygen(const tfhe_sns_pks_params& pp, const tfhe_rng_key& rk, const uint64_t* in_key, uint64_t* out_key,
                    uint64_t* pksk);
void sns_pks_pack_host(const tfhe_sns_pks_params& pp, const uint64_t* pksk, const uint64_t* lwes, size_t count,
                       uint64_t* glwes);
size_t sns_pks_packed_words(const tfhe_sns_pks_params& pp, uint32_t bodies);
void sns_pks_compress(const tfhe_sns_pks_params& pp, const uint64_t* glwe, uint32_t bodies, uint64_t* packed);
void sns_pks_extract(const tfhe_sns_pks_params& pp, const uint64_t* packed, uint32_t bodies, uint64_t* glwe);
void glwe_phase128(uint32_t k, uint32_t N, const uint64_t* key, const uint64_t* glwe, uint64_t* out);
void binary_key(const tfhe_rng_key& rk, uint64_t stream, size_t count, uint64_t* out);  // count bits of one ChaCha stream
}  // namespace client

// compressed (seeded) server keys (seeded.cpp)
namespace seeded {
void aes128_block(const uint8_t key[16], const uint8_t in[16], uint8_t out[16]);
void csprng_words(const uint64_t seed[2], uint64_t first, size_t count, uint64_t* out);
void seeded_server_keygen(const tfhe_params& p, const tfhe_rng_key& rk, const uint64_t bsk_seed[2],
                          const uint64_t ksk_seed[2], const uint64_t* lwe_key, const uint64_t* glwe_key,
                          uint64_t* bsk_bodies, uint64_t* ksk_bodies);
// multi-bit: bodies [n/g][2^g][L][k+1][N] (seeded.cpp); g in {2, 3, 4}, n % g == 0 and the shape are the caller's checks
void seeded_mb_server_keygen(const tfhe_params& p, uint32_t g, const tfhe_rng_key& rk, const uint64_t bsk_seed[2],
                             const uint64_t* lwe_key, const uint64_t* glwe_key, uint64_t* bsk_bodies);
void decompress_bsk_mb(const tfhe_params& p, uint32_t g, const uint64_t seed[2], const uint64_t* bodies,
                       uint64_t* bsk_mb);
// the 44 little-endian round-key words of a seed (the argument of the device kernels in seeded_keys.hip)
void aes_round_keys(const uint64_t seed[2], uint32_t out[44]);
void seeded_lwe_list(uint32_t dim, uint32_t count, const uint64_t* key, int32_t noise_log2, const tfhe_rng_key& rk,
                     uint64_t stream0, const uint64_t seed[2], const uint64_t* msgs, uint64_t* bodies);
void decompress_bsk(const tfhe_params& p, const uint64_t seed[2], const uint64_t* bodies, uint64_t* bsk);
void decompress_ksk(const tfhe_params& p, const uint64_t seed[2], const uint64_t* bodies, uint64_t* ksk);
void decompress_lwe_list(uint32_t dim, uint32_t count, const uint64_t seed[2], const uint64_t* bodies, uint64_t* out);
// seeded 128-bit keys (seeded.cpp; include/tfhe_hip.h tfhe_hip_sns_seeded_*, tfhe_hip_sns_pks_seeded_*): u128 words
// as (lo, hi) u64 pairs in the stream and in the bodies
void csprng_words128(const uint64_t seed[2], uint64_t first, size_t count, uint64_t* out_pairs);
size_t sns_bodies_len(const tfhe_sns_params& sp);          // n L (k+1) 2 N
size_t sns_pks_bodies_len(const tfhe_sns_pks_params& pp);  // in_dim level 2 out_N
void sns_seeded_keygen(const tfhe_sns_params& sp, const tfhe_rng_key& rk, const uint64_t seed[2],
                       const uint64_t* lwe_key, uint64_t* glwe_key, uint64_t* bodies /* nullable */);
void sns_decompress_bsk(const tfhe_sns_params& sp, const uint64_t seed[2], const uint64_t* bodies, uint64_t* bsk);
void sns_pks_seeded_keygen(const tfhe_sns_pks_params& pp, const tfhe_rng_key& rk, const uint64_t seed[2],
                           const uint64_t* in_key, uint64_t* out_key, uint64_t* bodies /* nullable */);
void sns_pks_decompress_key(const tfhe_sns_pks_params& pp, const uint64_t seed[2], const uint64_t* bodies,
                            uint64_t* pksk);
// encrypted matrix x clear matrix, client and CPU side (include/tfhe_hip.h tfhe_hip_matmul_*)
size_t matmul_body_words(const tfhe_matmul_params& mp);
void matmul_encrypt(const tfhe_matmul_params& mp, const uint64_t* glwe_key, const tfhe_rng_key& rk, uint64_t stream0,
                    const uint64_t* seeds, const int64_t* values, size_t G, uint64_t* packed);
void matmul_expand(const tfhe_matmul_params& mp, const uint64_t* seeds, const uint64_t* packed, size_t G, uint64_t* glwes);
void matmul_dot(const tfhe_matmul_params& mp, const int32_t* w, size_t K, size_t C, const uint64_t* glwes, size_t R,
                size_t col_stride, uint64_t* lwes);
void matmul_decode(const tfhe_matmul_params& mp, const uint64_t* phases, size_t count, int64_t* out);
}  // namespace seeded
}  // namespace tfhe
