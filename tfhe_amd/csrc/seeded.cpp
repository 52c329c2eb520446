// seeded.cpp — compressed (seeded) server keys: the CompressedServerKey half of SURVEY §8f f3 (host C++).
//
// tfhe-rs ships evaluation keys compressed: every GLWE / LWE ciphertext of the bootstrapping key, the keyswitching
// key and the modulus-switch zeros keeps only its body, and the masks are regenerated from a 128-bit seed
// (tfhe-rs core_crypto decompress_seeded_lwe_bootstrap_key, decompress_seeded_lwe_keyswitch_key,
// decompress_seeded_lwe_ciphertext_list; the fhEVM coprocessor keeps its tenants' keys this way,
// tests/fhevm-suite/fhevm/docker-compose/coprocessor-docker-compose.yml:96).  tfhe-rs is absent from the reference
// mount, and the mount holds no server-key file, so this restates the published algorithm and is PARITY UNPINNED
// at the byte level; AES-128 itself is pinned by the FIPS-197 known answer (tests/test_seeded.py).
//
// Mask stream (tfhe-csprng AesCtrGenerator, software backend, as restated here):
//   AES-128 key = the seed's 16 bytes, little endian; block b of the stream = AES_key(b as a 128-bit little-endian
//   counter); the generator starts at table index SECOND (block 0, byte 1: the first byte is never output); a
//   native-modulus mask element is the next 8 bytes, little endian.  Forks hand out consecutive byte ranges, so
//   the masks of a whole key are one contiguous run of the stream in the order the encryption walks them:
//     bootstrapping key   GGSW i < n, level l < L (most significant first), row c <= k: k*N mask words
//     keyswitching key    input key element j < k*N, storage row s < ks_level: n mask words, where storage row s
//                         holds decomposition level ks_level - s (tfhe-rs generate_lwe_keyswitch_key walks the
//                         levels (1..=level_count).rev(), least significant first, so a block lines up with the
//                         SignedDecomposer's low-to-high digit iterator); this engine's KSK row l is level l + 1
//                         (most significant first), so storage row s <-> engine row ks_level - 1 - s
//     ciphertext list     ciphertext z: dim mask words
// A GGSW row c < k of tfhe-rs encrypts -m*g*S_c and row k encrypts m*g (g = 2^(64 - beta (l + 1))); this engine's
// keygen adds m*g to mask c of an encryption of zero instead.  Both have the same phase, which is all the external
// product uses, so an ingested row is stored as it is.
//
// Multi-bit bootstrapping key (tfhe-rs SeededLweMultiBitBootstrapKey, grouping factor g; PARITY UNPINNED at the byte
// level like the rest): group q < n/g holds 2^g GGSWs, sigma = 0 .. 2^g - 1, bit i of sigma belonging to key element
// g q + i; GGSW (q, sigma) encrypts the indicator [(s_{gq+i})_i = bits of sigma] in the row form above.  Bodies
// [n/g][2^g][L][k+1][N]; stream row rho = ((q 2^g + sigma) L + l)(k+1) + c owns mask words rho k N ... of the seed's
// stream.  This engine keeps sigma >= 1 only, in [q][sigma - 1][l][c][j][N] (level-major, unlike the classic
// [i][c L + l]): decompress_bsk_mb ignores the bodies of sigma = 0 and steps over its mask words.  That is valid
// because sum_sigma indicator_sigma = 1, so tfhe-rs's sum_sigma X^{t_sigma} GGSW_sigma [.] acc equals this engine's
// acc + sum_{sigma >= 1} (X^{t_sigma} - 1) GGSW_sigma [.] acc up to noise.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/tfhe_hip.h"
#include "client.h"

namespace tfhe {
namespace seeded {

// ------------------------------------------------------------------------------- AES-128 (FIPS-197)
namespace {
uint8_t SBOX[256];

inline uint8_t rotl8(uint8_t x, int s) { return (uint8_t)((x << s) | (x >> (8 - s))); }
inline uint8_t xt(uint8_t x) { return (uint8_t)((x << 1) ^ ((x >> 7) * 0x1b)); }

void init_sbox() {
  // walk the multiplicative group by p *= 3, q = p^-1 (q /= 3), S(p) = affine(q)
  uint8_t p = 1, q = 1;
  do {
    p = (uint8_t)(p ^ (p << 1) ^ (p & 0x80 ? 0x1b : 0));
    q ^= (uint8_t)(q << 1);
    q ^= (uint8_t)(q << 2);
    q ^= (uint8_t)(q << 4);
    if (q & 0x80) q ^= 0x09;
    SBOX[p] = (uint8_t)(q ^ rotl8(q, 1) ^ rotl8(q, 2) ^ rotl8(q, 3) ^ rotl8(q, 4) ^ 0x63);
  } while (p != 1);
  SBOX[0] = 0x63;
}

struct Aes128 {
  uint8_t rk[176];
  explicit Aes128(const uint8_t key[16]) {
    static const uint8_t RCON[10] = {0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1b, 0x36};
    memcpy(rk, key, 16);
    for (int i = 4; i < 44; i++) {
      uint8_t t[4] = {rk[4 * (i - 1)], rk[4 * (i - 1) + 1], rk[4 * (i - 1) + 2], rk[4 * (i - 1) + 3]};
      if (i % 4 == 0) {
        const uint8_t t0 = t[0];
        t[0] = (uint8_t)(SBOX[t[1]] ^ RCON[i / 4 - 1]);
        t[1] = SBOX[t[2]];
        t[2] = SBOX[t[3]];
        t[3] = SBOX[t0];
      }
      for (int b = 0; b < 4; b++) rk[4 * i + b] = (uint8_t)(rk[4 * (i - 4) + b] ^ t[b]);
    }
  }
  // state byte r + 4 c = row r, column c
  void encrypt(const uint8_t in[16], uint8_t out[16]) const {
    uint8_t s[16];
    for (int i = 0; i < 16; i++) s[i] = (uint8_t)(in[i] ^ rk[i]);
    for (int round = 1; round <= 10; round++) {
      uint8_t t[16];
      for (int c = 0; c < 4; c++)  // SubBytes + ShiftRows
        for (int r = 0; r < 4; r++) t[r + 4 * c] = SBOX[s[r + 4 * ((c + r) & 3)]];
      if (round < 10)
        for (int c = 0; c < 4; c++) {  // MixColumns
          const uint8_t a0 = t[4 * c], a1 = t[4 * c + 1], a2 = t[4 * c + 2], a3 = t[4 * c + 3];
          const uint8_t x = (uint8_t)(a0 ^ a1 ^ a2 ^ a3);
          t[4 * c] = (uint8_t)(a0 ^ x ^ xt((uint8_t)(a0 ^ a1)));
          t[4 * c + 1] = (uint8_t)(a1 ^ x ^ xt((uint8_t)(a1 ^ a2)));
          t[4 * c + 2] = (uint8_t)(a2 ^ x ^ xt((uint8_t)(a2 ^ a3)));
          t[4 * c + 3] = (uint8_t)(a3 ^ x ^ xt((uint8_t)(a3 ^ a0)));
        }
      for (int i = 0; i < 16; i++) s[i] = (uint8_t)(t[i] ^ rk[16 * round + i]);
    }
    memcpy(out, s, 16);
  }
};

struct SboxInit {
  SboxInit() { init_sbox(); }
};
const SboxInit sbox_init;

// stream bytes [byte0, byte0 + n) of the seed's AES-CTR stream (absolute byte index: block = index / 16)
void stream_bytes(const Aes128& aes, uint64_t byte0, size_t n, uint8_t* out) {
  uint64_t blk = byte0 / 16;
  size_t off = (size_t)(byte0 % 16), done = 0;
  while (done < n) {
    uint8_t ctr[16] = {0}, ks[16];
    for (int b = 0; b < 8; b++) ctr[b] = (uint8_t)(blk >> (8 * b));  // 128-bit little-endian counter (< 2^64 here)
    aes.encrypt(ctr, ks);
    const size_t take = std::min((size_t)16 - off, n - done);
    memcpy(out + done, ks + off, take);
    done += take;
    off = 0;
    blk++;
  }
}

template <class F>
void parallel_for(int64_t count, F&& f) {
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const int64_t nt = std::min<int64_t>(std::min<int64_t>(hw, 32), count);
  if (nt <= 1) {
    for (int64_t i = 0; i < count; i++) f(i);
    return;
  }
  std::vector<std::thread> th;
  for (int64_t t = 0; t < nt; t++)
    th.emplace_back([&, t] {
      for (int64_t i = t; i < count; i += nt) f(i);
    });
  for (auto& x : th) x.join();
}

void key_bytes(const uint64_t seed[2], uint8_t key[16]) {
  for (int b = 0; b < 8; b++) {
    key[b] = (uint8_t)(seed[0] >> (8 * b));
    key[8 + b] = (uint8_t)(seed[1] >> (8 * b));
  }
}

constexpr uint64_t STREAM_START = 1;  // TableIndex::SECOND

// mask words [w0, w0 + count) of the seed's stream
void mask_words(const Aes128& aes, uint64_t w0, size_t count, uint64_t* out) {
  std::vector<uint8_t> b(count * 8);
  stream_bytes(aes, STREAM_START + 8 * w0, b.size(), b.data());
  for (size_t i = 0; i < count; i++) {
    uint64_t v = 0;
    for (int k = 0; k < 8; k++) v |= (uint64_t)b[8 * i + k] << (8 * k);
    out[i] = v;
  }
}

// body += a (*) s (negacyclic, binary s)
void add_product(uint32_t N, const uint64_t* a, const uint64_t* s, uint64_t* body) {
  for (uint32_t j = 0; j < N; j++) {
    if (!s[j]) continue;
    for (uint32_t i = 0; i < N; i++) {
      const uint32_t d = i + j;
      if (d < N) body[d] += a[i];
      else body[d - N] -= a[i];
    }
  }
}
}  // namespace

void aes128_block(const uint8_t key[16], const uint8_t in[16], uint8_t out[16]) { Aes128(key).encrypt(in, out); }

// the 44 round-key words of a seed, little endian (word 4 i + c = column c of round key i): what the device kernels
// of seeded_keys.hip take, so the key schedule runs once per seed
void aes_round_keys(const uint64_t seed[2], uint32_t out[44]) {
  uint8_t key[16];
  key_bytes(seed, key);
  const Aes128 aes(key);
  for (int i = 0; i < 44; i++)
    out[i] = (uint32_t)aes.rk[4 * i] | ((uint32_t)aes.rk[4 * i + 1] << 8) | ((uint32_t)aes.rk[4 * i + 2] << 16) |
             ((uint32_t)aes.rk[4 * i + 3] << 24);
}

void csprng_words(const uint64_t seed[2], uint64_t first, size_t count, uint64_t* out) {
  uint8_t key[16];
  key_bytes(seed, key);
  const Aes128 aes(key);
  const size_t chunk = 1 << 14;
  const int64_t nch = (int64_t)((count + chunk - 1) / chunk);
  parallel_for(nch, [&](int64_t c) {
    const size_t o = (size_t)c * chunk;
    mask_words(aes, first + o, std::min(chunk, count - o), out + o);
  });
}

// seeded BSK / KSK bodies for given binary secret keys; noise from the ChaCha streams of server_keygen
void seeded_server_keygen(const tfhe_params& p, const tfhe_rng_key& rk, const uint64_t bsk_seed[2],
                          const uint64_t ksk_seed[2], const uint64_t* lwe_key, const uint64_t* glwe_key,
                          uint64_t* bsk_bodies, uint64_t* ksk_bodies) {
  const uint32_t k = p.k, N = p.N, L = p.pbs_level, n = p.n;
  uint8_t key[16];
  if (bsk_bodies) {
    key_bytes(bsk_seed, key);
    const Aes128 aes(key);
    parallel_for((int64_t)n, [&](int64_t i) {
      std::vector<uint64_t> mask((size_t)k * N);
      std::vector<int64_t> e((size_t)L * (k + 1) * N);
      client::noise_words(rk, 0x1000 + (uint64_t)i, p.glwe_noise_log2, e.size(), e.data());
      for (uint32_t l = 0; l < L; l++) {
        const uint64_t g = 1ull << (64 - p.pbs_base_log * (l + 1));
        for (uint32_t c = 0; c <= k; c++) {
          const size_t row = ((size_t)i * L + l) * (k + 1) + c;
          mask_words(aes, row * k * N, (size_t)k * N, mask.data());
          uint64_t* body = bsk_bodies + row * N;
          for (uint32_t t = 0; t < N; t++) body[t] = (uint64_t)e[((size_t)l * (k + 1) + c) * N + t];
          for (uint32_t cc = 0; cc < k; cc++) add_product(N, mask.data() + (size_t)cc * N, glwe_key + (size_t)cc * N, body);
          if (lwe_key[i]) {  // plaintext -m g S_c (row c < k) / m g (row k)
            if (c < k)
              for (uint32_t t = 0; t < N; t++) body[t] -= g * glwe_key[(size_t)c * N + t];
            else
              body[0] += g;
          }
        }
      }
    });
  }
  if (ksk_bodies) {
    key_bytes(ksk_seed, key);
    const Aes128 aes(key);
    parallel_for((int64_t)k * N, [&](int64_t j) {
      std::vector<uint64_t> mask(n);
      std::vector<int64_t> e(p.ks_level);
      client::noise_words(rk, 0x100000 + (uint64_t)j, p.lwe_noise_log2, e.size(), e.data());
      for (uint32_t s = 0; s < p.ks_level; s++) {  // storage row s = engine level ks_level - 1 - s
        const size_t row = (size_t)j * p.ks_level + s;
        mask_words(aes, row * n, n, mask.data());
        uint64_t acc = (uint64_t)e[s] + (glwe_key[j] << (64 - p.ks_base_log * (p.ks_level - s)));
        for (uint32_t t = 0; t < n; t++) acc += mask[t] * lwe_key[t];
        ksk_bodies[row] = acc;
      }
    });
  }
}

// seeded multi-bit BSK bodies [n/g][2^g][L][k+1][N] (the header of this file); noise of GGSW (q, sigma) from ChaCha
// stream 0x700000 + 16 q + sigma
void seeded_mb_server_keygen(const tfhe_params& p, uint32_t g, const tfhe_rng_key& rk, const uint64_t bsk_seed[2],
                             const uint64_t* lwe_key, const uint64_t* glwe_key, uint64_t* bsk_bodies) {
  const uint32_t k = p.k, N = p.N, L = p.pbs_level, per_q = 1u << g;
  uint8_t key[16];
  key_bytes(bsk_seed, key);
  const Aes128 aes(key);
  parallel_for((int64_t)(p.n / g) * per_q, [&](int64_t idx) {
    const uint32_t q = (uint32_t)(idx / per_q), sigma = (uint32_t)(idx % per_q);
    bool ind = true;
    for (uint32_t i = 0; i < g; i++) ind = ind && lwe_key[(size_t)g * q + i] == ((sigma >> i) & 1u);
    std::vector<uint64_t> mask((size_t)k * N);
    std::vector<int64_t> e((size_t)L * (k + 1) * N);
    client::noise_words(rk, 0x700000 + 16 * (uint64_t)q + sigma, p.glwe_noise_log2, e.size(), e.data());
    for (uint32_t l = 0; l < L; l++) {
      const uint64_t gl = 1ull << (64 - p.pbs_base_log * (l + 1));
      for (uint32_t c = 0; c <= k; c++) {
        const size_t row = ((size_t)idx * L + l) * (k + 1) + c;
        mask_words(aes, row * k * N, (size_t)k * N, mask.data());
        uint64_t* body = bsk_bodies + row * N;
        for (uint32_t t = 0; t < N; t++) body[t] = (uint64_t)e[((size_t)l * (k + 1) + c) * N + t];
        for (uint32_t cc = 0; cc < k; cc++) add_product(N, mask.data() + (size_t)cc * N, glwe_key + (size_t)cc * N, body);
        if (ind) {  // plaintext -m g S_c (row c < k) / m g (row k)
          if (c < k)
            for (uint32_t t = 0; t < N; t++) body[t] -= gl * glwe_key[(size_t)c * N + t];
          else
            body[0] += gl;
        }
      }
    }
  });
}

void seeded_lwe_list(uint32_t dim, uint32_t count, const uint64_t* key, int32_t noise_log2, const tfhe_rng_key& rk,
                     uint64_t stream0, const uint64_t seed[2], const uint64_t* msgs, uint64_t* bodies) {
  uint8_t kb[16];
  key_bytes(seed, kb);
  const Aes128 aes(kb);
  parallel_for((int64_t)count, [&](int64_t z) {
    std::vector<uint64_t> mask(dim);
    int64_t e;
    client::noise_words(rk, stream0 + (uint64_t)z, noise_log2, 1, &e);
    mask_words(aes, (uint64_t)z * dim, dim, mask.data());
    uint64_t acc = (uint64_t)e + (msgs ? msgs[z] : 0);
    for (uint32_t t = 0; t < dim; t++) acc += mask[t] * key[t];
    bodies[z] = acc;
  });
}

void decompress_bsk(const tfhe_params& p, const uint64_t seed[2], const uint64_t* bodies, uint64_t* bsk) {
  const uint32_t k = p.k, N = p.N, L = p.pbs_level;
  const size_t row_len = (size_t)(k + 1) * N, per_i = (size_t)(k + 1) * L * row_len;
  uint8_t key[16];
  key_bytes(seed, key);
  const Aes128 aes(key);
  parallel_for((int64_t)p.n, [&](int64_t i) {
    for (uint32_t l = 0; l < L; l++)
      for (uint32_t c = 0; c <= k; c++) {
        const size_t row = ((size_t)i * L + l) * (k + 1) + c;
        uint64_t* out = bsk + per_i * i + row_len * (c * L + l);  // this engine's [i][c * L + l][j]
        mask_words(aes, row * k * N, (size_t)k * N, out);
        memcpy(out + (size_t)k * N, bodies + row * N, (size_t)N * 8);
      }
  });
}

// the multi-bit key in this engine's layout [q][sigma - 1][l][c][j][N]: sigma = 0 is skipped (its bodies ignored,
// its mask words stepped over by the source row index)
void decompress_bsk_mb(const tfhe_params& p, uint32_t g, const uint64_t seed[2], const uint64_t* bodies,
                       uint64_t* bsk_mb) {
  const uint32_t k = p.k, N = p.N, L = p.pbs_level, per_q = (1u << g) - 1;
  const size_t row_len = (size_t)(k + 1) * N, rows_per_ggsw = (size_t)L * (k + 1);
  uint8_t key[16];
  key_bytes(seed, key);
  const Aes128 aes(key);
  parallel_for((int64_t)(p.n / g) * per_q, [&](int64_t idx) {
    const size_t q = (size_t)idx / per_q, sigma = (size_t)idx % per_q + 1;
    for (size_t t = 0; t < rows_per_ggsw; t++) {  // t = l (k + 1) + c in both layouts
      const size_t src = (q * (per_q + 1) + sigma) * rows_per_ggsw + t;
      uint64_t* out = bsk_mb + ((size_t)idx * rows_per_ggsw + t) * row_len;
      mask_words(aes, src * k * N, (size_t)k * N, out);
      memcpy(out + (size_t)k * N, bodies + src * N, (size_t)N * 8);
    }
  });
}

void decompress_ksk(const tfhe_params& p, const uint64_t seed[2], const uint64_t* bodies, uint64_t* ksk) {
  const uint32_t n = p.n;
  uint8_t key[16];
  key_bytes(seed, key);
  const Aes128 aes(key);
  parallel_for((int64_t)p.k * p.N, [&](int64_t j) {
    for (uint32_t s = 0; s < p.ks_level; s++) {  // storage row s (least significant first) -> engine row
      const size_t row = (size_t)j * p.ks_level + s;
      uint64_t* out = ksk + ((size_t)j * p.ks_level + (p.ks_level - 1 - s)) * (n + 1);
      mask_words(aes, row * n, n, out);
      out[n] = bodies[row];
    }
  });
}

void decompress_lwe_list(uint32_t dim, uint32_t count, const uint64_t seed[2], const uint64_t* bodies, uint64_t* out) {
  uint8_t key[16];
  key_bytes(seed, key);
  const Aes128 aes(key);
  parallel_for((int64_t)count, [&](int64_t z) {
    uint64_t* o = out + (size_t)z * (dim + 1);
    mask_words(aes, (uint64_t)z * dim, dim, o);
    o[dim] = bodies[z];
  });
}

// ------------------------------------------------- seeded 128-bit keys: noise squashing and ct128 packing (DESIGN §7h'')
// The 128-bit mask stream: u128 mask word w of a seed is stream bytes 16 w + 1 .. 16 w + 16, little endian (the start
// at byte 1 of the 64-bit stream above), i.e. lo = word 2 w and hi = word 2 w + 1 of csprng_words: block w less its
// byte 0, plus byte 0 of block w + 1.  PARITY UNPINNED at the byte level, as every seeded path here.
//   squashing key   bodies [n][L][k+1][N] u128 as (lo, hi) u64 pairs (the bytes of a Vec<u128>); stream row
//                   rho = (i L + l)(k + 1) + c, level l = 0 most significant, owns u128 mask words rho k N ..
//                   (polynomial j, then coefficient t); GGSW rows in tfhe-rs's form (row c < k: -s_i g_l S_c, row k:
//                   s_i g_l on coefficient 0, g_l = 2^(128 - base_log (l + 1))); noise of GGSW i from ChaCha stream
//                   0x800000 + i; engine layout [i][c L + l][j][lo, hi][N]
//   packing key     one seeded GLWE per (input element j, storage row s), rho = j level + s; storage row s holds
//                   decomposition level `level - s` (least significant first, as the keyswitching key above) and lands
//                   in engine row level - 1 - s; mask out_k out_N u128 words, body [out_N] pairs with
//                   in_key[j] 2^(128 - base_log (l + 1)) on coefficient 0 (l the engine row); noise of input element j
//                   from ChaCha stream 0x900000 + j; engine layout [j][l][c][lo, hi][N]
namespace {
typedef unsigned __int128 u128;

// u128 mask words [w0, w0 + count) of the seed's stream as planes lo[count], hi[count]
void mask_planes128(const Aes128& aes, uint64_t w0, size_t count, uint64_t* lo, uint64_t* hi) {
  std::vector<uint64_t> w(2 * count);
  mask_words(aes, 2 * w0, w.size(), w.data());
  for (size_t t = 0; t < count; t++) lo[t] = w[2 * t], hi[t] = w[2 * t + 1];
}

std::vector<std::vector<uint32_t>> set_bits(uint32_t k, uint32_t N, const uint64_t* key) {
  std::vector<std::vector<uint32_t>> bits(k);
  for (uint32_t c = 0; c < k; c++)
    for (uint32_t u = 0; u < N; u++)
      if (key[(size_t)c * N + u]) bits[c].push_back(u);
  return bits;
}

// body of one seeded 128-bit GLWE row: e + sum_c mask_c (*) S_c (negacyclic, mod 2^128) for the masks of stream row
// rho; planes is a k x 2 x N scratch
void zero_body128(const Aes128& aes, uint64_t rho, uint32_t k, uint32_t N,
                  const std::vector<std::vector<uint32_t>>& bits, const int64_t* e, uint64_t* planes, u128* body) {
  for (uint32_t t = 0; t < N; t++) body[t] = (u128)(__int128)e[t];
  for (uint32_t c = 0; c < k; c++) {
    uint64_t *lo = planes + (size_t)c * 2 * N, *hi = lo + N;
    mask_planes128(aes, (rho * k + c) * N, N, lo, hi);
    for (const uint32_t u : bits[c]) {
      for (uint32_t x = 0; x < u; x++) body[x] -= ((u128)hi[x + N - u] << 64) | lo[x + N - u];
      for (uint32_t x = u; x < N; x++) body[x] += ((u128)hi[x - u] << 64) | lo[x - u];
    }
  }
}

inline void store_pairs(const u128* body, uint32_t N, uint64_t* out) {
  for (uint32_t t = 0; t < N; t++) out[2 * t] = (uint64_t)body[t], out[2 * t + 1] = (uint64_t)(body[t] >> 64);
}

// one expanded row: k mask polynomials of stream row rho as planes, then the body pairs de-interleaved
void expand_row128(const Aes128& aes, uint64_t rho, uint32_t k, uint32_t N, const uint64_t* body_pairs, uint64_t* out) {
  for (uint32_t c = 0; c < k; c++) mask_planes128(aes, (rho * k + c) * N, N, out + (size_t)c * 2 * N, out + (size_t)c * 2 * N + N);
  uint64_t *lo = out + (size_t)k * 2 * N, *hi = lo + N;
  for (uint32_t t = 0; t < N; t++) lo[t] = body_pairs[2 * t], hi[t] = body_pairs[2 * t + 1];
}
}  // namespace

void csprng_words128(const uint64_t seed[2], uint64_t first, size_t count, uint64_t* out_pairs) {
  csprng_words(seed, 2 * first, 2 * count, out_pairs);
}

size_t sns_bodies_len(const tfhe_sns_params& sp) { return (size_t)sp.n * sp.level * (sp.k + 1) * 2 * sp.N; }
size_t sns_pks_bodies_len(const tfhe_sns_pks_params& pp) { return (size_t)pp.in_dim * pp.level * 2 * pp.out_N; }

void sns_seeded_keygen(const tfhe_sns_params& sp, const tfhe_rng_key& rk, const uint64_t seed[2],
                       const uint64_t* lwe_key, uint64_t* glwe_key, uint64_t* bodies) {
  const uint32_t k = sp.k, N = sp.N, L = sp.level;
  client::binary_key(rk, 5, (size_t)k * N, glwe_key);
  if (!bodies) return;
  const std::vector<std::vector<uint32_t>> bits = set_bits(k, N, glwe_key);
  uint8_t key[16];
  key_bytes(seed, key);
  const Aes128 aes(key);
  parallel_for((int64_t)sp.n, [&](int64_t i) {
    std::vector<int64_t> e((size_t)L * (k + 1) * N);
    std::vector<uint64_t> planes((size_t)k * 2 * N);
    std::vector<u128> body(N);
    client::noise_words(rk, 0x800000 + (uint64_t)i, sp.noise_log2, e.size(), e.data());
    for (uint32_t l = 0; l < L; l++) {
      const u128 g = (u128)1 << (128 - sp.base_log * (l + 1));
      for (uint32_t c = 0; c <= k; c++) {
        const uint64_t rho = ((uint64_t)i * L + l) * (k + 1) + c;
        zero_body128(aes, rho, k, N, bits, e.data() + ((size_t)l * (k + 1) + c) * N, planes.data(), body.data());
        if (lwe_key[i]) {  // plaintext -s_i g S_c (row c < k) / s_i g (row k)
          if (c < k) {
            for (const uint32_t u : bits[c]) body[u] -= g;
          } else {
            body[0] += g;
          }
        }
        store_pairs(body.data(), N, bodies + rho * 2 * N);
      }
    }
  });
}

void sns_decompress_bsk(const tfhe_sns_params& sp, const uint64_t seed[2], const uint64_t* bodies, uint64_t* bsk) {
  const uint32_t k = sp.k, N = sp.N, L = sp.level;
  const size_t row_len = (size_t)(k + 1) * 2 * N, per_i = (size_t)(k + 1) * L * row_len;
  uint8_t key[16];
  key_bytes(seed, key);
  const Aes128 aes(key);
  parallel_for((int64_t)sp.n, [&](int64_t i) {
    for (uint32_t l = 0; l < L; l++)
      for (uint32_t c = 0; c <= k; c++) {
        const uint64_t rho = ((uint64_t)i * L + l) * (k + 1) + c;
        expand_row128(aes, rho, k, N, bodies + rho * 2 * N, bsk + per_i * i + row_len * (c * L + l));
      }
  });
}

void sns_pks_seeded_keygen(const tfhe_sns_pks_params& pp, const tfhe_rng_key& rk, const uint64_t seed[2],
                           const uint64_t* in_key, uint64_t* out_key, uint64_t* bodies) {
  const uint32_t k = pp.out_k, N = pp.out_N, L = pp.level;
  client::binary_key(rk, 6, (size_t)k * N, out_key);
  if (!bodies) return;
  const std::vector<std::vector<uint32_t>> bits = set_bits(k, N, out_key);
  uint8_t key[16];
  key_bytes(seed, key);
  const Aes128 aes(key);
  parallel_for((int64_t)pp.in_dim, [&](int64_t j) {
    std::vector<int64_t> e((size_t)L * N);
    std::vector<uint64_t> planes((size_t)k * 2 * N);
    std::vector<u128> body(N);
    client::noise_words(rk, 0x900000 + (uint64_t)j, pp.noise_log2, e.size(), e.data());
    for (uint32_t s = 0; s < L; s++) {  // storage row s = engine row L - 1 - s
      const uint64_t rho = (uint64_t)j * L + s;
      zero_body128(aes, rho, k, N, bits, e.data() + (size_t)s * N, planes.data(), body.data());
      if (in_key[j]) body[0] += (u128)1 << (128 - pp.base_log * (L - s));
      store_pairs(body.data(), N, bodies + rho * 2 * N);
    }
  });
}

void sns_pks_decompress_key(const tfhe_sns_pks_params& pp, const uint64_t seed[2], const uint64_t* bodies,
                            uint64_t* pksk) {
  const uint32_t k = pp.out_k, N = pp.out_N, L = pp.level;
  const size_t row_len = (size_t)(k + 1) * 2 * N;
  uint8_t key[16];
  key_bytes(seed, key);
  const Aes128 aes(key);
  parallel_for((int64_t)pp.in_dim, [&](int64_t j) {
    for (uint32_t s = 0; s < L; s++) {
      const uint64_t rho = (uint64_t)j * L + s;
      expand_row128(aes, rho, k, N, bodies + rho * 2 * N, pksk + ((size_t)j * L + (L - 1 - s)) * row_len);
    }
  });
}

// ------------------------------------------------- encrypted matrix x clear matrix: client and CPU side
// The conventions of include/tfhe_hip.h (tfhe_hip_matmul_*), restated from the reference: encode encryption.rs:5-40,
// seeded encryption ml.rs:131-189 / encryption.rs:88-133, storage switch and packing compression.rs:59-105, expansion
// compression.rs:110-128, product and extraction computations.rs:80-132 / ml.rs:95-121, decode encryption.rs:135-174.
// PARITY UNPINNED at the byte level, as the seeded keys above.
size_t matmul_body_words(const tfhe_matmul_params& mp) { return ((size_t)mp.N * mp.in_storage_log + 63) / 64; }

void matmul_encrypt(const tfhe_matmul_params& mp, const uint64_t* glwe_key, const tfhe_rng_key& rk, uint64_t stream0,
                    const uint64_t* seeds, const int64_t* values, size_t G, uint64_t* packed) {
  const uint32_t N = mp.N, w = mp.in_storage_log;
  const size_t bw = matmul_body_words(mp);
  const uint64_t vmask = (w == 64) ? ~0ull : ((1ull << w) - 1);
  parallel_for((int64_t)G, [&](int64_t g) {
    uint8_t kb[16];
    key_bytes(seeds + 2 * g, kb);
    const Aes128 aes(kb);
    std::vector<uint64_t> mask(N), body(N);
    std::vector<int64_t> e(N);
    mask_words(aes, 0, N, mask.data());
    client::noise_words(rk, stream0 + (uint64_t)g, mp.noise_log2, N, e.data());
    for (uint32_t t = 0; t < N; t++)
      body[t] = (uint64_t)e[t] + ((uint64_t)values[(size_t)g * N + t] << (64 - mp.bits_reserved));
    add_product(N, mask.data(), glwe_key, body.data());
    uint64_t* out = packed + (size_t)g * bw;
    memset(out, 0, bw * 8);
    for (uint32_t t = 0; t < N; t++) {
      const uint64_t x = body[t];
      const uint64_t ms = (w == 64) ? x : ((((x >> (64 - w - 1)) + 1) >> 1) & vmask);
      const size_t bit = (size_t)t * w, word = bit >> 6, off = bit & 63;
      out[word] |= ms << off;
      if (off + w > 64) out[word + 1] |= ms >> (64 - off);
    }
  });
}

void matmul_expand(const tfhe_matmul_params& mp, const uint64_t* seeds, const uint64_t* packed, size_t G, uint64_t* glwes) {
  const uint32_t N = mp.N, w = mp.in_storage_log;
  const size_t bw = matmul_body_words(mp);
  parallel_for((int64_t)G, [&](int64_t g) {
    uint8_t kb[16];
    key_bytes(seeds + 2 * g, kb);
    const Aes128 aes(kb);
    uint64_t* o = glwes + (size_t)g * 2 * N;
    mask_words(aes, 0, N, o);
    const uint64_t* p = packed + (size_t)g * bw;
    for (uint32_t t = 0; t < N; t++) {
      const size_t bit = (size_t)t * w, word = bit >> 6, off = bit & 63;
      uint64_t v = p[word] >> off;
      if (off + w > 64) v |= p[word + 1] << (64 - off);
      o[N + t] = v << (64 - w);
    }
  });
}

// one (row, column) per task: mask[i] = sum_kb sum_t w[t] a'[t - i] as t loops over shifted copies of a
void matmul_dot(const tfhe_matmul_params& mp, const int32_t* w, size_t K, size_t C, const uint64_t* glwes, size_t R,
                size_t col_stride, uint64_t* lwes) {
  const size_t N = mp.N, Kb = (K + N - 1) / N;
  parallel_for((int64_t)(R * C), [&](int64_t rc) {
    const size_t r = (size_t)rc / C, c = (size_t)rc % C;
    uint64_t* o = lwes + (r * col_stride + c) * (N + 1);
    memset(o, 0, (N + 1) * 8);
    for (size_t kb = 0; kb < Kb; kb++) {
      const uint64_t* a = glwes + (r * Kb + kb) * 2 * N;
      const uint64_t* b = a + N;
      for (size_t t = 0; t < N && kb * N + t < K; t++) {
        const uint64_t wt = (uint64_t)(int64_t)w[(kb * N + t) * C + c];
        if (!wt) continue;
        for (size_t i = 0; i <= t; i++) o[i] += wt * a[t - i];
        for (size_t i = t + 1; i < N; i++) o[i] -= wt * a[N + t - i];
        o[N] += wt * b[t];
      }
    }
  });
}

void matmul_decode(const tfhe_matmul_params& mp, const uint64_t* phases, size_t count, int64_t* out) {
  const uint32_t b = mp.bits_reserved;
  const uint64_t mod_mask = (1ull << b) - 1, half = 1ull << (b - 1);
  for (size_t i = 0; i < count; i++) {
    const uint64_t v = (((phases[i] >> (64 - b - 1)) + 1) >> 1) & mod_mask;
    out[i] = (int64_t)(v >= half ? v - (1ull << b) : v);
  }
}

}  // namespace seeded
}  // namespace tfhe
