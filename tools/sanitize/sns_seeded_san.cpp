// AddressSanitizer + UndefinedBehaviorSanitizer run of the host code of the seeded 128-bit keys
// (tfhe_amd/csrc/seeded.cpp: csprng_words128, sns_seeded_keygen, sns_decompress_bsk, sns_pks_seeded_keygen,
// sns_pks_decompress_key) as a stand-alone program, in the manner of sns_pks_san.cpp:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/sanitize/sns_seeded_san.cpp tfhe_amd/csrc/seeded.cpp tfhe_amd/csrc/client.cpp -o sns_seeded_san -pthread \
//       && ./sns_seeded_san
// Run by tests/test_sns_seeded.py.  Every buffer has its exact size, so an overrun is reported.  No GPU code.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/tfhe_hip.h"
#include "../../tfhe_amd/csrc/client.h"

using namespace tfhe;
typedef unsigned __int128 u128;

static int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      fails++;                                                     \
    }                                                              \
  } while (0)

static const uint64_t SEED[2] = {0xFEDCBA9876543210ull, 0x0123456789ABCDEFull};

static u128 absdiff(u128 a, u128 b) {
  const u128 d = a - b;
  return (d >> 127) ? (u128)0 - d : d;
}

// the stream: u128 word w = 64-bit words (2 w, 2 w + 1)
static void stream() {
  std::vector<uint64_t> p(2 * 33), w(2 * 33);
  seeded::csprng_words128(SEED, 7, 33, p.data());
  seeded::csprng_words(SEED, 14, 66, w.data());
  CHECK(!memcmp(p.data(), w.data(), p.size() * 8));
}

// squashing key at n: every decompressed row decrypts to the GGSW plaintext within 8 sigma
static void squashing(uint32_t n) {
  const tfhe_sns_params sp{n, 2, 2048, 24, 3, -34};
  const size_t k = sp.k, N = sp.N, L = sp.level, row = (k + 1) * 2 * N;
  std::vector<uint64_t> lwe(n), glwe(k * N), bodies(seeded::sns_bodies_len(sp)), bsk(client::sns_bsk_len(sp)), ph(2 * N);
  for (uint32_t i = 0; i < n; i++) lwe[i] = (i + 1) & 1;
  seeded::sns_seeded_keygen(sp, client::rng_key_from_seed(0x5EED128), SEED, lwe.data(), glwe.data(), bodies.data());
  seeded::sns_decompress_bsk(sp, SEED, bodies.data(), bsk.data());
  const u128 bound = (u128)1 << (67 + sp.noise_log2);
  for (size_t i = 0; i < n; i++)
    for (size_t c = 0; c <= k; c++)
      for (size_t l = 0; l < L; l++) {
        const uint64_t* r = bsk.data() + (i * (k + 1) * L + c * L + l) * row;
        client::glwe_phase128((uint32_t)k, (uint32_t)N, glwe.data(), r, ph.data());
        const u128 g = (u128)1 << (128 - sp.base_log * (l + 1));
        u128 worst = 0;
        for (size_t t = 0; t < N; t++) {
          u128 want = 0;
          if (lwe[i]) want = c < k ? (glwe[c * N + t] ? (u128)0 - g : 0) : (t == 0 ? g : 0);
          const u128 d = absdiff(((u128)ph[N + t] << 64) | ph[t], want);
          if (d > worst) worst = d;
        }
        CHECK(worst < bound);
      }
  printf("squashing key n %u: %zu rows decrypt\n", n, (size_t)n * (k + 1) * L);
}

// packing key: every decompressed row (engine row l = storage row level - 1 - l) decrypts to in_key[j] g_l
static void packing(const tfhe_sns_pks_params& pp) {
  const size_t k = pp.out_k, N = pp.out_N, L = pp.level, row = (k + 1) * 2 * N;
  std::vector<uint64_t> in_key(pp.in_dim), out_key(k * N), bodies(seeded::sns_pks_bodies_len(pp)),
      pksk(client::sns_pksk_len(pp)), ph(2 * N);
  for (uint32_t j = 0; j < pp.in_dim; j++) in_key[j] = (j * 7 + 1) % 3 == 0;
  seeded::sns_pks_seeded_keygen(pp, client::rng_key_from_seed(0x5EED128), SEED, in_key.data(), out_key.data(),
                                bodies.data());
  seeded::sns_pks_decompress_key(pp, SEED, bodies.data(), pksk.data());
  const u128 bound = (u128)1 << (67 + pp.noise_log2);
  for (size_t j = 0; j < pp.in_dim; j++)
    for (size_t l = 0; l < L; l++) {
      const uint64_t* r = pksk.data() + (j * L + l) * row;
      client::glwe_phase128((uint32_t)k, (uint32_t)N, out_key.data(), r, ph.data());
      const u128 g = (u128)1 << (128 - pp.base_log * (l + 1));
      for (size_t t = 0; t < N; t++) {
        const u128 want = (t == 0 && in_key[j]) ? g : 0;
        CHECK(absdiff(((u128)ph[N + t] << 64) | ph[t], want) < bound);
      }
      // the body pairs of storage row L - 1 - l, de-interleaved
      const uint64_t* b = bodies.data() + (j * L + (L - 1 - l)) * 2 * N;
      for (size_t t = 0; t < N; t++) CHECK(r[k * 2 * N + t] == b[2 * t] && r[k * 2 * N + N + t] == b[2 * t + 1]);
    }
  printf("packing key in_dim %u k %u N %u 2^%u x %u: %zu rows decrypt\n", pp.in_dim, pp.out_k, pp.out_N, pp.base_log,
         pp.level, (size_t)pp.in_dim * L);
}

int main() {
  stream();
  squashing(1);
  squashing(2);
  packing(tfhe_sns_pks_params{16, 1, 32, 61, 1, 32, 128, -62});  // the smallest ring, one level
  packing(tfhe_sns_pks_params{16, 1, 64, 40, 3, 32, 128, -62});  // three levels: the reversal
  printf(fails ? "SNS SEEDED SANITIZE FAIL %d\n" : "SNS SEEDED SANITIZE OK\n", fails);
  return fails ? 1 : 0;
}
