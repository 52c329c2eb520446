// AddressSanitizer + UndefinedBehaviorSanitizer run of the host code of the squashed-ciphertext compression
// (tfhe_amd/csrc/client.cpp: sns_pks_keygen, sns_pks_pack_host, sns_pks_compress, sns_pks_extract, glwe_phase128)
// as a stand-alone program, in the manner of san_check.cpp:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/sanitize/sns_pks_san.cpp tfhe_amd/csrc/client.cpp -o sns_pks_san -pthread && ./sns_pks_san
// Run by tests/test_sns_compression.py.  No GPU code.
#include <stdio.h>
#include <string.h>

#include <algorithm>
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

static uint64_t mix(uint64_t& s) {  // splitmix64: test inputs only
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// keygen, pack of `count` valid encryptions, the stored form and back, decryption of every message
static void run(const tfhe_sns_pks_params& pp, size_t count) {
  const size_t N = pp.out_N, k = pp.out_k, glwe_words = (k + 1) * 2 * N, ct_words = 2 * ((size_t)pp.in_dim + 1);
  std::vector<uint64_t> in_key(pp.in_dim), out_key(k * N), pksk(client::sns_pksk_len(pp));
  uint64_t s = 0x5A5;
  for (auto& b : in_key) b = mix(s) & 1;
  client::sns_pks_keygen(pp, client::rng_key_from_seed(0x5C0128), in_key.data(), out_key.data(), pksk.data());
  const u128 delta = ((u128)1 << 127) / 16;
  std::vector<uint64_t> lwes(count * ct_words);
  for (size_t q = 0; q < count; q++) {
    uint64_t* ct = lwes.data() + q * ct_words;
    u128 b = delta * (q % 16);
    for (size_t j = 0; j < pp.in_dim; j++) {
      // the edge words of the decomposition among random ones
      const u128 a = j % 11 == 3 ? ~(u128)0 : j % 11 == 7 ? (u128)1 << (127 - pp.base_log * pp.level)
                                                          : ((u128)mix(s) << 64) | mix(s);
      ct[2 * j] = (uint64_t)a;
      ct[2 * j + 1] = (uint64_t)(a >> 64);
      if (in_key[j]) b += a;
    }
    ct[2 * pp.in_dim] = (uint64_t)b;
    ct[2 * pp.in_dim + 1] = (uint64_t)(b >> 64);
  }
  const size_t lpg = pp.lwe_per_glwe, groups = (count + lpg - 1) / lpg;
  std::vector<uint64_t> glwes(groups * glwe_words), back(glwe_words), ph(2 * N);
  client::sns_pks_pack_host(pp, pksk.data(), lwes.data(), count, glwes.data());
  for (size_t g = 0; g < groups; g++) {
    const uint32_t bodies = (uint32_t)std::min(lpg, count - g * lpg);
    std::vector<uint64_t> packed(client::sns_pks_packed_words(pp, bodies));  // exact size: an overrun is reported
    client::sns_pks_compress(pp, glwes.data() + g * glwe_words, bodies, packed.data());
    client::sns_pks_extract(pp, packed.data(), bodies, back.data());
    if (pp.storage_log == 128) CHECK(!memcmp(back.data(), glwes.data() + g * glwe_words, (k * 2 * N) * 8));
    client::glwe_phase128(pp.out_k, pp.out_N, out_key.data(), back.data(), ph.data());
    for (uint32_t i = 0; i < bodies; i++) {
      const u128 x = ((u128)ph[N + i] << 64) | ph[i];
      CHECK((uint64_t)(((x + delta / 2) / delta) % 16) == (g * lpg + i) % 16);
    }
  }
  printf("in_dim %u k %u N %u 2^%u x %u storage %u: %zu ciphertexts decrypt\n", pp.in_dim, pp.out_k, pp.out_N,
         pp.base_log, pp.level, pp.storage_log, count);
}

int main() {
  run(tfhe_sns_pks_params{64, 1, 32, 61, 1, 32, 128, -62}, 2 * 32 + 5);  // set A of the tests
  run(tfhe_sns_pks_params{48, 2, 64, 20, 3, 20, 75, -62}, 21);           // stored values across three words
  run(tfhe_sns_pks_params{80, 1, 64, 63, 2, 64, 64, -62}, 1);            // widest digit, precision 126
  printf(fails ? "SNS PKS SANITIZE FAIL %d\n" : "SNS PKS SANITIZE OK\n", fails);
  return fails ? 1 : 0;
}
