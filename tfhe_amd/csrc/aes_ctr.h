// aes_ctr.h — the AES-128 block function of the seeded mask stream on the device, shared by csprng.hip (one seed per
// row, the key expanded per workgroup) and seeded_keys.hip (one seed per key, the round keys handed in).  Device code
// only; include it from a .hip file inside namespace-free scope.
//
// The T-table Te0[x] = (2 S(x), S(x), S(x), 3 S(x)) is built at compile time from the field arithmetic; a kernel
// stages its 256 words into LDS (te[tid] = TE0.v[tid] with 256 threads) so that every data-dependent lookup of the
// cipher is an LDS read.  Te1..Te3 are byte rotations of Te0 and the S-box is its second byte.  Words are little
// endian: state word c holds column c, its low byte row 0.
#pragma once
#include <hip/hip_runtime.h>

#include "gl64.h"

namespace tfhe {
namespace aes {

// ---- Te0, built at compile time (FIPS-197 §4.2, §5.1.1; the walk over the multiplicative group is init_sbox of
// seeded.cpp)
struct te_table {
  u32 v[256];
};

constexpr u32 rotl8(u32 x, int s) { return ((x << s) | (x >> (8 - s))) & 0xffu; }

constexpr te_table make_te0() {
  te_table t{};
  u32 sbox[256] = {};
  u32 p = 1, q = 1;
  do {
    p = (p ^ (p << 1) ^ ((p & 0x80u) ? 0x1bu : 0u)) & 0xffu;  // p *= 3
    q = (q ^ (q << 1)) & 0xffu;                                // q /= 3
    q = (q ^ (q << 2)) & 0xffu;
    q = (q ^ (q << 4)) & 0xffu;
    if (q & 0x80u) q ^= 0x09u;
    sbox[p] = q ^ rotl8(q, 1) ^ rotl8(q, 2) ^ rotl8(q, 3) ^ rotl8(q, 4) ^ 0x63u;
  } while (p != 1);
  sbox[0] = 0x63u;
  for (int x = 0; x < 256; x++) {
    const u32 s = sbox[x], s2 = ((s << 1) ^ ((s >> 7) * 0x1bu)) & 0xffu, s3 = s2 ^ s;
    t.v[x] = s2 | (s << 8) | (s << 16) | (s3 << 24);
  }
  return t;
}

static const __device__ te_table TE0 = make_te0();
static_assert(make_te0().v[0] == 0xa56363c6u && make_te0().v[0x53] == 0x2cededc1u, "Te0: S(00) = 63, S(53) = ed");

__device__ __forceinline__ u32 rotl32(u32 x, int s) { return (x << s) | (x >> (32 - s)); }
__device__ __forceinline__ u32 sub_byte(const u32* te, u32 x) { return (te[x] >> 8) & 0xffu; }

// one column of a full round: SubBytes + ShiftRows + MixColumns of the bytes (row r from column c + r)
__device__ __forceinline__ u32 round_col(const u32* te, u32 a, u32 b, u32 c, u32 d) {
  return te[a & 0xffu] ^ rotl32(te[(b >> 8) & 0xffu], 8) ^ rotl32(te[(c >> 16) & 0xffu], 16) ^ rotl32(te[d >> 24], 24);
}
__device__ __forceinline__ u32 last_col(const u32* te, u32 a, u32 b, u32 c, u32 d) {
  return sub_byte(te, a & 0xffu) | (sub_byte(te, (b >> 8) & 0xffu) << 8) | (sub_byte(te, (c >> 16) & 0xffu) << 16) |
         (sub_byte(te, d >> 24) << 24);
}

// AES-128 key expansion (FIPS-197 §5.2) on little-endian words: rk[0..3] = the key, rk[4 i ..] = round key i.  40
// dependent S-box reads: one lane's work
__device__ __forceinline__ void expand_key(const u32* te, u64 lo, u64 hi, u32* rk) {
  u32 w0 = (u32)lo, w1 = (u32)(lo >> 32), w2 = (u32)hi, w3 = (u32)(hi >> 32);
  rk[0] = w0, rk[1] = w1, rk[2] = w2, rk[3] = w3;
  u32 rcon = 1;
  for (int i = 1; i <= 10; i++) {
    const u32 t = (w3 >> 8) | (w3 << 24);  // RotWord
    w0 ^= last_col(te, t, t, t, t) ^ rcon;
    w1 ^= w0, w2 ^= w1, w3 ^= w2;
    rk[4 * i] = w0, rk[4 * i + 1] = w1, rk[4 * i + 2] = w2, rk[4 * i + 3] = w3;
    rcon = ((rcon << 1) ^ ((rcon >> 7) * 0x1bu)) & 0xffu;
  }
}

// Block b of the counter-mode stream (b as a 64-bit little-endian counter in the low 8 bytes, the high 8 bytes 0):
// the four output words, o[0] holding stream bytes 0..3 of the block.  rk: anything indexable with 44 words
template <class RK>
__device__ __forceinline__ void ctr_block(const u32* te, const RK& rk, u64 b, u32 o[4]) {
  u32 s0 = (u32)b ^ rk[0], s1 = (u32)(b >> 32) ^ rk[1], s2 = rk[2], s3 = rk[3];
#pragma unroll
  for (int round = 1; round < 10; round++) {
    const u32 t0 = round_col(te, s0, s1, s2, s3) ^ rk[4 * round];
    const u32 t1 = round_col(te, s1, s2, s3, s0) ^ rk[4 * round + 1];
    const u32 t2 = round_col(te, s2, s3, s0, s1) ^ rk[4 * round + 2];
    const u32 t3 = round_col(te, s3, s0, s1, s2) ^ rk[4 * round + 3];
    s0 = t0, s1 = t1, s2 = t2, s3 = t3;
  }
  o[0] = last_col(te, s0, s1, s2, s3) ^ rk[40];
  o[1] = last_col(te, s1, s2, s3, s0) ^ rk[41];
  o[2] = last_col(te, s2, s3, s0, s1) ^ rk[42];
  o[3] = last_col(te, s3, s0, s1, s2) ^ rk[43];
}

// The stream starts at byte 1, so word w is stream bytes 1 + 8 w .. 8 + 8 w: block b holds word 2b (its bytes 1..8),
// the low 7 bytes of word 2b + 1 (bytes 9..15) and, in its byte 0, the top byte of word 2b - 1.  Returns (word 2b,
// word 2b + 1 with a zero top byte); *top = byte 0
__device__ __forceinline__ ulonglong2 block_words(const u32 o[4], unsigned char* top) {
  const u64 lo = (u64)o[0] | ((u64)o[1] << 32), hi = (u64)o[2] | ((u64)o[3] << 32);
  ulonglong2 pair;
  pair.x = (lo >> 8) | (hi << 56);
  pair.y = hi >> 8;
  *top = (unsigned char)(o[0] & 0xffu);
  return pair;
}

}  // namespace aes
}  // namespace tfhe
