// csprng.hip — the seeded mask stream on the device: AES-128 in counter mode, one seed per output row (the mask half
// of tfhe-rs ServerKey::generate_oblivious_pseudo_random*; seeded.cpp states the stream and is the host reference).
//
// Stream of a seed (lo, hi), as seeded.cpp restates tfhe-csprng's AesCtrGenerator (PARITY UNPINNED at the byte
// level; AES-128 itself is pinned by FIPS-197): key = the seed's 16 bytes, little endian; block b =
// AES_key(b as a 64-bit little-endian counter in the low 8 bytes, high 8 bytes 0); the stream starts at byte 1, so
// word w is stream bytes 1 + 8w .. 8 + 8w, little endian.  A block b therefore holds word 2b (its bytes 1..8), the
// low 7 bytes of word 2b + 1 (bytes 9..15) and the top byte of word 2b - 1 (byte 0).
//
// Grid: rows x chunks.  A workgroup writes CS_CHUNK = 1022 consecutive words of one row: whatever the parity of its
// first word, those lie in at most 512 blocks, two per lane.  A row of 918 words is one workgroup (460 blocks), a
// 4096-row call 4096 workgroups; one long row (a key's mask run) spreads over ceil(dim / 1022) workgroups, each of
// which recomputes the one or two boundary blocks it shares with its neighbours.
//
// LDS (9.9 KB): the T-table Te0 (1 KB, staged once per workgroup from the static table below; Te1..Te3 are byte
// rotations of it and the S-box is its second byte), the row's 44 round-key words (lane 0 expands the key after
// the table is staged), and the exchange area: a lane stores the two words of its block as one 16-byte LDS write
// (odd word with a zero top byte) plus the block's byte 0 into a byte array; after one barrier the lanes read the
// chunk back in word order, OR the straddling byte from the next block into the odd words, and store
// lane-contiguous 8-byte words (rows are only 8-byte aligned: n + 1 is odd for n = 918).  Every data-dependent
// lookup of the cipher is an LDS read.
#include <hip/hip_runtime.h>

#include "pbs_kernels.h"

namespace tfhe {
namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_CHUNK = 1022;       // words per workgroup
constexpr int CS_MAX_BLOCKS = 512;   // AES blocks that CS_CHUNK words can touch

// ---- Te0[x] = (2 S(x), S(x), S(x), 3 S(x)) as a little-endian column, built at compile time from the field
// arithmetic (FIPS-197 §4.2, §5.1.1; the walk over the multiplicative group is init_sbox of seeded.cpp)
struct te_table {
  u32 v[256];
};

constexpr u32 cs_rotl8(u32 x, int s) { return ((x << s) | (x >> (8 - s))) & 0xffu; }

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
    sbox[p] = q ^ cs_rotl8(q, 1) ^ cs_rotl8(q, 2) ^ cs_rotl8(q, 3) ^ cs_rotl8(q, 4) ^ 0x63u;
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

// grid: rows * chunks workgroups, index r * chunks + c
__global__ __launch_bounds__(CS_THREADS) void csprng_rows_kernel(const u64* __restrict__ seeds, unsigned chunks,
                                                                 u64 first_word, u32 dim, size_t row_stride,
                                                                 int zero_body, u64* __restrict__ out) {
  __shared__ u32 te[256];
  __shared__ u32 rk[44];
  __shared__ __attribute__((aligned(16))) u64 wbuf[2 * CS_MAX_BLOCKS];  // words 2 b0 .. of the chunk's blocks
  __shared__ unsigned char top[CS_MAX_BLOCKS];                          // byte 0 of every block
  const int tid = threadIdx.x;
  const size_t r = blockIdx.x / chunks;
  const u32 w_lo = (blockIdx.x % chunks) * (u32)CS_CHUNK;  // first word of this chunk within the row (< dim)
  const u32 cnt = min((u32)CS_CHUNK, dim - w_lo);
  const u64 w_first = first_word + w_lo;
  const u64 b0 = w_first >> 1;
  const int nblk = (int)(((w_first + cnt) >> 1) - b0) + 1;  // through the block of the last word's top byte; <= 512

  te[tid] = TE0.v[tid];
  __syncthreads();
  if (tid == 0) {  // AES-128 key expansion (FIPS-197 §5.2) on little-endian words
    const u64 lo = seeds[2 * r], hi = seeds[2 * r + 1];
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
  __syncthreads();

  for (int j = tid; j < nblk; j += CS_THREADS) {
    const u64 b = b0 + (u64)j;
    u32 s0 = (u32)b ^ rk[0], s1 = (u32)(b >> 32) ^ rk[1], s2 = rk[2], s3 = rk[3];
#pragma unroll
    for (int round = 1; round < 10; round++) {
      const u32 t0 = round_col(te, s0, s1, s2, s3) ^ rk[4 * round];
      const u32 t1 = round_col(te, s1, s2, s3, s0) ^ rk[4 * round + 1];
      const u32 t2 = round_col(te, s2, s3, s0, s1) ^ rk[4 * round + 2];
      const u32 t3 = round_col(te, s3, s0, s1, s2) ^ rk[4 * round + 3];
      s0 = t0, s1 = t1, s2 = t2, s3 = t3;
    }
    const u32 o0 = last_col(te, s0, s1, s2, s3) ^ rk[40];
    const u32 o1 = last_col(te, s1, s2, s3, s0) ^ rk[41];
    const u32 o2 = last_col(te, s2, s3, s0, s1) ^ rk[42];
    const u32 o3 = last_col(te, s3, s0, s1, s2) ^ rk[43];
    const u64 lo = (u64)o0 | ((u64)o1 << 32), hi = (u64)o2 | ((u64)o3 << 32);
    ulonglong2 pair;
    pair.x = (lo >> 8) | (hi << 56);  // word 2b: bytes 1..8
    pair.y = hi >> 8;                 // word 2b + 1: bytes 9..15; its top byte is byte 0 of block b + 1
    *(ulonglong2*)&wbuf[2 * j] = pair;
    top[j] = (unsigned char)(o0 & 0xffu);
  }
  __syncthreads();

  u64* row = out + r * row_stride + w_lo;
  const u32 odd = (u32)(w_first & 1);
  for (u32 i = tid; i < cnt; i += CS_THREADS) {
    const u32 e = odd + i;  // index from word 2 b0; an odd e takes its top byte from block (e + 1) / 2 < nblk
    u64 v = wbuf[e];
    if (e & 1) v |= (u64)top[(e + 1) >> 1] << 56;
    row[i] = v;
  }
  if (zero_body && tid == 0 && w_lo + cnt == dim) row[cnt] = 0;
}

// body of row r += post_add[idx ? idx[r] : 0]; an index past n_lut leaves the row alone
__global__ __launch_bounds__(CS_THREADS) void body_add_kernel(u64* __restrict__ lwes, unsigned rows, size_t row_len,
                                                              const u64* __restrict__ post_add, unsigned n_lut,
                                                              const u32* __restrict__ idx) {
  const unsigned r = blockIdx.x * CS_THREADS + threadIdx.x;
  if (r >= rows) return;
  const u32 l = idx ? idx[r] : 0;
  if (l < n_lut) lwes[(size_t)r * row_len + row_len - 1] += post_add[l];
}

}  // namespace

hipError_t launch_csprng_rows(const u64* seeds, size_t rows, u64 first_word, u32 dim, size_t row_stride,
                              bool zero_body, u64* out, hipStream_t s) {
  if (rows == 0 || dim == 0) return hipSuccess;
  if (!seeds || !out || row_stride < (size_t)dim + (zero_body ? 1 : 0) || first_word > (1ull << 60) ||
      dim > (1ull << 60) - first_word)
    return hipErrorInvalidValue;
  const size_t chunks = ((size_t)dim + CS_CHUNK - 1) / CS_CHUNK;
  if (rows > 0x7FFFFFFF / chunks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(csprng_rows_kernel, dim3((unsigned)(rows * chunks)), dim3(CS_THREADS), 0, s, seeds,
                     (unsigned)chunks, first_word, dim, row_stride, zero_body ? 1 : 0, out);
  return hipGetLastError();
}

hipError_t launch_body_add(u64* lwes, size_t rows, size_t row_len, const u64* post_add, size_t n_lut, const u32* idx,
                           hipStream_t s) {
  if (rows == 0) return hipSuccess;
  if (!lwes || !post_add || row_len == 0 || n_lut == 0 || rows > 0x7FFFFFFF || n_lut > 0xFFFFFFFFu)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(body_add_kernel, dim3((unsigned)((rows + CS_THREADS - 1) / CS_THREADS)), dim3(CS_THREADS), 0, s,
                     lwes, (unsigned)rows, row_len, post_add, (unsigned)n_lut, idx);
  return hipGetLastError();
}

}  // namespace tfhe
