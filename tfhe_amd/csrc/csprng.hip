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
// LDS (9.9 KB): the T-table Te0 (1 KB, staged once per workgroup from the static table of aes_ctr.h, which holds the
// cipher's round functions for this file and seeded_keys.hip; Te1..Te3 are byte rotations of it and the S-box is its
// second byte), the row's 44 round-key words (lane 0 expands the key after the table is staged), and the exchange
// area: a lane stores the two words of its block as one 16-byte LDS write (odd word with a zero top byte) plus the block's byte 0 into a byte array; after one barrier the lanes read the
// chunk back in word order, OR the straddling byte from the next block into the odd words, and store
// lane-contiguous 8-byte words (rows are only 8-byte aligned: n + 1 is odd for n = 918).  Every data-dependent
// lookup of the cipher is an LDS read.
#include <hip/hip_runtime.h>

#include "aes_ctr.h"
#include "pbs_kernels.h"

namespace tfhe {
namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_CHUNK = 1022;       // words per workgroup
constexpr int CS_MAX_BLOCKS = 512;   // AES blocks that CS_CHUNK words can touch

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

  te[tid] = aes::TE0.v[tid];
  __syncthreads();
  if (tid == 0) aes::expand_key(te, seeds[2 * r], seeds[2 * r + 1], rk);
  __syncthreads();

  for (int j = tid; j < nblk; j += CS_THREADS) {
    u32 o[4];
    aes::ctr_block(te, rk, b0 + (u64)j, o);
    *(ulonglong2*)&wbuf[2 * j] = aes::block_words(o, &top[j]);  // word 2b + 1's top byte is byte 0 of block b + 1
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
