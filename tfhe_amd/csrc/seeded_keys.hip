// seeded_keys.hip — seeded (compressed) server keys expanded on the device: from one 128-bit seed and a body buffer
// to finished standard-domain rows in this engine's key layouts (seeded.cpp decompress_bsk / decompress_bsk_mb /
// decompress_ksk / decompress_lwe_list are the host references, word for word).  The mask stream is that of
// csprng.hip (AES-128 in counter mode from byte 1, aes_ctr.h); PARITY UNPINNED at the byte level, DESIGN §7h.
//
// One kernel for the four key kinds.  A stored row t has a source index rho (its place in the seed's stream and in
// the body buffer) and a destination row, both closed forms of t:
//   LWE list          t = z                                   rho = t                        dst = t
//   keyswitching key  t = j LV + s                            rho = t                        dst = j LV + (LV - 1 - s)
//   classic BSK       t = (i L + l)(k + 1) + c                rho = t                        dst = i (k+1) L + c L + l
//   multi-bit BSK     t = ((q (2^g - 1) + sigma - 1) L + l)(k + 1) + c, sigma >= 1           dst = t
//                                                             rho = ((q 2^g + sigma) L + l)(k + 1) + c
// Row rho owns stream words rho * mask_len .. and body words rho * body_len ..; a destination row is mask_len mask
// words followed by body_len body words.  The container's sigma = 0 GGSWs are never launched: their bodies are not
// read and their stream words are stepped over by rho.
//
// Grid: rows x chunks.  A workgroup of 256 lanes writes SK_CHUNK = 2048 consecutive mask words of one row, which lie
// in at most 1025 blocks whatever the parity of the first word (a block owns word 2b, seven bytes of word 2b + 1 and
// the top byte of word 2b - 1), so four blocks per lane and one more on lane 0; a bootstrapping-key row at k = 1,
// N = 2048 is one workgroup, a keyswitching-key row of n = 918 words one workgroup of 460 blocks.  The chunk's share
// of the row's body words is copied by the same workgroup.
//
// Round keys: thousands of workgroups share one seed here, so the key schedule runs once per seed on the host
// (seeded.cpp aes_round_keys) and the 44 words travel as a kernel argument: every use is a scalar read at a constant
// offset, and no lane walks the 40 dependent S-box reads of the schedule.
//
// LDS (18.4 KB): Te0 (1 KB), the exchange area (a lane stores the two words of a block as one 16-byte write plus the
// block's byte 0 into a byte array), read back after one barrier.  A chunk that starts on an even stream word at a
// 16-byte-aligned address (every bootstrapping-key row) is read back as 16-byte pairs, the straddling byte OR-ed
// into the odd word, and stored lane-contiguous 16 bytes wide; any other chunk (keyswitching-key and list rows are
// n + 1 words, so only 8-byte aligned, and rows of odd n alternate parity) as lane-contiguous 8-byte words.
#include <hip/hip_runtime.h>

#include "aes_ctr.h"
#include "pbs_kernels.h"

namespace tfhe {
namespace {

constexpr int SK_THREADS = 256;
constexpr u32 SK_CHUNK = 2048;        // mask words per workgroup
constexpr int SK_MAX_BLOCKS = 1025;   // AES blocks that SK_CHUNK words can touch

struct sk_plan {
  u32 kind;      // seeded_kind
  u32 mask_len;  // mask words of a row
  u32 body_len;  // body words of a row
  u32 chunks;    // ceil(mask_len / SK_CHUNK)
  u32 L, k1;     // bootstrapping keys: levels, k + 1
  u32 LV;        // keyswitching key: levels
  u32 g;         // multi-bit: grouping factor
};

struct sk_row {
  u64 src, dst;
};

__device__ __forceinline__ sk_row row_map(const sk_plan& P, u32 t) {
  sk_row r{t, t};
  if (P.kind == SEEDED_KSK) {
    const u32 j = t / P.LV, s = t % P.LV;
    r.dst = (u64)j * P.LV + (P.LV - 1 - s);
  } else if (P.kind == SEEDED_BSK) {
    const u32 c = t % P.k1, il = t / P.k1, l = il % P.L, i = il / P.L;
    r.dst = ((u64)i * P.k1 + c) * P.L + l;
  } else if (P.kind == SEEDED_BSK_MB) {
    const u32 per_ggsw = P.L * P.k1, per_q = (1u << P.g) - 1;
    const u32 in_ggsw = t % per_ggsw, ggsw = t / per_ggsw;  // ggsw = q (2^g - 1) + sigma - 1
    const u32 q = ggsw / per_q, sigma = ggsw % per_q + 1;
    r.src = ((u64)q * (per_q + 1) + sigma) * per_ggsw + in_ggsw;
  }
  return r;
}

// grid: rows * chunks workgroups, index t * chunks + c
__global__ __launch_bounds__(SK_THREADS) void seeded_rows_kernel(const seeded_round_keys rk, const sk_plan P,
                                                                 const u64* __restrict__ bodies,
                                                                 u64* __restrict__ out) {
  __shared__ u32 te[256];
  __shared__ __attribute__((aligned(16))) u64 wbuf[2 * SK_MAX_BLOCKS];  // words 2 b0 .. of the chunk's blocks
  __shared__ unsigned char top[SK_MAX_BLOCKS];                          // byte 0 of every block
  const int tid = threadIdx.x;
  const u32 t = blockIdx.x / P.chunks, ch = blockIdx.x % P.chunks;
  const sk_row r = row_map(P, t);
  const u32 w_lo = ch * SK_CHUNK;  // first mask word of this chunk within the row (< mask_len)
  const u32 cnt = min(SK_CHUNK, P.mask_len - w_lo);
  const u64 w_first = r.src * P.mask_len + w_lo;
  const u64 b0 = w_first >> 1;
  const int nblk = (int)(((w_first + cnt) >> 1) - b0) + 1;  // through the block of the last word's top byte; <= 1025

  te[tid] = aes::TE0.v[tid];
  __syncthreads();
  for (int j = tid; j < nblk; j += SK_THREADS) {
    u32 o[4];
    aes::ctr_block(te, rk.w, b0 + (u64)j, o);
    *(ulonglong2*)&wbuf[2 * j] = aes::block_words(o, &top[j]);
  }
  __syncthreads();

  u64* row = out + r.dst * ((u64)P.mask_len + P.body_len);
  u64* dst = row + w_lo;
  const u32 odd = (u32)(w_first & 1);
  if (!odd && ((uintptr_t)dst & 15) == 0) {  // pair i = block i: its two words, the odd one's top byte from block i + 1
    for (u32 i = tid; i < cnt / 2; i += SK_THREADS) {
      ulonglong2 v = *(const ulonglong2*)&wbuf[2 * i];
      v.y |= (u64)top[i + 1] << 56;
      *(ulonglong2*)&dst[2 * i] = v;
    }
    if ((cnt & 1) && tid == 0) dst[cnt - 1] = wbuf[cnt - 1];
  } else {
    for (u32 i = tid; i < cnt; i += SK_THREADS) {
      const u32 e = odd + i;  // index from word 2 b0; an odd e takes its top byte from block (e + 1) / 2 < nblk
      u64 v = wbuf[e];
      if (e & 1) v |= (u64)top[(e + 1) >> 1] << 56;
      dst[i] = v;
    }
  }
  // this chunk's share of the row's body words
  const u32 y_lo = (u32)((u64)P.body_len * ch / P.chunks), y_hi = (u32)((u64)P.body_len * (ch + 1) / P.chunks);
  const u64* bsrc = bodies + r.src * P.body_len;
  u64* bdst = row + P.mask_len;
  if ((((uintptr_t)bsrc | (uintptr_t)bdst) & 15) == 0 && !((y_lo | y_hi) & 1)) {
    for (u32 i = y_lo / 2 + tid; i < y_hi / 2; i += SK_THREADS) ((ulonglong2*)bdst)[i] = ((const ulonglong2*)bsrc)[i];
  } else {
    for (u32 i = y_lo + tid; i < y_hi; i += SK_THREADS) bdst[i] = bsrc[i];
  }
}

// element-major transpose of the modulus-switch zeros: rows [count][dim] -> [dim][pitch], padding columns zero
__global__ __launch_bounds__(SK_THREADS) void zeros_transpose_kernel(const u64* __restrict__ rows, u32 count, u32 dim,
                                                                     u32 pitch, u64* __restrict__ tr) {
  const size_t idx = (size_t)blockIdx.x * SK_THREADS + threadIdx.x;
  if (idx >= (size_t)dim * pitch) return;
  const u32 i = (u32)(idx / pitch), z = (u32)(idx % pitch);
  tr[idx] = z < count ? rows[(size_t)z * dim + i] : 0;
}

}  // namespace

hipError_t launch_seeded_rows(const seeded_round_keys& rk, seeded_kind kind, const seeded_shape& sh, const u64* bodies,
                              u64* out, hipStream_t s) {
  sk_plan P{};
  P.kind = (u32)kind;
  P.L = sh.L, P.k1 = sh.k + 1, P.LV = sh.LV, P.g = sh.g;
  u64 rows = 0, src_rows = 0;
  switch (kind) {
    case SEEDED_LIST:
      P.mask_len = sh.n, P.body_len = 1;
      rows = src_rows = sh.count;
      break;
    case SEEDED_KSK:
      if (!sh.LV) return hipErrorInvalidValue;
      P.mask_len = sh.n, P.body_len = 1;
      rows = src_rows = (u64)sh.k * sh.N * sh.LV;
      break;
    case SEEDED_BSK:
      if (!sh.L) return hipErrorInvalidValue;
      P.mask_len = sh.k * sh.N, P.body_len = sh.N;
      rows = src_rows = (u64)sh.n * sh.L * (sh.k + 1);
      break;
    case SEEDED_BSK_MB:
      if (!sh.L || sh.g < 2 || sh.g > 4 || sh.n % sh.g) return hipErrorInvalidValue;
      P.mask_len = sh.k * sh.N, P.body_len = sh.N;
      rows = (u64)(sh.n / sh.g) * ((1u << sh.g) - 1) * sh.L * (sh.k + 1);
      src_rows = (u64)(sh.n / sh.g) * (1u << sh.g) * sh.L * (sh.k + 1);
      break;
    default:
      return hipErrorInvalidValue;
  }
  if (rows == 0) return hipSuccess;
  if (!bodies || !out || P.mask_len == 0 || (u64)sh.k * sh.N > 0x7FFFFFFFull) return hipErrorInvalidValue;
  P.chunks = (P.mask_len + SK_CHUNK - 1) / SK_CHUNK;
  if (rows * P.chunks > 0x7FFFFFFFull || src_rows > (1ull << 60) / P.mask_len) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seeded_rows_kernel, dim3((unsigned)(rows * P.chunks)), dim3(SK_THREADS), 0, s, rk, P, bodies, out);
  return hipGetLastError();
}

hipError_t launch_ms_zeros_transpose(const u64* rows, u32 count, u32 dim, u64* tr, hipStream_t s) {
  const size_t pitch = ms_zeros_pitch(count), total = (size_t)dim * pitch;
  if (total == 0) return hipSuccess;
  if (!rows || !tr || pitch > 0xFFFFFFFFull || (total + SK_THREADS - 1) / SK_THREADS > 0x7FFFFFFFull)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(zeros_transpose_kernel, dim3((unsigned)((total + SK_THREADS - 1) / SK_THREADS)), dim3(SK_THREADS),
                     0, s, rows, count, dim, (u32)pitch, tr);
  return hipGetLastError();
}

}  // namespace tfhe
