// seeded_keys128.hip — seeded 128-bit keys expanded on the device: the noise-squashing bootstrapping key and the ct128
// packing keyswitch key, from one 128-bit seed and a body buffer to finished rows in the plane layouts that
// sns_bsk_to_fft and the packing GEMM read (seeded.cpp sns_decompress_bsk / sns_pks_decompress_key are the host
// references, word for word).  The mask stream is that of seeded_keys.hip (AES-128 in counter mode from byte 1,
// aes_ctr.h) read 16 bytes at a time: u128 word w = stream bytes 16 w + 1 .. 16 w + 16 = block w less its byte 0, plus
// byte 0 of block w + 1.  PARITY UNPINNED at the byte level, DESIGN §7h''.
//
// A launched row t (relative to the launch's first row, which starts a unit of whole GGSWs / input elements) has a
// stream row rho and a destination row, both closed forms of t:
//   squashing key   t = (i L + l)(k + 1) + c      rho = row0 + t      dst = i (k + 1) L + c L + l
//   packing key     t = j L + s                   rho = row0 + t      dst = j L + (L - 1 - s)
// Stream row rho owns u128 mask words rho k N .. (polynomial p, then coefficient) and the body pairs t N .. of the
// launch's body buffer; a destination row is k + 1 polynomials of two planes [lo][N], [hi][N], the body last.
//
// Grid: rows x k.  A workgroup of 256 lanes produces the mask words of one (row, polynomial): N u128 words from N + 1
// blocks, lane-contiguous blocks so that the cipher's cost is spread evenly, in passes of SK128_CHUNK = 2048 words
// (one pass up to N = 2048, the squashing key; a larger packing ring loops).  Every block is stored into LDS as its
// word (lo, hi less the top byte) and its byte 0; after one barrier a lane reads two neighbouring words back as
// 16-byte LDS reads, ORs bytes 0 of blocks 2 i + 1 and 2 i + 2 into the hi words and writes the lo plane and the hi
// plane with lane-contiguous 16-byte stores (N is a power of two >= 32 and the buffers are 16-byte aligned, so every
// plane is).  The row's body pairs are de-interleaved into the body polynomial's planes by the row's k workgroups, an
// even share of pairs each: two pairs per lane, 32 contiguous bytes in, 16 bytes out to each plane.
//
// Round keys: as seeded_keys.hip, the key schedule runs once per seed on the host (seeded.cpp aes_round_keys) and the
// 44 words travel as a kernel argument.  LDS 35.9 KB: Te0 (1 KB), lo and hi words (2 x 16.4 KB), bytes 0 (2 KB).
#include <hip/hip_runtime.h>

#include "aes_ctr.h"
#include "pbs_kernels.h"

namespace tfhe {
namespace {

constexpr int SK128_THREADS = 256;
constexpr u32 SK128_CHUNK = 2048;  // u128 mask words per pass

struct sk128_plan {
  u32 kind;  // seeded128_kind
  u32 N;     // polynomial size
  u32 k;     // mask polynomials of a row
  u32 L;     // levels
  u64 row0;  // stream row of the first launched row
};

// grid: rows * k workgroups, index t * k + p
__global__ __launch_bounds__(SK128_THREADS) void seeded_rows128_kernel(const seeded_round_keys rk, const sk128_plan P,
                                                                       const u64* __restrict__ bodies,
                                                                       u64* __restrict__ out) {
  __shared__ u32 te[256];
  __shared__ __attribute__((aligned(16))) u64 wlo[SK128_CHUNK + 2];  // word b (low half) of the pass's blocks
  __shared__ __attribute__((aligned(16))) u64 whi[SK128_CHUNK + 2];  // high half, top byte zero
  __shared__ unsigned char top[SK128_CHUNK + 4];                     // byte 0 of every block
  const u32 tid = threadIdx.x;
  const u32 t = blockIdx.x / P.k, p = blockIdx.x % P.k;
  const u32 N = P.N;
  u64 dst;
  if (P.kind == SEEDED128_SNS_BSK) {
    const u32 k1 = P.k + 1, c = t % k1, il = t / k1, l = il % P.L, i = il / P.L;
    dst = ((u64)i * k1 + c) * P.L + l;
  } else {
    const u32 j = t / P.L, s = t % P.L;
    dst = (u64)j * P.L + (P.L - 1 - s);
  }
  u64* row = out + dst * ((u64)(P.k + 1) * 2 * N);
  u64* plane_lo = row + (u64)p * 2 * N;
  u64* plane_hi = plane_lo + N;
  const u64 w_first = ((P.row0 + t) * P.k + p) * N;  // the polynomial's first u128 word = its first block

  te[tid] = aes::TE0.v[tid];
  for (u32 c0 = 0; c0 < N; c0 += SK128_CHUNK) {
    const u32 cnt = min(SK128_CHUNK, N - c0);  // even: N is a power of two >= 32
    __syncthreads();                           // Te0 staged; the previous pass's words read
    for (u32 j = tid; j <= cnt; j += SK128_THREADS) {
      u32 o[4];
      aes::ctr_block(te, rk.w, w_first + c0 + j, o);
      const ulonglong2 w = aes::block_words(o, &top[j]);
      wlo[j] = w.x;
      whi[j] = w.y;
    }
    __syncthreads();
    for (u32 i = tid; i < cnt / 2; i += SK128_THREADS) {
      const ulonglong2 lo = *(const ulonglong2*)&wlo[2 * i];
      ulonglong2 hi = *(const ulonglong2*)&whi[2 * i];
      hi.x |= (u64)top[2 * i + 1] << 56;
      hi.y |= (u64)top[2 * i + 2] << 56;
      *(ulonglong2*)&plane_lo[c0 + 2 * i] = lo;
      *(ulonglong2*)&plane_hi[c0 + 2 * i] = hi;
    }
  }

  // this workgroup's share of the row's body pairs, in twos: [y_lo, y_hi) of N / 2
  const u32 y_lo = (u32)((u64)(N / 2) * p / P.k), y_hi = (u32)((u64)(N / 2) * (p + 1) / P.k);
  const ulonglong2* bsrc = (const ulonglong2*)(bodies + (u64)t * 2 * N);
  u64* body_lo = row + (u64)P.k * 2 * N;
  u64* body_hi = body_lo + N;
  for (u32 i = y_lo + tid; i < y_hi; i += SK128_THREADS) {
    const ulonglong2 a = bsrc[2 * i], b = bsrc[2 * i + 1];  // pairs 2 i and 2 i + 1: (lo, hi), (lo, hi)
    ulonglong2 lo, hi;
    lo.x = a.x, lo.y = b.x;
    hi.x = a.y, hi.y = b.y;
    *(ulonglong2*)&body_lo[2 * i] = lo;
    *(ulonglong2*)&body_hi[2 * i] = hi;
  }
}

}  // namespace

hipError_t launch_seeded_rows128(const seeded_round_keys& rk, seeded128_kind kind, const seeded128_shape& sh, u64 row0,
                                 u64 rows, const u64* bodies, u64* out, hipStream_t s) {
  if (kind != SEEDED128_SNS_BSK && kind != SEEDED128_SNS_PKSK) return hipErrorInvalidValue;
  if (!sh.k || !sh.L || sh.N < 32 || (sh.N & (sh.N - 1))) return hipErrorInvalidValue;
  const u64 unit = kind == SEEDED128_SNS_BSK ? (u64)sh.L * (sh.k + 1) : sh.L;  // rows of one GGSW / input element
  if (row0 % unit || rows % unit) return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  if (!bodies || !out || (((uintptr_t)bodies | (uintptr_t)out) & 15)) return hipErrorInvalidValue;
  // grid and stream-word limits: rows k workgroups, (row0 + rows) k N blocks
  if (rows * sh.k > 0x7FFFFFFFull || (row0 + rows) > (1ull << 60) / ((u64)sh.k * sh.N)) return hipErrorInvalidValue;
  sk128_plan P{};
  P.kind = (u32)kind, P.N = sh.N, P.k = sh.k, P.L = sh.L, P.row0 = row0;
  hipLaunchKernelGGL(seeded_rows128_kernel, dim3((unsigned)(rows * sh.k)), dim3(SK128_THREADS), 0, s, rk, P, bodies,
                     out);
  return hipGetLastError();
}

}  // namespace tfhe
