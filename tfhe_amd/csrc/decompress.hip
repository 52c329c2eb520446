// decompress.hip — unpack compressed GLWEs and sample-extract their coefficients (the first half of tfhe-rs
// CompressedCiphertextList::get / DecompressionKey::unpack; the blind rotation that follows is the PBS kernels').
//
// Input: G = ceil(count / lpg) compressed GLWEs back to back, each as tfhe_hip_pks_compress writes it: value v at
// bit v * w (LSB first, may straddle two words), the k N mask coefficients first, then only the group's own
// bodies (lpg of them, the remainder in the last group); every group but the last is words(lpg) long.  Output row
// q = g * lpg + i is the LWE of coefficient i of group g on the native torus, with val = stored << (64 - w):
//   a'[cN + j] =  val(c, i - j)       (j <= i)
//   a'[cN + j] = -val(c, N + i - j)   (j >  i)        b' = body(i)
//
// One workgroup per (group, mask polynomial, tile of DX_ROWS rows): it unpacks its polynomial into LDS once
// (N stored values = N w / 8 bytes of reads, lanes on consecutive values) and writes its rows from that copy.
// The grid therefore grows with count: a full group at N = 2048 is 2048 rows x 2049 words = 33 MB of stores, spread
// over 256 workgroups; the price is that each tile re-reads the 6.7 KB polynomial.  The rows of a tile are one flat
// index space e = r N + j, so every lane stores at small N too; within a row the stores are ascending j,
// lane-contiguous 8-byte words (rows are kN + 1 long: only 8-byte aligned), and the LDS read of lane j is word
// (i - j) mod N: descending consecutive words, no bank conflict (as sample_extract_many.hip).  N is a power of two:
// the row / column split is a shift and a mask, the wrap a mask and a sign test; the only divisions are the three
// that decode the workgroup index, once per workgroup.
#include <hip/hip_runtime.h>

#include "pbs_kernels.h"

namespace tfhe {
namespace {

constexpr int DX_THREADS = 256;
constexpr int DX_ROWS = 8;       // rows per workgroup
constexpr int DX_MAX_N = 4096;   // 32 KB of LDS

// stored value v of a group, moved to the top of the word
__device__ __forceinline__ u64 dx_value(const u64* __restrict__ grp, size_t v, int w) {
  const size_t bit = v * (size_t)w, word = bit >> 6;
  const int off = (int)(bit & 63);
  u64 ms = grp[word] >> off;
  if (off + w > 64) ms |= grp[word + 1] << (64 - off);  // the value ends in the next word, which the group owns
  return ms << (64 - w);                                // drops the bits above w
}

// grid: G * tiles * k workgroups, index ((g * tiles) + t) * k + c; dynamic LDS: N words
__global__ __launch_bounds__(DX_THREADS) void unpack_extract_kernel(const u64* __restrict__ packed, unsigned count,
                                                                    int k, int logN, unsigned lpg, int w,
                                                                    unsigned tiles, size_t group_words,
                                                                    u64* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) u64 poly[];
  const int tid = threadIdx.x;
  const int N = 1 << logN;
  const unsigned c = blockIdx.x % (unsigned)k, gt = blockIdx.x / (unsigned)k;
  const unsigned g = gt / tiles, t = gt % tiles;
  const unsigned bodies = min(lpg, count - g * lpg);  // g < G, so count - g * lpg >= 1
  const unsigned i0 = t * DX_ROWS;
  if (i0 >= bodies) return;  // a tile past the last group's remainder (uniform over the workgroup)
  const unsigned rows = min((unsigned)DX_ROWS, bodies - i0);
  const u64* grp = packed + (size_t)g * group_words;
  for (int j = tid; j < N; j += DX_THREADS) poly[j] = dx_value(grp, ((size_t)c << logN) + j, w);
  __syncthreads();
  const size_t big = ((size_t)k << logN) + 1;
  u64* row0 = out + ((size_t)g * lpg + i0) * big + ((size_t)c << logN);
  for (unsigned e = tid; e < (rows << logN); e += DX_THREADS) {
    const unsigned r = e >> logN;
    const int j = (int)(e & (unsigned)(N - 1)), idx = (int)(i0 + r) - j;
    const u64 v = poly[idx & (N - 1)];
    row0[r * big + j] = idx < 0 ? 0 - v : v;
  }
  if (c == 0 && tid < (int)rows) row0[tid * big + ((size_t)k << logN)] = dx_value(grp, ((size_t)k << logN) + i0 + tid, w);
}

}  // namespace

hipError_t launch_unpack_extract(const u64* packed, size_t count, int k, int N, int lpg, int w, u64* out,
                                 hipStream_t s) {
  if (count == 0) return hipSuccess;
  if (k < 1 || N < 2 || N > DX_MAX_N || (N & (N - 1)) || lpg < 1 || lpg > N || w < 1 || w > 63 ||
      count > 0x7FFFFFFF || !packed || !out)
    return hipErrorInvalidValue;
  int logN = 0;
  while ((1 << logN) < N) logN++;
  const size_t groups = (count + lpg - 1) / lpg, tiles = ((size_t)lpg + DX_ROWS - 1) / DX_ROWS;
  const size_t wgs = groups * tiles * (size_t)k;
  if (wgs > 0x7FFFFFFF) return hipErrorInvalidValue;
  const size_t group_words = (((size_t)k * N + lpg) * w + 63) / 64;
  hipLaunchKernelGGL(unpack_extract_kernel, dim3((unsigned)wgs), dim3(DX_THREADS), (size_t)N * sizeof(u64), s, packed,
                     (unsigned)count, k, logN, (unsigned)lpg, w, (unsigned)tiles, group_words, out);
  return hipGetLastError();
}

}  // namespace tfhe
