// expand.hip — expand a compact ciphertext list into LWE ciphertexts (tfhe-rs CompactCiphertextList::expand on the
// LWE level; the casting PBS that follows is the PBS kernels').
//
// Input: the list's `data: Vec<u64>` as tfhe-rs stores it: bins x N mask words, bins = ceil(count / N), then count
// body words.  Output row r is list entry q = r / rep (rep consecutive copies of every entry: one row per radix
// block of a packed list at rep = 2), in bin g = q / N at degree i = q % N, with M the mask polynomial of bin g:
//   a[k] =  M[k + i + 1 - N]   (k + i + 1 >= N)
//   a[k] = -M[k + i + 1]       (otherwise)            b = bodies[q]
// (tfhe_amd/ctlist.py: expand).
//
// One workgroup per tile of EX_ROWS output rows: it stages its bin's mask polynomial into LDS once and writes its
// rows from that copy.  A bin has N * rep rows, which EX_ROWS divides for every allowed N, so tiles are cut per bin
// and a tile never straddles two masks; the last tile of a call may be short (rows is anything up to count * rep).
// The rows of a tile are one flat index space e = r N + k, so lanes are not idled row by row at small N (a tile is
// 8 N elements: all 256 lanes store from N = 32 up, one wave of the four at N = 8); within a row the
// stores are ascending k, lane-contiguous 8-byte words (rows are N + 1 long: only 8-byte aligned), and the LDS read
// of lane k is word (k + i + 1) mod N: ascending consecutive words, no bank conflict.  N is a power of two: the
// row / column split is a shift and a mask, the wrap a mask, the sign a compare.  The divisions (bin of the tile,
// list entry of each of its rows) run once per workgroup; the rows' degrees wait in LDS behind the polynomial.
#include <hip/hip_runtime.h>

#include "pbs_kernels.h"

namespace tfhe {
namespace {

constexpr int EX_THREADS = 256;
constexpr int EX_ROWS = 8;       // rows per workgroup; divides N * rep for every N >= 8
constexpr int EX_MIN_N = 8;
constexpr int EX_MAX_N = 4096;   // 32 KB of LDS for the polynomial, 64 bytes more for the rows' entries

// grid: ceil(rows / EX_ROWS) workgroups; dynamic LDS: N words + EX_ROWS words
__global__ __launch_bounds__(EX_THREADS) void expand_compact_kernel(const u64* __restrict__ list, unsigned bins,
                                                                    int logN, unsigned rep, unsigned rows,
                                                                    u64* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) u64 poly[];
  const int tid = threadIdx.x;
  const int N = 1 << logN;
  u64* entry = poly + N;  // list entry of each row of the tile
  const unsigned r0 = blockIdx.x * EX_ROWS;                  // < rows
  const unsigned tile_rows = min((unsigned)EX_ROWS, rows - r0);
  const unsigned q0 = r0 / rep, g = q0 >> logN;              // the tile's bin: q0 < count, so g < bins
  const u64* mask = list + ((size_t)g << logN);
  const u64* bodies = list + ((size_t)bins << logN);
  for (int j = tid; j < N; j += EX_THREADS) poly[j] = mask[j];
  if (tid < (int)tile_rows) entry[tid] = (r0 + tid) / rep;
  __syncthreads();
  const size_t big = (size_t)N + 1;
  u64* row0 = out + (size_t)r0 * big;
  for (unsigned e = tid; e < (tile_rows << logN); e += EX_THREADS) {
    const unsigned r = e >> logN;
    const int k = (int)(e & (unsigned)(N - 1));
    const int idx = k + (int)((unsigned)entry[r] & (unsigned)(N - 1)) + 1;  // 1 .. 2N - 1
    const u64 v = poly[idx & (N - 1)];
    row0[r * big + k] = idx < N ? 0 - v : v;
  }
  if (tid < (int)tile_rows) row0[tid * big + N] = bodies[entry[tid]];
}

}  // namespace

hipError_t launch_expand_compact(const u64* list, size_t count, int lwe_dim, int rep, size_t rows, u64* out,
                                 hipStream_t s) {
  if (lwe_dim < EX_MIN_N || lwe_dim > EX_MAX_N || (lwe_dim & (lwe_dim - 1)) || rep < 1 || count > 0x7FFFFFFF ||
      rows > 0x7FFFFFFF || rows > count * (size_t)rep)
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  if (!list || !out) return hipErrorInvalidValue;
  int logN = 0;
  while ((1 << logN) < lwe_dim) logN++;
  const size_t bins = (count + lwe_dim - 1) / lwe_dim, wgs = (rows + EX_ROWS - 1) / EX_ROWS;
  if (wgs > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(expand_compact_kernel, dim3((unsigned)wgs), dim3(EX_THREADS),
                     ((size_t)lwe_dim + EX_ROWS) * sizeof(u64), s, list, (unsigned)bins, logN, (unsigned)rep,
                     (unsigned)rows, out);
  return hipGetLastError();
}

}  // namespace tfhe
