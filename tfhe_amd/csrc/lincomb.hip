// lincomb.hip — sparse linear combinations of LWE rows, all arithmetic wrapping mod 2^64: the linear part of a
// radix circuit level (tfhe-rs lwe_ciphertext_add_assign / lwe_ciphertext_cleartext_mul_assign /
// lwe_ciphertext_plaintext_add_assign applied blockwise) as ONE map from already-bootstrapped rows to the level's
// PBS inputs.
//
//   out[r][j] = sum over t in row_start[r] .. row_start[r + 1] - 1 of terms[t].coef * terms[t].src[j]   (j < dim)
//   out[r][dim - 1] += bias[r]
//
// terms[t].src is the device address of a source row, resolved and bounds-checked on the host (api.cpp
// lincomb_stage): the kernel never forms an address from an index.  A row without terms is a trivial ciphertext
// (zero mask, body bias[r]).  Sources may repeat within a row and across rows; the output overlaps no source.
//
// Grid: one workgroup of 256 lanes per output row (grid-stride beyond LC_MAX_GRID rows).  A lane owns words
// tid + 256 u of a 1024-word piece, u < 4, and walks the row's terms once per piece: the term's address and
// coefficient are wave-uniform, and its four 8-byte loads are independent, so four (eight with the compiler's
// unrolling of the term loop) are in flight per lane.  Loads and stores are 8 bytes wide and lane-contiguous:
// rows of an odd dim (2049, 919, 631) are only 8-byte aligned.  Memory-bound: dim * 8 * (terms + 1) bytes a row.
#include <hip/hip_runtime.h>

#include "pbs_kernels.h"

namespace tfhe {
namespace {

constexpr int LC_THREADS = 256;
constexpr int LC_UNROLL = 4;
constexpr unsigned LC_MAX_GRID = 1u << 20;

__global__ __launch_bounds__(LC_THREADS) void lincomb_kernel(const lin_term* __restrict__ terms,
                                                             const u32* __restrict__ row_start,
                                                             const u64* __restrict__ bias, u32 rows, u32 dim,
                                                             u64* __restrict__ out) {
  const u32 tid = threadIdx.x;
  for (size_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const u32 t0 = row_start[r], t1 = row_start[r + 1];
    const u64 b = bias ? bias[r] : 0;
    u64* o = out + r * dim;
    for (u32 j0 = 0; j0 < dim; j0 += LC_THREADS * LC_UNROLL) {
      u64 acc[LC_UNROLL];
#pragma unroll
      for (int u = 0; u < LC_UNROLL; u++) acc[u] = 0;
      for (u32 t = t0; t < t1; t++) {
        const u64* __restrict__ src = terms[t].src;
        const u64 c = terms[t].coef;
#pragma unroll
        for (int u = 0; u < LC_UNROLL; u++) {
          const u32 j = j0 + tid + u * LC_THREADS;
          if (j < dim) acc[u] += c * src[j];
        }
      }
#pragma unroll
      for (int u = 0; u < LC_UNROLL; u++) {
        const u32 j = j0 + tid + u * LC_THREADS;
        if (j < dim) o[j] = acc[u] + (j == dim - 1 ? b : 0);
      }
    }
  }
}

}  // namespace

hipError_t launch_lincomb(const lin_term* terms, const u32* row_start, const u64* bias, size_t rows, u32 dim, u64* out,
                          hipStream_t s) {
  if (rows == 0) return hipSuccess;
  if (!terms || !row_start || !out || dim == 0 || rows > 0x7FFFFFFF) return hipErrorInvalidValue;
  const unsigned grid = rows < LC_MAX_GRID ? (unsigned)rows : LC_MAX_GRID;
  hipLaunchKernelGGL(lincomb_kernel, dim3(grid), dim3(LC_THREADS), 0, s, terms, row_start, bias, (u32)rows, dim, out);
  return hipGetLastError();
}

}  // namespace tfhe
