// sample_extract_many.hip — sample extraction at several degrees of one accumulator (many-LUT PBS).
//
// A many-LUT accumulator holds n_fn tables side by side; after ONE blind rotation output f is the
// sample at degree d = f * stride (tfhe-rs apply_many_lookup_table).  For a mask polynomial A_c:
//   a'[cN + j] =  A_c[d - j]       (j <= d)
//   a'[cN + j] = -A_c[N + d - j]   (j >  d)        b' = Body[d]
// with the negation in the accumulator's ring: Z_p on the NTT engines (then converted to 2^64 by
// gl_to_torus, as the degree-0 epilogues do), Z_2^64 on the FFT64 engines.
//
// One workgroup per (ciphertext, mask polynomial): the polynomial is read from HBM once (16 B per lane,
// lane-contiguous) into LDS, and every one of the n_fn output rows is written from that copy.  A row is
// written in ascending j, lane-contiguous 8-byte stores (rows are kN + 1 words long, so only 8-byte
// aligned); the LDS read of lane j is word (d - j) mod N: descending consecutive 8-byte words, 32 lanes =
// one 256-byte bank row, no conflict.  N is a power of two, so the wrap is a mask and a sign test; nothing
// divides.  The body contributes n_fn words per ciphertext, read directly by the c = 0 workgroup.
#include <hip/hip_runtime.h>

#include "gl64.h"
#include "pbs_kernels.h"

namespace tfhe {
namespace {

constexpr int SEM_THREADS = 256;
constexpr int SEM_MAX_N = 2048;

template <bool ZP>
__device__ __forceinline__ u64 sem_out(u64 v, bool neg) {
  if (ZP) return gl_to_torus(neg ? gl_neg(v) : v);
  return neg ? 0 - v : v;
}

// grid (B, k); N a power of two, 2 <= N <= SEM_MAX_N; (n_fn - 1) * stride < N (checked by the launcher)
template <bool ZP>
__global__ __launch_bounds__(SEM_THREADS) void sample_extract_many_kernel(const u64* __restrict__ acc, int k, int N,
                                                                          int n_fn, int stride,
                                                                          u64* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) u64 poly[SEM_MAX_N];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const int c = blockIdx.y;
  const u64* A = acc + (b * (size_t)(k + 1) + c) * N;
  for (int i = 2 * tid; i < N; i += 2 * SEM_THREADS) {
    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(A + i);
    *reinterpret_cast<ulonglong2*>(&poly[i]) = v;
  }
  __syncthreads();
  const size_t big = (size_t)k * N + 1;
  u64* row = out + b * n_fn * big + (size_t)c * N;
  const u64* body = acc + (b * (size_t)(k + 1) + k) * N;
  for (int f = 0, d = 0; f < n_fn; f++, d += stride, row += big) {
    for (int j = tid; j < N; j += SEM_THREADS) {
      const int idx = d - j;
      row[j] = sem_out<ZP>(poly[idx & (N - 1)], idx < 0);
    }
    if (c == 0 && tid == 0) row[(size_t)k * N] = sem_out<ZP>(body[d], false);
  }
}

}  // namespace

hipError_t launch_sample_extract_many(const u64* acc, size_t B, int k, int N, bool zp, int n_fn, int stride, u64* out,
                                      hipStream_t s) {
  if (B == 0) return hipSuccess;
  if (k < 1 || k > 65535 || N < 2 || N > SEM_MAX_N || (N & (N - 1)) || n_fn < 1 || stride < 1 ||
      (long long)(n_fn - 1) * stride >= N || B > 0x7FFFFFFF || ((uintptr_t)acc & 15))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)B, (unsigned)k);
  if (zp)
    hipLaunchKernelGGL(sample_extract_many_kernel<true>, grid, dim3(SEM_THREADS), 0, s, acc, k, N, n_fn, stride, out);
  else
    hipLaunchKernelGGL(sample_extract_many_kernel<false>, grid, dim3(SEM_THREADS), 0, s, acc, k, N, n_fn, stride, out);
  return hipGetLastError();
}

}  // namespace tfhe
