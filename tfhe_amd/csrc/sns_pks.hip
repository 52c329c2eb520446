// sns_pks.hip — LWE -> GLWE packing keyswitch over the 2^128 torus: the compression of squashed ciphertexts
// (include/tfhe_hip.h tfhe_hip_sns_pks_*; the rule is stated there, the host form is client.cpp sns_pks_pack_host).
//
// pks.hip's shape on 128-bit words.  For a group of up to lwe_per_glwe LWEs packed into one GLWE:
//   out = sum_d X^d * ((0 | b_d) - T_d),   T_d = sum_{j,l} digit_{d,j,l} * PKSK[j][l]   (mod 2^128)
// The T_d of all LWEs form one integer GEMM  T[M][(k+1)N] = D[M][in_dim*L] x PKSK[in_dim*L][(k+1)N] (128 x 4096 x
// 7168 per GLWE at the fhEVM preset), followed by a negacyclic shift-and-sum that reads each T element once.
// A digit is a balanced integer of up to 63 bits; it is stored offset by B/2 to [0, 2^base_log] so that a MAC is
// u64 x u128 mod 2^128: the full 64 x 64 -> 128 product with the low key word plus the low half of the product
// with the high key word (v_mad_u64_u32 chains; no matrix-core form: the operands are 64 and 128 bits wide).  The
// offset's contribution, (B/2) * column sum of the key, is precomputed per key and subtracted in the GEMM epilogue.
//
// Kernels:
//   sns_pks_digits_kernel    one thread per mask word: SignedDecomposer digits on a u128 state
//   sns_pks_gemm_kernel      64 x 64 output tile per 256-thread workgroup, 4 x 4 u128 accumulators per thread
//                            (64 VGPRs), K staged through LDS in steps of 16 (24.4 KB)
//   sns_pks_shift_sum_kernel one thread per output coefficient: sum_d +-T_d[(t - d) mod N] + bodies
//   sns_pks_corr_kernel      (B/2) * column sums of the key, once per key load
#include <hip/hip_runtime.h>

#include "pbs_kernels.h"

namespace tfhe {
namespace {

typedef unsigned __int128 u128;

constexpr int SG_BM = 64, SG_BN = 64, SG_BK = 16, SG_THREADS = 256;
constexpr int SG_APAD = 2;  // u64 of row padding: the transposing stores of the digit tile spread over the banks

__global__ void sns_pks_digits_kernel(const u64* __restrict__ lwes, size_t count, int in_dim, int base_log, int L,
                                      u64* __restrict__ A) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= count * (size_t)in_dim) return;
  const size_t m = idx / in_dim, j = idx % in_dim;
  const u64* w = lwes + (m * ((size_t)in_dim + 1) + j) * 2;
  const u128 x = ((u128)w[1] << 64) | w[0];
  const int prec = base_log * L;
  u128 state = ((x >> (128 - prec - 1)) + 1) >> 1;
  state &= ((u128)1 << prec) - 1;
  const u128 low = ((u128)1 << base_log) - 1;
  const u64 half = 1ull << (base_log - 1);
  u64* out = A + m * (size_t)in_dim * L + j * (size_t)L;
  for (int l = L - 1; l >= 0; l--) {
    const u128 res = state & low;
    state >>= base_log;
    const u128 carry = ((((res - 1) | state) & res) >> (base_log - 1)) & 1;
    state += carry;
    out[l] = (u64)res - (u64)(carry << base_log) + half;  // digit + B/2, in [0, 2^base_log]
  }
}

// P: the key, [K][c][lo, hi][N]; corr: [Nc] u128; T: [M][Nc] u128
__global__ void __launch_bounds__(SG_THREADS)
    sns_pks_gemm_kernel(const u64* __restrict__ A, const u64* __restrict__ P, const u128* __restrict__ corr,
                        u128* __restrict__ T, int M, int K, int Nc, int logN) {
  __shared__ u64 As[SG_BK][SG_BM + SG_APAD];
  __shared__ u64 Bl[SG_BK][SG_BN];
  __shared__ u64 Bh[SG_BK][SG_BN];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int n0 = blockIdx.x * SG_BN, m0 = blockIdx.y * SG_BM;
  const int N = 1 << logN;
  u128 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = 0;
  for (int k0 = 0; k0 < K; k0 += SG_BK) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int e = tid + r * SG_THREADS;  // 1024 elements of each tile
      const int am = e / SG_BK, ak = e % SG_BK;
      As[ak][am] = (m0 + am < M) ? A[(size_t)(m0 + am) * K + k0 + ak] : 0ull;
      const int bk = e / SG_BN, bn = e % SG_BN, n = n0 + bn;
      // column n = coefficient n % N of polynomial n / N (a tile spans two polynomials at N = 32)
      const u64* src = P + ((size_t)(k0 + bk) * Nc + (size_t)(n >> logN) * N) * 2 + (n & (N - 1));
      Bl[bk][bn] = src[0];
      Bh[bk][bn] = src[N];
    }
    __syncthreads();
#pragma unroll 2
    for (int kk = 0; kk < SG_BK; kk++) {
      u64 a[4], bl[4], bh[4];
#pragma unroll
      for (int i = 0; i < 4; i++) a[i] = As[kk][ty * 4 + i];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        bl[j] = Bl[kk][tx * 4 + j];
        bh[j] = Bh[kk][tx * 4 + j];
      }
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] += (u128)a[i] * bl[j] + ((u128)(a[i] * bh[j]) << 64);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int m = m0 + ty * 4 + i;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int n = n0 + tx * 4 + j;
      T[(size_t)m * Nc + n] = acc[i][j] - corr[n];
    }
  }
}

__global__ void sns_pks_shift_sum_kernel(const u128* __restrict__ T, const u64* __restrict__ lwes, size_t count,
                                         int in_dim, int k, int N, int lpg, size_t groups, u64* __restrict__ out) {
  const int Nc = (k + 1) * N;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= groups * (size_t)Nc) return;
  const size_t g = idx / Nc;
  const int ct = (int)(idx % Nc), c = ct / N, t = ct % N;
  const size_t first = g * (size_t)lpg;
  const int cnt = (int)min((size_t)lpg, count - first);
  const u128* Tg = T + first * (size_t)Nc + (size_t)c * N;
  u128 acc = 0;
  for (int d = 0; d <= t && d < cnt; d++) acc -= Tg[(size_t)d * Nc + (t - d)];
  for (int d = t + 1; d < cnt; d++) acc += Tg[(size_t)d * Nc + (t - d + N)];
  if (c == k && t < cnt) {
    const u64* b = lwes + ((first + t) * ((size_t)in_dim + 1) + in_dim) * 2;
    acc += ((u128)b[1] << 64) | b[0];
  }
  u64* dst = out + (g * (size_t)Nc + (size_t)c * N) * 2;
  dst[t] = (u64)acc;
  dst[N + t] = (u64)(acc >> 64);
}

// column sums of the key times B/2 (the digit offset's contribution)
__global__ void sns_pks_corr_kernel(const u64* __restrict__ P, int K, int Nc, int logN, u64 half,
                                    u128* __restrict__ corr) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= Nc) return;
  const int N = 1 << logN;
  const u64* col = P + (size_t)(n >> logN) * N * 2 + (n & (N - 1));
  u128 s = 0;
  for (int r = 0; r < K; r++) {
    const u64* src = col + (size_t)r * Nc * 2;
    s += ((u128)src[N] << 64) | src[0];
  }
  corr[n] = s * half;
}

int log2_of(int N) {
  int l = 0;
  while ((1 << l) < N) l++;
  return l;
}

}  // namespace

hipError_t launch_sns_pks_corr(const u64* pksk, int K, int Nc, int N, int base_log, u64* corr, hipStream_t s) {
  sns_pks_corr_kernel<<<(Nc + 255) / 256, 256, 0, s>>>(pksk, K, Nc, log2_of(N), 1ull << (base_log - 1), (u128*)corr);
  return hipGetLastError();
}

// A workspace: count x in_dim*L u64; T workspace: count x Nc x 16 bytes; corr: Nc x 16 bytes
hipError_t launch_sns_pks_pack(const u64* lwes, size_t count, int in_dim, int base_log, int L, int k, int N, int lpg,
                               const u64* pksk, const u64* corr, u64* A, u64* T, u64* out, hipStream_t s) {
  if (count == 0) return hipSuccess;
  const int K = in_dim * L, Nc = (k + 1) * N;
  const size_t el = count * (size_t)in_dim, groups = (count + lpg - 1) / lpg, outs = groups * (size_t)Nc;
  const size_t tiles_m = (count + SG_BM - 1) / SG_BM;
  if ((el + 255) / 256 > 0x7FFFFFFFull || (outs + 255) / 256 > 0x7FFFFFFFull || tiles_m > 65535)
    return hipErrorInvalidValue;
  sns_pks_digits_kernel<<<(unsigned)((el + 255) / 256), 256, 0, s>>>(lwes, count, in_dim, base_log, L, A);
  dim3 grid(Nc / SG_BN, (unsigned)tiles_m);
  sns_pks_gemm_kernel<<<grid, SG_THREADS, 0, s>>>(A, pksk, (const u128*)corr, (u128*)T, (int)count, K, Nc, log2_of(N));
  sns_pks_shift_sum_kernel<<<(unsigned)((outs + 255) / 256), 256, 0, s>>>((const u128*)T, lwes, count, in_dim, k, N, lpg,
                                                                         groups, out);
  return hipGetLastError();
}

}  // namespace tfhe
