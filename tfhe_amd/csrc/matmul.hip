// matmul.hip — encrypted matrix x clear matrix: the GLWE x clear-matrix dot product with sample extraction, and the
// expansion of the seeded, modulus-switched input GLWEs (include/tfhe_hip.h, tfhe_hip_matmul_*).
//
// Rule, restated from the reference (ml/extensions/rust/src): the driver lib_python.rs:243-337 multiplies every input
// GLWE by the reversed weight column as a negacyclic polynomial (computations.rs:80-132, ml.rs:66-90), adds the
// products of a row's K-blocks and sample-extracts coefficient N-1 (ml.rs:95-121).  In closed form, for row r and
// column c, with w_kb[t] = W[kb N + t][c] and GLWE (a, b) = glwe_{r,kb} (k = 1, arithmetic mod 2^64):
//   mask[i] = sum_kb sum_t w_kb[t] * a'[t - i],   a'[d] = a[d] (d >= 0), -a[N + d] (d < 0)
//   body    = sum_kb sum_t w_kb[t] * b[t]
// Expansion (compression.rs:110-128, ml.rs:191-205): mask words 0 .. N-1 of the GLWE's seed (csprng.hip), body values
// unpacked LSB first and moved to the top of the word.  Seeded paths are PARITY UNPINNED at the byte level.
//
// Per encrypted row the masks are an integer GEMM  Mask_r[N x C] = sum_kb T(a_{r,kb}) x W_kb  whose left operand is the
// negacyclic Toeplitz matrix of one polynomial; it is never written out: for an i-tile and a chunk of 64 t the
// operand is a window of 127 consecutive values of a'.
//
// Kernels:
//   matmul_dot_kernel   one 256-thread workgroup per (64 i, 64 c, row r), 4 x 4 outputs per thread, t in chunks of 64:
//                       the window (1 KB) and the weight chunk (16 KB, u32) go through LDS; a thread's four i form a
//                       sliding window, so a t step reads one new u64 of a' and one 128-bit group of four weights for
//                       16 multiply-adds.  The weights are stored offset, w + 2^31, so the multiply-add is
//                       u32 x u64 as in pks.hip; here the two halves of the u64 go to accumulators of their own, two
//                       v_mad_u64_u32 in place per multiply-add (64 accumulator registers; the joint form costs the
//                       same two plus two moves between register pairs, 10.5 against 13.9 T multiply-adds/s
//                       measured).  The offset's share, 2^31 * sum_t a'[t - i], is taken off in the epilogue from a
//                       running sum of the window (one add per t step; the sums of the other three i differ from it
//                       by the values that enter and leave the window at a chunk's ends).  The K-blocks are
//                       accumulated in registers; i runs fastest across lanes in the store.
//   matmul_body_kernel  the bodies: 64 columns x 4 slices of t per workgroup, reduced through LDS
//   matmul_unpack_kernel one thread per body coefficient of the input GLWEs
#include <hip/hip_runtime.h>

#include "pbs_kernels.h"

namespace tfhe {
namespace {

constexpr int MM_TILE = 64, MM_THREADS = 256;

__global__ void __launch_bounds__(MM_THREADS) matmul_dot_kernel(const u64* __restrict__ glwes, const u32* __restrict__ W,
                                                               int N, int Kb, int Cpad, int C, size_t col_stride,
                                                               u64* __restrict__ out) {
  // win[1 + j] = a'[t0 - i0 - 63 + j], j < 127 (one slot in front keeps a thread's reads 16-byte aligned)
  __shared__ __attribute__((aligned(16))) u64 win[2 * MM_TILE];
  __shared__ __attribute__((aligned(16))) u32 Ws[MM_TILE][MM_TILE];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, ib = tx * 4;
  const int i0 = blockIdx.x * MM_TILE, c0 = blockIdx.y * MM_TILE;
  const size_t r = blockIdx.z;
  // sum w * x = lo + (hi << 32): one accumulator per half of x, each a v_mad_u64_u32 in place (of hi only the low word counts)
  u64 lo[4][4], hi[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) lo[i][j] = hi[i][j] = 0;
  // sum_t a'[t - (i0 + ib + ii)] = s0 + s[ii] (s[0] = 0)
  u64 s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  const u64* wp = win + (MM_TILE - ib);  // wp[tt - ii] = a'[t0 + tt - (i0 + ib + ii)]
  for (int kb = 0; kb < Kb; kb++) {
    const u64* a = glwes + (r * Kb + kb) * 2 * (size_t)N;
    const u32* Wk = W + (size_t)kb * N * Cpad + c0;
    for (int t0 = 0; t0 < N; t0 += MM_TILE) {
      if (tid < 2 * MM_TILE - 1) {
        const int d = t0 - i0 - (MM_TILE - 1) + tid;  // -(N - 1) .. N - 1
        win[1 + tid] = d >= 0 ? a[d] : 0 - a[N + d];
      }
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int e = tid + q * MM_THREADS, row = e >> 4, c4 = (e & 15) * 4;
        *(uint4*)&Ws[row][c4] = *(const uint4*)(Wk + (size_t)(t0 + row) * Cpad + c4);
      }
      __syncthreads();
      u64 x1 = wp[-1], x2 = wp[-2], x3 = wp[-3];
      s1 += x1;
      s2 += x1 + x2;
      s3 += x1 + x2 + x3;
#pragma unroll 8
      for (int tt = 0; tt < MM_TILE; tt++) {
        const u64 x0 = wp[tt];
        const uint4 w4 = *(const uint4*)&Ws[tt][ty * 4];
        const u32 w[4] = {w4.x, w4.y, w4.z, w4.w};
        s0 += x0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          lo[0][j] += (u64)w[j] * (u32)x0;
          lo[1][j] += (u64)w[j] * (u32)x1;
          lo[2][j] += (u64)w[j] * (u32)x2;
          lo[3][j] += (u64)w[j] * (u32)x3;
          hi[0][j] += (u64)w[j] * (u32)(x0 >> 32);
          hi[1][j] += (u64)w[j] * (u32)(x1 >> 32);
          hi[2][j] += (u64)w[j] * (u32)(x2 >> 32);
          hi[3][j] += (u64)w[j] * (u32)(x3 >> 32);
        }
        x3 = x2;
        x2 = x1;
        x1 = x0;
      }
      // x1, x2, x3: the last three values of the ii = 0 sequence, which the shifted ones do not reach
      s1 -= x1;
      s2 -= x1 + x2;
      s3 -= x1 + x2 + x3;
      __syncthreads();
    }
  }
  const u64 S[4] = {s0, s0 + s1, s0 + s2, s0 + s3};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = c0 + ty * 4 + j;
    if (c >= C) continue;
    u64* o = out + (r * col_stride + c) * (size_t)(N + 1) + i0 + ib;
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = lo[i][j] + (hi[i][j] << 32) - (S[i] << 31);
  }
}

__global__ void __launch_bounds__(MM_THREADS) matmul_body_kernel(const u64* __restrict__ glwes, const u32* __restrict__ W,
                                                                int N, int Kb, int Cpad, int C, size_t col_stride,
                                                                u64* __restrict__ out) {
  __shared__ u64 red[4][MM_TILE];
  const int tid = threadIdx.x, cl = tid & 63, sl = tid >> 6;
  const int c = blockIdx.x * MM_TILE + cl;  // < Cpad
  const size_t r = blockIdx.y;
  u64 acc = 0;
  for (int kb = 0; kb < Kb; kb++) {
    const u64* b = glwes + ((r * Kb + kb) * 2 + 1) * (size_t)N;
    const u32* Wk = W + (size_t)kb * N * Cpad + c;
#pragma unroll 8
    for (int t = sl; t < N; t += 4) {
      const long long w = (int)(Wk[(size_t)t * Cpad] ^ 0x80000000u);
      acc += (u64)w * b[t];
    }
  }
  red[sl][cl] = acc;
  __syncthreads();
  if (sl == 0 && c < C)
    out[(r * col_stride + c) * (size_t)(N + 1) + N] = red[0][cl] + red[1][cl] + red[2][cl] + red[3][cl];
}

__global__ void matmul_unpack_kernel(const u64* __restrict__ packed, size_t G, int N, int w, size_t body_words,
                                     u64* __restrict__ glwes) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G * (size_t)N) return;
  const size_t g = idx / N, t = idx % N;
  const u64* p = packed + g * body_words;
  const size_t bit = t * (size_t)w, word = bit >> 6;
  const int off = (int)(bit & 63);
  u64 v = p[word] >> off;
  if (off + w > 64) v |= p[word + 1] << (64 - off);
  glwes[(g * 2 + 1) * (size_t)N + t] = v << (64 - w);
}

}  // namespace

hipError_t launch_matmul_expand(const u64* seeds, const u64* packed, size_t G, int N, int w, u64* glwes, hipStream_t s) {
  if (G == 0) return hipSuccess;
  if (G * (size_t)N > 0x7FFFFFFFull * 256) return hipErrorInvalidValue;
  hipError_t e = launch_csprng_rows(seeds, G, 0, (u32)N, 2 * (size_t)N, false, glwes, s);
  if (e != hipSuccess) return e;
  const size_t el = G * (size_t)N, body_words = ((size_t)N * w + 63) / 64;
  matmul_unpack_kernel<<<(unsigned)((el + 255) / 256), 256, 0, s>>>(packed, G, N, w, body_words, glwes);
  return hipGetLastError();
}

hipError_t launch_matmul_dot(const u64* glwes, const u32* W, size_t R, int N, int Kb, int Cpad, int C, size_t col_stride,
                             u64* out, hipStream_t s) {
  if (R == 0) return hipSuccess;
  if (N % MM_TILE || Cpad % MM_TILE || C > Cpad || Cpad / MM_TILE > 65535 || col_stride < (size_t)C)
    return hipErrorInvalidValue;
  for (size_t r0 = 0; r0 < R; r0 += 65535) {
    const unsigned rows = (unsigned)(R - r0 < 65535 ? R - r0 : 65535);
    const u64* g = glwes + r0 * Kb * 2 * (size_t)N;
    u64* o = out + r0 * col_stride * (size_t)(N + 1);
    matmul_dot_kernel<<<dim3(N / MM_TILE, Cpad / MM_TILE, rows), MM_THREADS, 0, s>>>(g, W, N, Kb, Cpad, C, col_stride, o);
    matmul_body_kernel<<<dim3(Cpad / MM_TILE, rows), MM_THREADS, 0, s>>>(g, W, N, Kb, Cpad, C, col_stride, o);
  }
  return hipGetLastError();
}

}  // namespace tfhe
