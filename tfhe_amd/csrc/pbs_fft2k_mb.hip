// pbs_fft2k_mb.hip — multi-bit blind rotation (tfhe-rs LweMultiBitBootstrapKey) at the shape of pbs_fft2k.hip: FFT64,
// k = 1, N = 2048, PBS gadget 2^23 x 1, grouping factor g in {2, 3, 4} (include/tfhe_hip.h has the semantics).
//
// The key holds, per group q of g mask elements, the 2^g - 1 GGSWs of the indicators [group bits == sigma], converted
// like a classic key (convert_bsk_f2k: spectra negated, x 2^-42), GGSW (q, sigma) at index q (2^g - 1) + sigma - 1.
// One kernel shape for every batch size: workgroup = 8 waves = 2 ciphertexts (the latency shape of pbs_fft2k.hip);
// waves w < 4 are the transform waves (p, c) = (w >> 1, w & 1) holding component c of ciphertext p in registers,
// every wave owns MAC slots 2 w, 2 w + 1 of both ciphertexts.  LDS: the 16 KB pass-A table + 4 areas x 16 KB + the
// 64 KB root table = 144 KB, one workgroup per CU (its 256 VGPRs per lane allow no second one anyway).
// Per group q:
//   every wave: t_sigma = ms4096(sum_{i in sigma} a_{gq+i} mod 2^64) of both ciphertexts, wave-uniform (sum first,
//     then switch); the key words of sigma = 1 requested (the MAC-only waves: of the first NB sigmas)
//   transform waves: NEGATED 23-bit digits of acc_c itself from registers (no rotation, no LDS image), the forward
//     transform, the spectrum D_c stored to the area [slot][lane]
//   barrier
//   bundle-MAC, all waves, per ciphertext and owned point p:
//     O_j[p] = sum_sigma (w_sigma[p] - 1) (D_0[p] K_{sigma,0,j}[p] + D_1[p] K_{sigma,1,j}[p])
//     in this fixed order: sigma ascending from O = (0, 0); P = the classic chain (pbs_fft2k.hip: fma from (0, 0),
//     c = 0 first, re: +d.x k.x, -d.y k.y, im: +d.x k.y, +d.y k.x); f = (w.x - 1, w.y);
//     O.re = fma(f.x, P.re, O.re), O.re = fma(-f.y, P.im, O.re), O.im = fma(f.x, P.im, O.im), O.im = fma(f.y, P.re, O.im).
//     The key words travel through a ring of NB register buffers (NB = 3 at g = 2, else 2): those of sigma + NB are
//     requested when the MAC of sigma has consumed its buffer, so the loads of sigma + 1 are in flight during the MAC
//     of sigma; they are shared by both ciphertexts.  D is re-read from the areas per sigma.  O_j over D_j.
//   barrier
//   transform waves: the inverse transform, acc_c += rint mod 2^64 (torus_acc_add_wide_y)
// Sequential depth n / g group steps of two transforms each, against n CMUXes.
//
// The twiddle w_sigma[p] = X^{t_sigma} at point p = zeta^{(t_sigma e[p]) mod 4096}, zeta = e^{2 pi i / 4096}: slot m1 of
// lane L holds Z[k], k = (L & 3) + 4 (L >> 4) + 16 ((L >> 2) & 3) + 64 m1 (fft1k.h), and Z[k] = sum_n (a_n + i a_{n+1024})
// zeta^n zeta^{4 n k} is the polynomial at x = zeta^{1 + 4 k} (x^1024 = i), so e[p] = (1 + 4 k) mod 4096.  Both the
// exponents and the 4096 roots are host tables (make_tables_f2k_mb; the roots by the generator of every other table,
// fft_twiddle), so the result is a function of the inputs alone.  The whole 64 KB root table is copied into LDS at
// the kernel start.  Read through L2 / the vector L1 instead (the first form of this kernel) the gathers bound the
// kernel: a wave's gather touches up to 64 cache lines, 2 (2^g - 1) of them per slot and group, and a group step took
// 38 us at g = 4 against 17 us now (same box).  A quarter table would save 48 KB of LDS that nothing else
// wants (the registers allow one workgroup per CU) for an octant fix-up of 6-8 VALU per gather.
// root[0] = (1, 0) exactly (checked on the host), so w - 1 = (0, 0) at t_sigma = 0: such a term adds (+-0), and a group
// with all-zero masks is an exact identity.
//
// Magnitude: |digit| <= 2^22, a key coefficient |.| <= 2^63, N = 2048 terms, 2 rows: the classic |x| < 2^97 worst case;
// the bundle sums up to 2 (2^g - 1) <= 30 key-sized terms (|w - 1| <= 2), so |x| < 2^102, inside torus_acc_add_wide_y's
// |x| < 2^115.
#include "fft1k.h"
#include "pbs_kernels.h"

namespace tfhe {
namespace fft1k_mb {
using namespace fft1k;

constexpr int N2 = 2048;
constexpr int CTS = 2, NW = 8, SPW = 16 / NW;
// tables (8-byte words): root [4096] complex | e [1024] u32
constexpr int K_ROOT_W = 0, K_EXP_W = 2 * 4096;
[[maybe_unused]] constexpr int K_MB_WORDS = K_EXP_W + M1 / 2;

__device__ __forceinline__ int ms4096(u64 x) { return (int)((((x >> 51) + 1) >> 1) & 4095u); }

struct MbShared {
  double2 ta[M1];  // pass A table (K_TA)
  double2 area[2 * CTS][AREA_C64];
  double2 root[4096];  // zeta^t: the bundle-MAC's gathers
};

// NEGATED SignedDecomposer digits (2^23 x 1) of v itself: xr[e] <- coefficient L + 64 e, xi[e] <- + 1024.  The digit
// comes from the high word h alone, -dig23(h) = (int)(255 - h) >> 9 (pbs_fft2k.hip rotate_digits)
__device__ __forceinline__ void acc_digits(const u64 (&v)[32], double (&xr)[16], double (&xi)[16]) {
#pragma unroll
  for (int e = 0; e < 32; e++) {
    const double d = (double)((int)(255u - (u32)(v[e] >> 32)) >> 9);
    if (e < 16) xr[e] = d;
    else xi[e - 16] = d;
  }
}

template <int G, bool WRITE_ACC, bool WRITE_BIG>
__global__ __launch_bounds__(64 * NW, 1) void blind_rotate_fft2k_mb_kernel(
    const u64* __restrict__ lwe_in, int n, size_t B, const u64* __restrict__ luts, const u32* __restrict__ lut_index,
    int n_lut, const double2* __restrict__ bsk, const double2* __restrict__ tg, const double2* __restrict__ root,
    const u32* __restrict__ expo, u64* __restrict__ out_big, u64* __restrict__ out_acc) {
  constexpr int NS = (1 << G) - 1;  // stored GGSWs per group
  // key buffers in flight per wave, 32 VGPRs each: three cover a whole group at g = 2 (12 VGPRs spilled); at g = 3
  // and 4 a third buffer spills 40 VGPRs (and was slower than two when tried, then with the gathers through L1)
  constexpr int NB = G == 2 ? 3 : 2;
  __shared__ __attribute__((aligned(16))) MbShared sh;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const bool tw_wave = wave_s < 2 * CTS;
  const int c = wave & 1, p = tw_wave ? wave >> 1 : 0;
  const size_t b_raw = (size_t)blockIdx.x * CTS + p;
  const bool live = tw_wave && b_raw < B;
  const size_t b = b_raw < B ? b_raw : B - 1;  // the padding waves run a copy of the last ciphertext, store nothing
  const u64* ct = lwe_in + b * (size_t)(n + 1);
  const u64* ctq[CTS];  // both ciphertexts of the workgroup: every wave needs their t_sigma
#pragma unroll
  for (int q = 0; q < CTS; q++) {
    const size_t bq = (size_t)blockIdx.x * CTS + q;
    ctq[q] = lwe_in + (bq < B ? bq : B - 1) * (size_t)(n + 1);
  }
  double2* area = sh.area[tw_wave ? wave : 0];

  for (int q = threadIdx.x; q < M1; q += blockDim.x) sh.ta[q] = tg[K_TA + q];
  for (int q = threadIdx.x; q < 4096; q += blockDim.x) sh.root[q] = root[q];
  TwB tb;
  tb.load(tg, lane);
  u64 acc[32];
  if (tw_wave) {  // acc_c: A = 0, B = X^{-b~} * lut (as pbs_fft2k.hip)
    int li = lut_index ? (int)lut_index[b] : 0;
    li = (li < 0 || li >= n_lut) ? 0 : li;
    const u64* lut = luts + (size_t)li * N2;
    const int s = (4096 - ms4096(ct[n])) & 4095;
#pragma unroll
    for (int e = 0; e < 32; e++) {
      int d = 64 * e + lane - s;
      bool neg = false;
      if (d < 0) { d += N2; neg = !neg; }
      if (d < 0) { d += N2; neg = !neg; }
      const u64 v = gl_to_torus(lut[d]);
      acc[e] = c ? (neg ? 0 - v : v) : 0;
    }
  }
  __syncthreads();

  const int s0 = SPW * wave_s;  // MAC slots s0 .. s0 + SPW - 1
  u32 ex[SPW];                  // e[p] of the owned points
#pragma unroll
  for (int t = 0; t < SPW; t++) ex[t] = expo[64 * (s0 + t) + lane];
  // kv[t][cc][j] = K_{cc,j}[slot s0 + t][lane] of GGSW i
  auto load_key = [&](int i, double2 (&kv)[SPW][2][2]) {
#pragma unroll
    for (int t = 0; t < SPW; t++)
#pragma unroll
      for (int cc = 0; cc < 2; cc++)
#pragma unroll
        for (int j = 0; j < 2; j++) kv[t][cc][j] = bsk[((size_t)(i * 2 + cc) * 2 + j) * M1 + 64 * (s0 + t) + lane];
  };

  const int groups = n / G;
  for (int grp = 0; grp < groups; grp++) {
    int ts[CTS][NS];  // t_sigma, wave-uniform
#pragma unroll
    for (int q = 0; q < CTS; q++) {
      u64 am[G];
#pragma unroll
      for (int i = 0; i < G; i++) am[i] = ctq[q][G * grp + i];
#pragma unroll
      for (int sg = 1; sg <= NS; sg++) {
        u64 sum = 0;
#pragma unroll
        for (int i = 0; i < G; i++)
          if ((sg >> i) & 1) sum += am[i];
        ts[q][sg - 1] = __builtin_amdgcn_readfirstlane(ms4096(sum));
      }
    }
    // a ring of NB key buffers.  The MAC-only waves request the first NB sigmas here, so their latency hides behind
    // the transform waves' forward transform; a transform wave requests sigma = 1 here and the others once the
    // transform has freed its registers (holding three across it spills 60-80 VGPRs).  Sigma + NB is requested when
    // the MAC of sigma has consumed its buffer, so NB - 1 .. NB requests are in flight during every MAC step
    double2 kv[NB][SPW][2][2];
    load_key(grp * NS, kv[0]);
    if (!tw_wave) {
#pragma unroll
      for (int sg = 1; sg < NB && sg < NS; sg++) load_key(grp * NS + sg, kv[sg]);
    }
    if (tw_wave) {
      double xr[16], xi[16];
      acc_digits(acc, xr, xi);
      fft1k_fwd(xr, xi, area, lane, sh.ta, tb);
#pragma unroll
      for (int s = 0; s < 16; s++) area[64 * s + lane] = make_double2(xr[s], xi[s]);
#pragma unroll
      for (int sg = 1; sg < NB && sg < NS; sg++) load_key(grp * NS + sg, kv[sg]);
    }
    __syncthreads();
    // the spectra D stay in the areas until O overwrites them: they are re-read per sigma, which leaves their
    // registers to the key ring
    double2 o[CTS][SPW][2];
#pragma unroll
    for (int q = 0; q < CTS; q++)
#pragma unroll
      for (int t = 0; t < SPW; t++) o[q][t][0] = o[q][t][1] = make_double2(0.0, 0.0);
#pragma unroll
    for (int sg = 0; sg < NS; sg++) {
#pragma unroll
      for (int q = 0; q < CTS; q++)
#pragma unroll
        for (int t = 0; t < SPW; t++) {
          const double2 w = sh.root[((u32)ts[q][sg] * ex[t]) & 4095u];
          const double fx = w.x - 1.0, fy = w.y;
          const int idx = 64 * (s0 + t) + lane;
          const double2 d0 = sh.area[2 * q][idx], d1 = sh.area[2 * q + 1][idx];
#pragma unroll
          for (int j = 0; j < 2; j++) {
            const double2 k0 = kv[sg % NB][t][0][j], k1 = kv[sg % NB][t][1][j];
            double re = __builtin_fma(d0.x, k0.x, 0.0);
            re = __builtin_fma(-d0.y, k0.y, re);
            double im = __builtin_fma(d0.x, k0.y, 0.0);
            im = __builtin_fma(d0.y, k0.x, im);
            re = __builtin_fma(d1.x, k1.x, re);
            re = __builtin_fma(-d1.y, k1.y, re);
            im = __builtin_fma(d1.x, k1.y, im);
            im = __builtin_fma(d1.y, k1.x, im);
            double2& oo = o[q][t][j];
            oo.x = __builtin_fma(fx, re, oo.x);
            oo.x = __builtin_fma(-fy, im, oo.x);
            oo.y = __builtin_fma(fx, im, oo.y);
            oo.y = __builtin_fma(fy, re, oo.y);
          }
        }
      if (sg + NB < NS) load_key(grp * NS + sg + NB, kv[sg % NB]);
    }
#pragma unroll
    for (int q = 0; q < CTS; q++)
#pragma unroll
      for (int t = 0; t < SPW; t++) {
        const int idx = 64 * (s0 + t) + lane;
        sh.area[2 * q][idx] = o[q][t][0];
        sh.area[2 * q + 1][idx] = o[q][t][1];
      }
    __syncthreads();
    if (tw_wave) {
      double xr[16], xi[16];
#pragma unroll
      for (int s = 0; s < 16; s++) {
        const double2 v = area[64 * s + lane];
        xr[s] = v.x;
        xi[s] = v.y;
      }
      fft1k_inv(xr, xi, area, lane, sh.ta, tb);
      // the keys' spectra carry 2^-32 (pbs_fft2k.hip): y = x * 2^-32 bit for bit
#pragma unroll
      for (int e = 0; e < 16; e++) {
        acc[e] = torus_acc_add_wide_y(acc[e], xr[e]);
        acc[e + 16] = torus_acc_add_wide_y(acc[e + 16], xi[e]);
      }
    }
  }

  if (!live) return;
  if (WRITE_ACC) {
    u64* oa = out_acc + b * (2 * N2) + c * N2;
#pragma unroll
    for (int e = 0; e < 32; e++) oa[64 * e + lane] = acc[e];
  }
  if (WRITE_BIG) {  // sample extraction at degree 0: a'_0 = A[0], a'_j = -A[N-j], b' = B[0]
    u64* ob = out_big + b * (size_t)(N2 + 1);
    if (c == 0) {
#pragma unroll
      for (int e = 0; e < 32; e++) {
        const int t = 64 * e + lane;
        if (t == 0) ob[0] = acc[e];
        else ob[N2 - t] = 0 - acc[e];
      }
    } else if (lane == 0) {
      ob[N2] = acc[0];
    }
  }
}

}  // namespace fft1k_mb

// root[t] = zeta^t (fft_twiddle, the generator of the other tables), e[64 m1 + L] = (1 + 4 k) mod 4096 in the
// transform's output order.  false: root[0] is not exactly (1, 0) (w - 1 at t_sigma = 0 must be exactly zero)
static bool make_tables_f2k_mb(u64* tw) {
  using namespace fft1k_mb;
  double* r = (double*)(tw + K_ROOT_W);
  for (uint32_t t = 0; t < 4096; t++) fft_twiddle(t, 4096, &r[2 * t], &r[2 * t + 1]);
  u32* e = (u32*)(tw + K_EXP_W);
  for (uint32_t m1 = 0; m1 < 16; m1++)
    for (uint32_t L = 0; L < 64; L++) {
      const uint32_t k = (L & 3) + 4 * (L >> 4) + 16 * ((L >> 2) & 3) + 64 * m1;
      e[64 * m1 + L] = (1 + 4 * k) & 4095u;
    }
  return r[0] == 1.0 && r[1] == 0.0;
}

template <int G>
static hipError_t launch_br2k_mb(const u64* lwe_in, size_t B, int n, const u64* luts, const u32* lut_index, int n_lut,
                                 const u64* bsk, const u64* tw, const u64* tw_mb, u64* out_big, u64* out_acc,
                                 hipStream_t s) {
  using namespace fft1k_mb;
  return launch_out_mode(out_acc, out_big, [&](auto wa, auto wb) {
    hipLaunchKernelGGL((blind_rotate_fft2k_mb_kernel<G, wa(), wb()>), dim3((unsigned)((B + CTS - 1) / CTS)),
                       dim3(64 * NW), 0, s, lwe_in, n, B, luts, lut_index, n_lut, (const double2*)bsk,
                       (const double2*)tw, (const double2*)(tw_mb + K_ROOT_W), (const u32*)(tw_mb + K_EXP_W), out_big,
                       out_acc);
  });
}

static hipError_t blind_rotate_f2k_mb(const u64* lwe_in, size_t B, int n, int g, const u64* luts, const u32* lut_index,
                                      int n_lut, const u64* bsk, const u64* tw, const u64* tw_mb, u64* out_big,
                                      u64* out_acc, hipStream_t s) {
  if (B == 0) return hipSuccess;
  if (n <= 0 || g < 2 || g > 4 || n % g) return hipErrorInvalidValue;
  if (g == 2) return launch_br2k_mb<2>(lwe_in, B, n, luts, lut_index, n_lut, bsk, tw, tw_mb, out_big, out_acc, s);
  if (g == 3) return launch_br2k_mb<3>(lwe_in, B, n, luts, lut_index, n_lut, bsk, tw, tw_mb, out_big, out_acc, s);
  return launch_br2k_mb<4>(lwe_in, B, n, luts, lut_index, n_lut, bsk, tw, tw_mb, out_big, out_acc, s);
}

#ifndef __HIP_DEVICE_COMPILE__  // a host object (pbs_fft2k.hip)
const br_engine_mb ENGINE_FFT2K_MB = {&ENGINE_FFT2K, 2, 4, "blind_rotate_fft2k_mb_kernel", fft1k_mb::K_MB_WORDS,
                                      make_tables_f2k_mb, blind_rotate_f2k_mb};
#endif

}  // namespace tfhe
