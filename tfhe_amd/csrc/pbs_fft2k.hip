// pbs_fft2k.hip — P-FHEVM (N = 2048, k = 1, PBS 2^23 x 1) blind rotation with ONE wave per polynomial component
// (round 4): the 1024-point transform of fft1k.h, restated in oracle/fft_oracle.c (fft1k_fwd / fft1k_inv).
//
// Batch mode (round 4): workgroup = 4 waves = 2 ciphertexts x 2 components, TWO workgroups per CU (80 KB of LDS
// each: the 16 KB pass-A table + 4 skewed 16 KB areas, fft1k.h), so the barriers of one workgroup overlap the other's
// work; latency mode: 8 waves, CTS = 2 (below).  Waves w < 2 CTS are the transform waves (p, c) = (w >> 1, w & 1),
// each holding component c of ciphertext p (2048 u64 = 32 per lane, registers).
// Per CMUX i:
//   transform waves: (X^a acc_c - acc_c) through the wave's LDS area (rotation by DS offsets), 23-bit digits, the
//     forward transform (one LDS transpose), the spectrum D_c stored to the area [slot][lane]
//   barrier
//   MAC, all waves: wave w owns 16 / NW slots of every ciphertext of the workgroup,
//     O_j = D_0 (.) K_{0,j} + D_1 (.) K_{1,j}  (the oracle's fma chain from (0, 0), c = 0 first)
//     with the key words of those slots in registers (two slots requested at the CMUX start, the others when the
//     MAC starts; shared by the CTS ciphertexts), O_j written over D_j in the areas
//   barrier
//   transform waves: O_c from the own area, the inverse transform, acc_c += rint mod 2^64 (two-split form: the
//     23-bit digits give |x| up to 2^106)
// Two barriers per CMUX (the round-1..3 two-wave kernel had five to six: 512-point halves + a combine exchange per
// transform) and no wave waits for a partner mid-transform.  In latency mode (CTS = 2: four transform waves, one per
// SIMD, and four MAC-only waves) a workgroup takes two ciphertexts at the per-CMUX latency of one.  LDS: pass A table
// 16 KB (first, so an area's base minus 16 KB stays inside the block for the rotation's wrapped reads) | 2 CTS areas
// x 16 KB.  (Rounds 1-3 / early round 4: 4 ciphertexts x 8 waves, 8 padded 17 KB areas = 152 KB, one workgroup per CU:
// 45.8 ms per 4096; two workgroups per CU 44.4 ms, with the priority scheme below 42.8 ms,
// profiles/r04i_fhevm_2wg_ab.txt.)
#include "fft1k.h"
#include "pbs_kernels.h"

namespace tfhe {
namespace fft1k {

constexpr int N2 = 2048;

__device__ __forceinline__ int ms4096(u64 x) { return (int)((((x >> 51) + 1) >> 1) & 4095u); }
typedef __attribute__((address_space(3))) u64 lds_u64;

template <int CTS>
struct F1Shared {
  double2 ta[M1];                 // pass A table (K_TA)
  double2 area[2 * CTS][AREA_C64];
};

__device__ __forceinline__ void load_ta(double2* ta, const double2* __restrict__ tg) {
  for (int q = threadIdx.x; q < M1; q += blockDim.x) ta[q] = tg[K_TA + q];
}

// (X^a v - v) through the area, then NEGATED 23-bit digits as doubles: xr[e] <- coefficient L + 64 e, xi[e] <- + 1024.
// Every per-slot decision is wave-uniform, as in pbs_fft.hip's rotate_states (round 5): a = 2048 s + 64 A + r; the image
// is W = X^r v, only slot 31 of the lanes L + r >= 64 wraps on the write; slot e reads W[L + 64 (e - A)] for e >= A,
// -W[L + 64 (e - A + 32)] for e < A, sign xor s: 10 VALU per coefficient instead of the 14 of per-lane compares and
// selects, the same values.
// The digit is the tfhe-rs SignedDecomposer's 2^23 x 1 from the high word h alone (tests/test_fft.py):
// dig23(h) = ((((h + 2^8) >> 9) + 2^22 - 1) mod 2^23) - (2^22 - 1) = ceil((h - 255) / 512) in the signed reading of h with
// the digit range (-2^22, 2^22], so -dig23(h) = floor((255 - h) / 512) = (int)(255 - h) >> 9 (the i32 wrap of 255 - h
// lands exactly the tie h in [2^31 - 256, 2^31 + 256) on -2^22; checked for all 2^32 words).  The transforms run on the
// negated digits against negated key spectra (convert_bsk_f2k), and every product of the MAC -- digit term times
// key term -- is the same double, so the accumulators do not change by a bit.
__device__ __forceinline__ void rotate_digits(const u64 (&v)[32], int a, int lane, double2* area, double (&xr)[16],
                                              double (&xi)[16]) {
  u64* Tu = (u64*)area;
  a = __builtin_amdgcn_readfirstlane(a);  // ms4096(ct[i]): the same for every lane
  const int A = (a >> 6) & 31, r = a & 63;
  const bool sgn = a >= 2048;
  {
    const u32 wb = (u32)(uintptr_t)(lds_u64*)&Tu[lane + r];
#pragma unroll
    for (int e = 0; e < 31; e++) ((lds_u64*)(uintptr_t)wb)[64 * e] = v[e];
    const bool w31 = lane + r >= 64;  // coefficient 1984 + L + r >= 2048: to L + r - 64, negated
    const u32 a31 = w31 ? wb + 1984u * 8u - 16384u : wb + 1984u * 8u;
    *(lds_u64*)(uintptr_t)a31 = w31 ? 0 - v[31] : v[31];
  }
  lds_order();
  const u32 rb = (u32)(uintptr_t)(lds_u64*)&Tu[lane] - 512u * (u32)A;  // >= area - 15.5 KB: the table lies below
  // bit e of wmask: slot e reads the wrapped part (e < A); bit e of mbits: slot e negated.  Bit-field extracts of
  // these SGPR words keep every per-slot decision scalar (a compare would be rebuilt as a per-lane select)
  const u32 wmask = (1u << A) - 1u;
  const u32 mbits = __builtin_amdgcn_readfirstlane(wmask ^ (sgn ? ~0u : 0u));
#pragma unroll
  for (int e = 0; e < 32; e++) {
    // s_bfe_i32 (0 or -1) in inline asm: hipcc's known-bits treat the width-1 sbfe builtin as non-negative and drop
    // the sign extension (a probe kernel stores hi = 0 for it)
    int m32;
    asm("s_bfe_i32 %0, %1, %2" : "=s"(m32) : "s"(mbits), "i"(e | (1 << 16)));
    const u64 M = (u64)(long long)m32;
    const u64 x = ((const lds_u64*)(uintptr_t)(rb + (__builtin_amdgcn_ubfe(wmask, e, 1) << 14)))[64 * e];
    // 255 - hi(y) = hi(~y) + 256 = hi((v + M + 2^40 - 1) - (x ^ M)): the offset rides in the scalar M, so the negated
    // digit is one arithmetic shift of the high word (one VALU fewer per coefficient, the same value)
    const u64 Mz = M + ((1ull << 40) - 1);
    const double d = (double)((int)(u32)(((v[e] + Mz) - (x ^ M)) >> 32) >> 9);
    if (e < 16) xr[e] = d;
    else xi[e - 16] = d;
  }
  lds_order();
}

// NW waves per workgroup: 8 (the MAC spread over 8 waves, 2 slots each) or 2 CTS (every wave a transform wave,
// 16 / NW slots each; with CTS = 2 and 16 KB areas two workgroups share a CU)
#ifndef FFT_WGTIME
#define FFT_WGTIME 0
#endif
#if FFT_WGTIME
// diagnostic build only (as pbs_fft.hip): per-workgroup start / end, HW_ID, XCC_ID of the last launch
__device__ unsigned long long g_wgt2k[4 * 16384];
#endif
template <int CTS, int NW, bool WRITE_ACC, bool WRITE_BIG>
__global__ __launch_bounds__(64 * NW, 8 / NW) void blind_rotate_fft2k_kernel(
    const u64* __restrict__ lwe_in, int n, size_t B, const u64* __restrict__ luts, const u32* __restrict__ lut_index,
    int n_lut, const double2* __restrict__ bsk, const double2* __restrict__ tg, u64* __restrict__ out_big,
    u64* __restrict__ out_acc) {
  __shared__ __attribute__((aligned(16))) F1Shared<CTS> sh;
#if FFT_WGTIME
  const unsigned long long wg_t0 = __builtin_amdgcn_s_memrealtime();
#endif
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const bool tw_wave = wave_s < 2 * CTS;
  const int c = wave & 1, p = tw_wave ? wave >> 1 : 0;
  const size_t b_raw = (size_t)blockIdx.x * CTS + p;
  const bool live = tw_wave && b_raw < B;
  const size_t b = b_raw < B ? b_raw : B - 1;  // padding waves run a copy of the last ciphertext, store nothing
  const u64* ct = lwe_in + b * (size_t)(n + 1);
  double2* area = sh.area[tw_wave ? wave : 0];

  load_ta(sh.ta, tg);
  TwB tb;
  tb.load(tg, lane);
  u64 acc[32];
  if (tw_wave) {  // acc_c: A = 0, B = X^{-b~} * lut (LUT values in the Z_p encoding, mapped to the torus)
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

  int a_next = tw_wave ? ms4096(ct[0]) : 0;
  constexpr int SPW = 16 / NW;  // MAC slots per wave
  static_assert(NW == 8 || NW == 2 * CTS, "waves: 8, or one per polynomial");
  const int s0 = SPW * wave_s;  // MAC slots s0 .. s0 + SPW - 1
  // In the two-workgroup batch kernel the workgroups of the second dispatch half (blockIdx bit 8: with 256 CUs, the
  // second workgroup each CU receives first; MI355X only, on other CU counts the two workgroups of a CU just get an
  // arbitrary split) run at the higher wave priority, so the two workgroups of a CU drift apart instead of reaching
  // their barriers together: 44.24 -> 43.35 ms per 4096 on the same box (late round 4, profiles/r04i_fhevm_2wg_ab.txt)
  if constexpr (NW == 2 * CTS)
    if ((blockIdx.x >> 8) & 1) __builtin_amdgcn_s_setprio(1);
  // key words of CMUX i for the MAC phase: kv[t][cc][j] = K_{cc,j}[slot s0 + t][lane].  The first KPRE slots are
  // requested at the CMUX start (their latency hides behind the forward transform); with 4 slots per wave the
  // other two are requested after the forward transform (holding all four across the transform spills).
  constexpr int KPRE = SPW < 2 ? SPW : 2;
  auto load_key = [&](int i, double2 (&kv)[SPW][2][2], bool late) {
#pragma unroll
    for (int t = 0; t < SPW; t++)
      if ((t >= KPRE) == late)
#pragma unroll
        for (int cc = 0; cc < 2; cc++)
#pragma unroll
          for (int j = 0; j < 2; j++) kv[t][cc][j] = bsk[((size_t)(i * 2 + cc) * 2 + j) * M1 + 64 * (s0 + t) + lane];
  };
  auto cmux = [&](int i, double2 (&kv)[SPW][2][2]) {
    const int a = a_next;
    if (tw_wave && i + 1 < n) a_next = ms4096(ct[i + 1]);
    if (tw_wave) {
      double xr[16], xi[16];
      rotate_digits(acc, a, lane, area, xr, xi);
      fft1k_fwd(xr, xi, area, lane, sh.ta, tb);
#pragma unroll
      for (int s = 0; s < 16; s++) area[64 * s + lane] = make_double2(xr[s], xi[s]);
    }
    // the other key slots: requested before the barrier (the transform's registers are free by now), so their
    // latency overlaps the wait (+0.3-0.5 %, profiles/r04i_fhevm_2wg_ab.txt)
    if constexpr (SPW > KPRE) load_key(i, kv, true);
    __syncthreads();
    // every wave runs the short MAC phase at the top priority and then returns to its workgroup's level, so a CU's MAC
    // phases are not stalled behind the other workgroup's transforms: 43.43 -> 42.77 ms per 4096 on the same box
    // (profiles/r04i_fhevm_2wg_ab.txt)
    __builtin_amdgcn_s_setprio(3);
#pragma unroll
    for (int q = 0; q < CTS; q++) {
#pragma unroll
      for (int t = 0; t < SPW; t++) {
        const int idx = 64 * (s0 + t) + lane;
        const double2 d0 = sh.area[2 * q][idx], d1 = sh.area[2 * q + 1][idx];
        double2 o[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const double2 k0 = kv[t][0][j], k1 = kv[t][1][j];
          double re = __builtin_fma(d0.x, k0.x, 0.0);
          re = __builtin_fma(-d0.y, k0.y, re);
          double im = __builtin_fma(d0.x, k0.y, 0.0);
          im = __builtin_fma(d0.y, k0.x, im);
          re = __builtin_fma(d1.x, k1.x, re);
          re = __builtin_fma(-d1.y, k1.y, re);
          im = __builtin_fma(d1.x, k1.y, im);
          im = __builtin_fma(d1.y, k1.x, im);
          o[j] = make_double2(re, im);
        }
        sh.area[2 * q][idx] = o[0];
        sh.area[2 * q + 1][idx] = o[1];
      }
    }
    __syncthreads();
    if (NW == 2 * CTS && ((blockIdx.x >> 8) & 1)) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
    if (tw_wave) {
      double xr[16], xi[16];
#pragma unroll
      for (int s = 0; s < 16; s++) {
        const double2 v = area[64 * s + lane];
        xr[s] = v.x;
        xi[s] = v.y;
      }
      fft1k_inv(xr, xi, area, lane, sh.ta, tb);
#pragma unroll
      // the keys' spectra carry 2^-32 (scale 2^-42 at conversion), so the inverse transform returns y = x * 2^-32 bit for
      // bit and the accumulator update starts at floor(y) (round 5)
      for (int e = 0; e < 16; e++) {
        acc[e] = torus_acc_add_wide_y(acc[e], xr[e]);
        acc[e + 16] = torus_acc_add_wide_y(acc[e + 16], xi[e]);
      }
    }
  };
  for (int i = 0; i < n; i++) {
    double2 kv[SPW][2][2];  // requested at the CMUX start, consumed after the rotation and forward transform
    load_key(i, kv, false);
    cmux(i, kv);
  }
#if FFT_WGTIME
  if (threadIdx.x == 0 && blockIdx.x < 16384) {
    const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
    g_wgt2k[4 * blockIdx.x] = wg_t0;
    g_wgt2k[4 * blockIdx.x + 1] = t1;
    g_wgt2k[4 * blockIdx.x + 2] = (unsigned)__builtin_amdgcn_s_getreg(4 | (31 << 11));
    g_wgt2k[4 * blockIdx.x + 3] = (unsigned)__builtin_amdgcn_s_getreg(20 | (31 << 11));
  }
#endif

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

// one wave per polynomial: natural coefficients (int64 torus words) -> spectrum [slot][lane] x scale
__global__ __launch_bounds__(64) void fwd2k_kernel(const u64* __restrict__ in, double2* __restrict__ out,
                                                   const double2* __restrict__ tg, double scale) {
  __shared__ __attribute__((aligned(16))) double2 ta[M1];
  __shared__ __attribute__((aligned(16))) double2 area[AREA_C64];
  const int lane = threadIdx.x;
  load_ta(ta, tg);
  TwB tb;
  tb.load(tg, lane);
  const u64* src = in + (size_t)blockIdx.x * N2;
  double xr[16], xi[16];
#pragma unroll
  for (int e = 0; e < 16; e++) {
    xr[e] = i64_to_f64(src[64 * e + lane]);
    xi[e] = i64_to_f64(src[64 * e + lane + M1]);
  }
  __syncthreads();
  fft1k_fwd(xr, xi, area, lane, ta, tb);
  double2* dst = out + (size_t)blockIdx.x * M1;
#pragma unroll
  for (int s = 0; s < 16; s++) dst[64 * s + lane] = make_double2(xr[s] * scale, xi[s] * scale);
}

// inverse for the parity tests: spectrum [slot][lane] -> 2048 doubles (no 1/M, no rounding)
__global__ __launch_bounds__(64) void inv2k_kernel(const double2* __restrict__ in, double* __restrict__ out,
                                                   const double2* __restrict__ tg) {
  __shared__ __attribute__((aligned(16))) double2 ta[M1];
  __shared__ __attribute__((aligned(16))) double2 area[AREA_C64];
  const int lane = threadIdx.x;
  load_ta(ta, tg);
  TwB tb;
  tb.load(tg, lane);
  const double2* src = in + (size_t)blockIdx.x * M1;
  double xr[16], xi[16];
#pragma unroll
  for (int s = 0; s < 16; s++) {
    const double2 v = src[64 * s + lane];
    xr[s] = v.x;
    xi[s] = v.y;
  }
  __syncthreads();
  fft1k_inv(xr, xi, area, lane, ta, tb);
  double* dst = out + (size_t)blockIdx.x * N2;
#pragma unroll
  for (int e = 0; e < 16; e++) {
    dst[64 * e + lane] = xr[e];
    dst[64 * e + lane + M1] = xi[e];
  }
}

}  // namespace fft1k

#if FFT_WGTIME
extern "C" int tfhe_hip_debug_wgtimes2k(unsigned long long* out, size_t n) {
  if (n > 4 * 16384) n = 4 * 16384;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(fft1k::g_wgt2k), n * 8, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

// ta[k][L] = zeta^{L (1 + 4 k)}, tb[m][l0] = zeta^{64 l0 m}, zeta = e^{2 pi i / 4096} (the oracle's tab1k)
// false: the compile-time slot constants differ from the table generator's zeta^{64 e} in some bit
static bool make_tables_f2k(u64* tw) {
  using namespace fft1k;
  double* t = (double*)tw;
  for (uint32_t k = 0; k < 16; k++)
    for (uint32_t L = 0; L < 64; L++) {
      const int o = K_TA + 64 * k + L;
      fft_twiddle((L * (1 + 4 * k)) % 4096, 4096, &t[2 * o], &t[2 * o + 1]);
    }
  for (uint32_t m = 0; m < 4; m++)
    for (uint32_t l = 0; l < 16; l++) {
      const int o = K_TB + 16 * m + l;
      fft_twiddle((64 * l * m) % 4096, 4096, &t[2 * o], &t[2 * o + 1]);
    }
  for (int e = 0; e < 16; e++) {
    double c, s;
    fft_twiddle(64u * e, 4096u, &c, &s);
    if (c != ctw16::SLOT[e].x || s != ctw16::SLOT[e].y) return false;
  }
  return true;
}

// one wave per polynomial through fwd2k_kernel; the key spectra negated (rotate_digits) and x 2^-42
static hipError_t fwd_scaled_f2k(const u64* in, size_t count, u64* out, const u64* tw, double scale, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(fft1k::fwd2k_kernel, dim3((unsigned)count), dim3(64), 0, s, in, (double2*)out, (const double2*)tw,
                     scale);
  return hipGetLastError();
}
static hipError_t convert_bsk_f2k(const u64* bsk_std, u64* bsk_f, size_t polys, const u64* tw, hipStream_t s) {
  return fwd_scaled_f2k(bsk_std, polys, bsk_f, tw, -0x1p-42, s);
}
static hipError_t fft_fwd_f2k(const u64* in, size_t count, u64* out, const u64* tw, hipStream_t s) {
  return fwd_scaled_f2k(in, count, out, tw, 1.0, s);
}

static hipError_t fft_inv_f2k(const u64* in, size_t count, u64* out, const u64* tw, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(fft1k::inv2k_kernel, dim3((unsigned)count), dim3(64), 0, s, (const double2*)in, (double*)out,
                     (const double2*)tw);
  return hipGetLastError();
}

template <int CTS, int NW>
static hipError_t launch_br2k(const u64* lwe_in, size_t B, int n, const u64* luts, const u32* lut_index, int n_lut,
                              const double2* bk, const double2* t, u64* out_big, u64* out_acc, hipStream_t s) {
  return launch_out_mode(out_acc, out_big, [&](auto wa, auto wb) {
    hipLaunchKernelGGL((fft1k::blind_rotate_fft2k_kernel<CTS, NW, wa(), wb()>), dim3((unsigned)((B + CTS - 1) / CTS)),
                       dim3(64 * NW), 0, s, lwe_in, n, B, luts, lut_index, n_lut, bk, t, out_big, out_acc);
  });
}

// latency: two ciphertexts per workgroup (four transform waves on four SIMDs, eight MAC waves); batch: two per
// workgroup of four waves, two workgroups per CU (16 KB areas; with the padded 17 KB areas of F1_SWZ = 0 four per
// workgroup of eight waves, two transform waves per SIMD)
static hipError_t blind_rotate_f2k(const u64* lwe_in, size_t B, int n, const u64* luts, const u32* lut_index,
                                   int n_lut, const u64* bsk_f, const u64* tw, u64* out_big, u64* out_acc,
                                   bool latency, int, hipStream_t s) {
  if (B == 0) return hipSuccess;
  const double2 *bk = (const double2*)bsk_f, *t = (const double2*)tw;
  if (latency) return launch_br2k<2, 8>(lwe_in, B, n, luts, lut_index, n_lut, bk, t, out_big, out_acc, s);
#if F1_SWZ != 0
  return launch_br2k<2, 4>(lwe_in, B, n, luts, lut_index, n_lut, bk, t, out_big, out_acc, s);
#else
  return launch_br2k<4, 8>(lwe_in, B, n, luts, lut_index, n_lut, bk, t, out_big, out_acc, s);
#endif
}

// latency crossover 512: the one-wave kernel in latency mode covers 512 ciphertexts in one round over 256 CUs;
// both modes run blind_rotate_fft2k_kernel (<2, 8, ...> latency, <2, 4, ...> batch)
#ifndef __HIP_DEVICE_COMPILE__  // a host object: the device pass would emit it with its pointers to host functions
const br_engine ENGINE_FFT2K = {true,
                                fft1k::N2,
                                512,
                                "blind_rotate_fft2k_kernel",
                                "blind_rotate_fft2k_kernel",
                                2 * fft1k::K_C64,
                                make_tables_f2k,
                                convert_bsk_f2k,
                                blind_rotate_f2k,
                                fft_fwd_f2k,
                                fft_inv_f2k};
#endif

}  // namespace tfhe
