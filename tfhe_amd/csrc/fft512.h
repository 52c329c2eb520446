// fft512.h — the 512-point complex DFT building blocks of the FFT64 engine (gfx950), shared by the
// N = 1024 kernels (pbs_fft.hip: one wave per polynomial) and the N = 2048 kernels (pbs_fft2k.hip: two
// waves per polynomial, each running one 512-point half).  One fixed f64 operation sequence, restated
// in oracle/fft_oracle.c; contraction stays off in every file that includes this header.
#pragma once
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "gl64.h"
#include "ntt1024.h"

namespace tfhe {
namespace fftk {

constexpr int M = 512;
constexpr int S1 = 72, S2 = 65;   // transpose row strides (complex): T1 (passes A|B), T2 (passes B|C)
constexpr int T_C64 = 576;        // per-wave transpose scratch (9,216 B; also holds 1024 u64)
constexpr int TW_TWIST = 0, TW_A = 512, TW_B = 1024, TW_I = 1536, TW_C64 = 2048;  // table offsets (complex)
constexpr double SQRT1_2 = 0.70710678118654752440;

// Order between a wave's own LDS writes and reads of its private scratch: a full lgkmcnt(0) drain.  DS instructions of
// one wavefront execute in issue order, so a compiler-only fence would do; measured on MI355X that is 4 % SLOWER (31.97
// vs 30.71 ms per 4096-PBS blind rotation: hipcc then interleaves the transpose reads with the butterflies and stalls on
// them one by one).
__device__ __forceinline__ void lds_order() { wave_lds_sync(); }

// z * w (INV: z * conj(w)), the oracle's cmul(z, w.re, +-w.im)
template <bool INV>
__device__ __forceinline__ void cmul(double& re, double& im, double2 w) {
  const double p = re, q = im;
  if (!INV) {
    re = __builtin_fma(p, w.x, -(q * w.y));
    im = __builtin_fma(p, w.y, q * w.x);
  } else {
    re = __builtin_fma(p, w.x, q * w.y);
    im = __builtin_fma(p, -w.y, q * w.x);
  }
}

// t * e^{+-i pi J / 4} (oracle w8) for J = 2, the one the transforms use as such: the odd J carry a sqrt(1/2) that
// dft8 below and fft1k.h's dft16 fold into fmas
template <bool INV, int J>
__device__ __forceinline__ void w8(double& re, double& im) {
  static_assert(J == 2, "w8^1 and w8^3 are folded into the butterflies that use them");
  const double p = re, q = im;
  if (!INV) { re = -q; im = p; }
  else { re = q; im = -p; }
}

// The odd half of the 8-point DFT carries its sqrt(1/2) factor folded into the last stage's fmas (round 5).  With y5 = s u5,
// y7 = s u7 (u the unscaled w8 forms, s = sqrt(1/2)), z5 = s (u5 + u7) and z7 = s (u5 - u7), so x1 / x5 = z4 +- s (u5 + u7)
// and x3 / x7 = z6 +- (+-i) s (u5 - u7) are 8 fmas: 52 f64 instructions per DFT8 instead of the 56 of three plain radix-2
// stages (4 multiplies fewer), -48 per wave and CMUX in the P-GATE pair kernel.  The rounding sequence is restated in
// oracle/fft_oracle.c:dft8 (and judged by the exact arbiter).
// 8-point DFT in registers, natural order in and out (radix-2 DIF, bit-reversal by renaming)
template <bool INV>
__device__ __forceinline__ void dft8(double (&xr)[8], double (&xi)[8]) {
  double yr[4], yi[4];  // stage 1, even half: y_j = x_j + x_(j+4)
#pragma unroll
  for (int j = 0; j < 4; j++) {
    yr[j] = xr[j] + xr[j + 4];
    yi[j] = xi[j] + xi[j + 4];
  }
  // odd half: t_j = x_j - x_(j+4); y4 = t0, y6 = (+-i) t2, y5 / y7 = s u5 / s u7 (u5, u7 kept unscaled)
  const double t0r = xr[0] - xr[4], t0i = xi[0] - xi[4];
  const double t1r = xr[1] - xr[5], t1i = xi[1] - xi[5];
  const double t2r = xr[2] - xr[6], t2i = xi[2] - xi[6];
  const double t3r = xr[3] - xr[7], t3i = xi[3] - xi[7];
  double ar, ai, cr, ci;  // u5 = (ar, ai), u7 = (cr, ci)
  if (!INV) {
    ar = t1r - t1i; ai = t1r + t1i;        // w8^1 / s
    cr = -(t3r + t3i); ci = t3r - t3i;     // w8^3 / s
  } else {
    ar = t1r + t1i; ai = t1i - t1r;
    cr = t3i - t3r; ci = -(t3r + t3i);
  }
  const double z5r = ar + cr, z5i = ai + ci;  // z5 / s
  const double z7r = ar - cr, z7i = ai - ci;  // z7 / s (before its rotation by +-i)
  // z4 = y4 + y6, z6 = y4 - y6 with y6 = (+-i) t2
  const double z4r = INV ? t0r + t2i : t0r - t2i, z4i = INV ? t0i - t2r : t0i + t2r;
  const double z6r = INV ? t0r - t2i : t0r + t2i, z6i = INV ? t0i + t2r : t0i - t2r;
  // even half: stages 2 and 3 as before
  const double e0r = yr[0] + yr[2], e0i = yi[0] + yi[2];
  const double e2r = yr[0] - yr[2], e2i = yi[0] - yi[2];
  const double e1r = yr[1] + yr[3], e1i = yi[1] + yi[3];
  double e3r = yr[1] - yr[3], e3i = yi[1] - yi[3];
  w8<INV, 2>(e3r, e3i);
  xr[0] = e0r + e1r; xi[0] = e0i + e1i;
  xr[4] = e0r - e1r; xi[4] = e0i - e1i;
  xr[2] = e2r + e3r; xi[2] = e2i + e3i;
  xr[6] = e2r - e3r; xi[6] = e2i - e3i;
  // odd half, stage 3 with s folded: x1 = z4 + s z5', x5 = z4 - s z5', x3 = z6 + r(s z7'), x7 = z6 - r(s z7'),
  // r = multiplication by +i (forward) / -i (inverse)
  xr[1] = __builtin_fma(SQRT1_2, z5r, z4r); xi[1] = __builtin_fma(SQRT1_2, z5i, z4i);
  xr[5] = __builtin_fma(-SQRT1_2, z5r, z4r); xi[5] = __builtin_fma(-SQRT1_2, z5i, z4i);
  if (!INV) {  // r z = (-z.im, z.re)
    xr[3] = __builtin_fma(-SQRT1_2, z7i, z6r); xi[3] = __builtin_fma(SQRT1_2, z7r, z6i);
    xr[7] = __builtin_fma(SQRT1_2, z7i, z6r); xi[7] = __builtin_fma(-SQRT1_2, z7r, z6i);
  } else {     // r z = (z.im, -z.re)
    xr[3] = __builtin_fma(SQRT1_2, z7i, z6r); xi[3] = __builtin_fma(-SQRT1_2, z7r, z6i);
    xr[7] = __builtin_fma(-SQRT1_2, z7i, z6r); xi[7] = __builtin_fma(SQRT1_2, z7r, z6i);
  }
}

// 64-bit register exchanges across the wave: v_permlane32_swap / v_permlane16_swap (gfx950: each swaps one operand's upper
// 32-lane half / odd 16-lane rows with the other's lower half / even rows, probed in tools/microbench/permlane_probe.hip).
// fft1k.h's exchange_hi is built on them.  (A register form of this header's transpose 1 from the same moves was measured
// and lost: the P-GATE batch kernel 27.40 -> 28.80 ms -- its 96 cross-lane moves and selects cost more VALU time than the
// 16 LDS operations and two waits they replace.)
typedef unsigned int u32x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void swap32_d(double& a, double& b) {
  const u32x2v x = __builtin_bit_cast(u32x2v, a), y = __builtin_bit_cast(u32x2v, b);
  const auto lo = __builtin_amdgcn_permlane32_swap(x.x, y.x, false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap(x.y, y.y, false, false);
  a = __builtin_bit_cast(double, (u32x2v){lo[0], hi[0]});
  b = __builtin_bit_cast(double, (u32x2v){lo[1], hi[1]});
}
__device__ __forceinline__ void swap16_d(double& a, double& b) {
  const u32x2v x = __builtin_bit_cast(u32x2v, a), y = __builtin_bit_cast(u32x2v, b);
  const auto lo = __builtin_amdgcn_permlane16_swap(x.x, y.x, false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap(x.y, y.y, false, false);
  a = __builtin_bit_cast(double, (u32x2v){lo[0], hi[0]});
  b = __builtin_bit_cast(double, (u32x2v){lo[1], hi[1]});
}
template <bool INV>
__device__ __forceinline__ void twist_slots(double (&xr)[8], double (&xi)[8]);

// the slot twist + pass A's DFT8 of the N = 1024 forward transform (natural order in and out): twist, then DFT8.  The two
// merged into ONE twisted DFT8 (a negacyclic-style split into 12 tangent-form butterflies, 72 f64 instructions against
// 28 + 52) was measured SLOWER on MI355X (round 5, same box, three rounds: 24.76 vs 24.62 ms per 4096,
// profiles/r05c_ab_tdft8.txt: the three dependent fma stages and 3 spilled VGPRs cost more than the 8 f64 instructions
// saved).
__device__ __forceinline__ void twist_dft8_fwd(double (&xr)[8], double (&xi)[8]) {
  twist_slots<false>(xr, xi);
  dft8<false>(xr, xi);
}

// per-lane transpose bases: b1 = T1 read / inverse write, b2 = T2 read / inverse write
struct TBase {
  int b1, b2;
  __device__ __forceinline__ explicit TBase(int lane)
      : b1((lane >> 3) * S1 + (lane & 7)), b2((lane & 7) * S2 + 8 * (lane >> 3)) {}
};

// ---------------------------------------------------------------------------------------------
// The 512-point transform: three DFT8 passes over the slots with two transposes of the wave-private LDS area between
// them.  Forward: natural order in (lane L, slot e <-> L + 64 e, the input not yet twisted: pass A's DFT8 is
// twist_dft8_fwd), device order out; the transpose after pass A multiplies by pass A's twiddles (slot 0 too: the
// N = 1024 tables fold the lane part of the twist into pass A), the one after pass B by pass B's (slots 1..7).  Inverse
// (no 1/M): device order in, natural order out -- the forward's passes reversed, the twiddles conjugated: pass C' takes
// pass B's table, pass B' the TW_I table.  Two forms of each: every twiddle from a table (twA, twB, twI: 512
// complex each, [64 e + L]; TW_A | TW_B | TW_I of the table tw) with plain transposes -- multiply, store, full drain, load, full drain -- and the
// pair kernel's, with pass A's and pass B's twiddles in registers and the transposes placed by hand (xpose_p below).
__device__ __forceinline__ void dft512_fwd_t(double (&xr)[8], double (&xi)[8], double2* T, int lane, TBase tb,
                                             const double2* twA, const double2* twB) {
  twist_dft8_fwd(xr, xi);
#pragma unroll
  for (int e = 0; e < 8; e++) cmul<false>(xr[e], xi[e], twA[64 * e + lane]);
#pragma unroll
  for (int e = 0; e < 8; e++) T[lane + S1 * e] = make_double2(xr[e], xi[e]);
  lds_order();
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const double2 v = T[tb.b1 + 8 * e];
    xr[e] = v.x;
    xi[e] = v.y;
  }
  lds_order();
  dft8<false>(xr, xi);
#pragma unroll
  for (int e = 1; e < 8; e++) cmul<false>(xr[e], xi[e], twB[64 * e + lane]);
#pragma unroll
  for (int e = 0; e < 8; e++) T[lane + S2 * e] = make_double2(xr[e], xi[e]);
  lds_order();
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const double2 v = T[tb.b2 + e];
    xr[e] = v.x;
    xi[e] = v.y;
  }
  lds_order();
  dft8<false>(xr, xi);
}

__device__ __forceinline__ void dft512_inv_t(double (&xr)[8], double (&xi)[8], double2* T, int lane, TBase tb,
                                             const double2* twB, const double2* twI) {
  dft8<true>(xr, xi);
#pragma unroll
  for (int e = 1; e < 8; e++) cmul<true>(xr[e], xi[e], twB[64 * e + lane]);
#pragma unroll
  for (int e = 0; e < 8; e++) T[tb.b2 + e] = make_double2(xr[e], xi[e]);
  lds_order();
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const double2 v = T[lane + S2 * e];
    xr[e] = v.x;
    xi[e] = v.y;
  }
  lds_order();
  dft8<true>(xr, xi);
#pragma unroll
  for (int e = 0; e < 8; e++) cmul<true>(xr[e], xi[e], twI[64 * e + lane]);
#pragma unroll
  for (int e = 0; e < 8; e++) T[tb.b1 + 8 * e] = make_double2(xr[e], xi[e]);
  lds_order();
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const double2 v = T[lane + S1 * e];
    xr[e] = v.x;
    xi[e] = v.y;
  }
  lds_order();
  dft8<true>(xr, xi);
}

__device__ __forceinline__ void dft512_fwd(double (&xr)[8], double (&xi)[8], double2* T, int lane, TBase tb,
                                           const double2* tw) {
  dft512_fwd_t(xr, xi, T, lane, tb, tw + TW_A, tw + TW_B);
}
__device__ __forceinline__ void dft512_inv(double (&xr)[8], double (&xi)[8], double2* T, int lane, TBase tb,
                                           const double2* tw) {
  dft512_inv_t(xr, xi, T, lane, tb, tw + TW_B, tw + TW_I);
}

// One transpose with the twiddles w[e] in registers and its LDS traffic placed by hand (round 7): slots E0.. times w
// (INV: conj w), stores at Tw[WS e], reads from Tr[RS e].  Pure placement of stores, loads
// and waits: the f64 operations, their operands and their order are those of the plain transposes above.
//   * per slot, the twiddle multiply and then that slot's transpose store, the order pinned, so a ds_write_b128 goes out
//     under the next slot's four f64 instructions (hipcc's own schedule is all eight multiplies, a full drain, then eight
//     stores back to back with the wave issuing nothing else);
//   * no s_waitcnt between the stores and the reads of the same private area (DS operations of one wave execute in issue
//     order; the ordering left is compiler-only), the eight reads pinned as ONE group in the order the next DFT8's first
//     stage consumes them (0, 4, 1, 5, 2, 6, 3, 7) and consumed under hipcc's counted lgkmcnt waits.  (A compiler-only
//     fence in lds_order lost because it left the reads free to scatter.)
// Measured on MI355X, same box, three interleaved rounds, ms per 4096-PBS blind rotation (profiles/r07b_ab_steps.txt,
// DESIGN 3j): the two pay only TOGETHER.  On top of the pipelined MAC (22.73): the first alone 22.80, both 22.61 (round-6
// code 22.90); the second without the first is slower than round 6 (23.13 against 22.95 on another box).  Reading the
// inverse's eight pass-B' twiddles as one early group was measured too and lost 0.05-0.12 ms:
// tools/ab_patches/r07_twi_group.patch.
template <bool INV, int E0, int WS, int RS>
__device__ __forceinline__ void xpose_p(double (&xr)[8], double (&xi)[8], const double2 (&w)[8], double2* Tw,
                                        const double2* Tr) {
#pragma unroll
  for (int e = 0; e < 8; e++) {
    if (e >= E0) cmul<INV>(xr[e], xi[e], w[e]);
    Tw[WS * e] = make_double2(xr[e], xi[e]);
    __builtin_amdgcn_sched_barrier(0);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int e = (k >> 1) + 4 * (k & 1);
    const double2 v = Tr[RS * e];
    xr[e] = v.x;
    xi[e] = v.y;
  }
  __builtin_amdgcn_sched_barrier(0);
}

// wb[0] is unused
__device__ __forceinline__ void dft512_fwd_rab_p(double (&xr)[8], double (&xi)[8], double2* T, int lane, TBase tb,
                                                 const double2 (&wa)[8], const double2 (&wb)[8]) {
  twist_dft8_fwd(xr, xi);
  xpose_p<false, 0, S1, 8>(xr, xi, wa, T + lane, T + tb.b1);
  dft8<false>(xr, xi);
  xpose_p<false, 1, S2, 1>(xr, xi, wb, T + lane, T + tb.b2);
  dft8<false>(xr, xi);
}

// pass C' from wb, pass B' from the LDS table twI
__device__ __forceinline__ void dft512_inv_rb_p(double (&xr)[8], double (&xi)[8], double2* T, int lane, TBase tb,
                                                const double2 (&wb)[8], const double2* twI) {
  dft8<true>(xr, xi);
  xpose_p<true, 1, 1, S2>(xr, xi, wb, T + tb.b2, T + lane);
  dft8<true>(xr, xi);
  double2 wi[8];  // pass B' twiddles: a constant LDS table, read where hipcc places them (between the multiplies)
#pragma unroll
  for (int e = 0; e < 8; e++) wi[e] = twI[64 * e + lane];
  xpose_p<true, 0, 8, S1>(xr, xi, wi, T + tb.b1, T + lane);
  dft8<true>(xr, xi);
}

// ---------------------------------------------------------------------------------------------
// N = 1024 (P-GATE) merged twist.  z_j = a_j zeta^j with j = L + 64 e splits as zeta^L * zeta^(64 e): the
// slot part c_e = zeta^(64 e) is a per-slot constant (an SGPR operand, no table read) applied before
// pass A, and the lane part zeta^L commutes with pass A's 8-point DFT over the slots, so it is folded
// into pass A's table: TW_A[e][L] = w^(L e) zeta^L = zeta^(L (1 + 4 e)).  The inverse does the mirror
// image: zeta^(n0 + 8 n1) rides in pass B''s table (TW_I[e][L] = zeta^((n0 + 8 e)(4 k0 + 1)), L = n0 + 8
// k0), conj(c_e) is applied after pass A'.  Saves 15 of the 54 LDS reads of a forward digit transform
// and 8 of an inverse (oracle/fft_oracle.c: or_fft_fwd / or_fft_inv at N = 1024 restate the order).
// N = 2048 (pbs_fft2k.hip) does the same per parity h: zeta_4096^(2 m + h) = zeta^(2 L + h) zeta^(128 e), the
// slot constants are the same values (128 e / 4096 = 64 e / 2048), the tables A'_h, I'_h per parity.
// The constants come from the table generator's own series, evaluated at compile time (IEEE double,
// no contraction in constant evaluation) so they equal the host tables bit for bit.
namespace ctw {
constexpr double sin_s(double x) {
  double x2 = x * x, term = x, sum = 0.0;
  for (int i = 1; i <= 21; i += 2) { sum += term; term = -term * x2 / (double)((i + 1) * (i + 2)); }
  return sum;
}
constexpr double cos_s(double x) {
  double x2 = x * x, term = 1.0, sum = 0.0;
  for (int i = 0; i <= 20; i += 2) { sum += term; term = -term * x2 / (double)((i + 1) * (i + 2)); }
  return sum;
}
struct c64 {
  double x, y;
};
// cos / sin (2 pi t / 2048) for t = 64 e, e = 0..7 (t <= 448 < M / 4: octant and quarter cases only)
constexpr c64 slot(int e) {
  const unsigned t = 64u * (unsigned)e, m = 2048u;
  if (8 * t > m) {
    const double x = (double)(m / 4 - t) * (6.28318530717958647692 / (double)m);
    return c64{sin_s(x), cos_s(x)};
  }
  const double x = (double)t * (6.28318530717958647692 / (double)m);
  return c64{cos_s(x), sin_s(x)};
}
constexpr c64 SLOT[8] = {slot(0), slot(1), slot(2), slot(3), slot(4), slot(5), slot(6), slot(7)};
}  // namespace ctw

// z * c_e (forward) / z * conj(c_e) (inverse) for slot e > 0, c_e a compile-time constant; the
// operation order of cmul
template <bool INV>
__device__ __forceinline__ void twist_slots(double (&xr)[8], double (&xi)[8]) {
#pragma unroll
  for (int e = 1; e < 8; e++) {
    const double wr = ctw::SLOT[e].x, wi = ctw::SLOT[e].y;
    const double p = xr[e], q = xi[e];
    if (!INV) {
      xr[e] = __builtin_fma(p, wr, -(q * wi));
      xi[e] = __builtin_fma(p, wi, q * wr);
    } else {
      xr[e] = __builtin_fma(p, wr, q * wi);
      xi[e] = __builtin_fma(p, -wi, q * wr);
    }
  }
}

// (double)(int64)x, correctly rounded: exact hi * 2^32 plus exact lo, one rounding
__device__ __forceinline__ double i64_to_f64(u64 x) {
  return __builtin_fma((double)(int)(x >> 32), 0x1p32, (double)(u32)x);
}

// The accumulator update: acc += rint(x) mod 2^64 without the rint and without building the u64 from two halves (round 5).
// h = floor(x 2^-32), l = fma(-h, 2^32, x) (exact whenever |x| >= 2^32 or h = 0; for -2^32 < x < 0 it is x + 2^32 rounded
// once), and the two words come straight out of doubles' bit patterns:
//   l + 2^52                     bits = 0x43300000_00000000 + rint(l)        (rint(l) may be 2^32: the carry is kept)
//   h + (1.5 2^52 - 0x43300000)  low word = (h - 0x43300000) mod 2^32       (|h| < 2^51 - 2^32)
// acc += (hb << 32) + lb (two v_lshl_add_u64), the 0x43300000 offsets cancel mod 2^64.  The value is h 2^32 + rint(l):
// rint(x) mod 2^64 exactly, except that a tiny negative x (|x| < 2^32) rounds twice (x + 2^32, then to an integer) --
// oracle/fft_oracle.c:or_f64_to_torus_dev restates these operations.  The kernels run the two forms below, which start
// from y = x 2^-32 (the keys' spectra carry the 2^-32) and give the same bits in fewer operations (tests/test_fft.py
// restates all three).

// acc + (low word of d's bit pattern) << 32: a 32-bit add on acc's high word (no carry can come from below; hipcc
// otherwise moves the word into the high half of a fresh pair for a 64-bit add -- v_lshl_add_u64 shifts by 0..4 only)
__device__ __forceinline__ u64 add_hi_word(u64 acc, double d) {
  const u32x2v a = __builtin_bit_cast(u32x2v, acc);
  const u32x2v w = __builtin_bit_cast(u32x2v, d);
  return __builtin_bit_cast(u64, (u32x2v){a.x, a.y + w.x});
}
// the update by x = y * 2^32 (|x| < 2^83), given y: the N = 1024 keys' spectra carry 2^-32 (bsk_to_fourier_kernel
// scales by 2^-41) and, as for torus_acc_add_wide_y below, the MAC and the inverse transform then return
// x * 2^-32 bit for bit.  h = floor(y), (y - h) + 2^20 = 2^-32 RN(l + 2^52) (low word rint(l), high word 0x41300000),
// h + 1.5 2^52 - 0x41300000 (low word h - 0x41300000 mod 2^32): the rint-free update above, bit for bit, in four f64
// operations instead of five (the oracle's or_f64_to_torus_dev)
__device__ __forceinline__ u64 torus_acc_add_y(u64 acc, double y) {
  const double h = __builtin_floor(y);
  const double lb = (y - h) + 0x1p20;
  const double hb = h + (0x1.8p52 - 1093664768.0);  // 1.5 * 2^52 - 0x41300000
  return add_hi_word(acc, hb) + (u64)__double_as_longlong(lb);
}

// the update for any |x| < 2^115 (N = 2048 with 23-bit digits reaches |x| ~ 2^91, beyond the magic-number step for the
// high word above), x = y * 2^32, given y: the N = 2048 keys' spectra carry the factor 2^-32 (convert_bsk_f2k
// scales by 2^-42 instead of 2^-10) and every later step -- the MAC's fmas, the inverse transform's adds, multiplies and
// fmas -- rounds a power-of-two multiple of its exact value, so y is x * 2^-32 bit for bit.  Then h = floor(y) directly,
// and y - h = 2^-32 RN(x - 2^32 h) (the same scaling argument), so (y - h) + 2^20 = 2^-32 RN(l + 2^52): the same low
// word as l + 2^52 above (ulp 2^-32 at 2^20), the high word 0x41300000 instead of 0x43300000 (hb's constant compensates), one
// f64 operation (the x * 2^-32) fewer per coefficient.  The oracle keeps the x form.
// The high word: h is an integer, so fract(h 2^-32) = (h mod 2^32) 2^-32 exactly (granularity 2^-32, any sign), and
// fract + 2^20 carries h mod 2^32 in its low word; the two 0x41300000 high words cost one v_add3_u32 operand.
// Six f64 operations per coefficient against eight.
__device__ __forceinline__ u64 torus_acc_add_wide_y(u64 acc, double y) {
  const double h = __builtin_floor(y);
  const double lb = (y - h) + 0x1p20;
  const double hb = __builtin_amdgcn_fract(h * 0x1p-32) + 0x1p20;
  const u32x2v a = __builtin_bit_cast(u32x2v, acc);
  const u32x2v w = __builtin_bit_cast(u32x2v, hb);
  return __builtin_bit_cast(u64, (u32x2v){a.x, a.y + w.x - 0x41300000u}) + (u64)__double_as_longlong(lb);
}

}  // namespace fftk

// cos / sin (2 pi t / m): fixed series in plain double, octant-reduced (the oracle's or_fft_twiddle)
void fft_twiddle(uint32_t t, uint32_t m, double* c, double* s);

}  // namespace tfhe
