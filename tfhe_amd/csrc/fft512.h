// fft512.h — the 512-point complex DFT building blocks of the FFT64 engine (gfx950), shared by the
// N = 1024 kernels (pbs_fft.hip: one wave per polynomial) and the N = 2048 kernels (pbs_fft2k.hip: two
// waves per polynomial, each running one 512-point half).  One fixed f64 operation sequence, restated
// in oracle/fft_oracle.c; contraction stays off in every file that includes this header.
#pragma once
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <type_traits>

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
// In pieces (round 11), so that the pair kernel's transposes can take the last stage output by output (dft8_xpose_p
// below); dft8 itself runs the pieces in the order it always had.
template <bool INV>
struct Dft8 {
  double yr[4], yi[4], tr[4], ti[4];                  // stage 1: y_j = x_j + x_(j+4), t_j = x_j - x_(j+4)
  double ar, ai, cr, ci;                              // u5 = (ar, ai), u7 = (cr, ci), unscaled
  double z5r, z5i, z7r, z7i, z4r, z4i, z6r, z6i;      // z5 / s, z7 / s (before its rotation by +-i), z4, z6
  double e0r, e0i, e1r, e1i, e2r, e2i, e3r, e3i;      // even half after stage 2 (e3 rotated)

  __device__ __forceinline__ void stage1(const double (&xr)[8], const double (&xi)[8]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      yr[j] = xr[j] + xr[j + 4];
      yi[j] = xi[j] + xi[j + 4];
    }
    // odd half: y4 = t0, y6 = (+-i) t2, y5 / y7 = s u5 / s u7 (u5, u7 kept unscaled)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      tr[j] = xr[j] - xr[j + 4];
      ti[j] = xi[j] - xi[j + 4];
    }
  }
  __device__ __forceinline__ void odd_u() {
    if (!INV) {
      ar = tr[1] - ti[1]; ai = tr[1] + ti[1];        // w8^1 / s
      cr = -(tr[3] + ti[3]); ci = tr[3] - ti[3];     // w8^3 / s
    } else {
      ar = tr[1] + ti[1]; ai = ti[1] - tr[1];
      cr = ti[3] - tr[3]; ci = -(tr[3] + ti[3]);
    }
  }
  __device__ __forceinline__ void odd_z57() {
    z5r = ar + cr; z5i = ai + ci;
    z7r = ar - cr; z7i = ai - ci;
  }
  // z4 = y4 + y6, z6 = y4 - y6 with y6 = (+-i) t2
  __device__ __forceinline__ void odd_z46() {
    z4r = INV ? tr[0] + ti[2] : tr[0] - ti[2]; z4i = INV ? ti[0] - tr[2] : ti[0] + tr[2];
    z6r = INV ? tr[0] - ti[2] : tr[0] + ti[2]; z6i = INV ? ti[0] + tr[2] : ti[0] - tr[2];
  }
  __device__ __forceinline__ void even2() {
    e0r = yr[0] + yr[2]; e0i = yi[0] + yi[2];
    e2r = yr[0] - yr[2]; e2i = yi[0] - yi[2];
    e1r = yr[1] + yr[3]; e1i = yi[1] + yi[3];
    e3r = yr[1] - yr[3]; e3i = yi[1] - yi[3];
    w8<INV, 2>(e3r, e3i);
  }
  // The last stage, one output (two instructions) at a time.  Even half: x0, x4 = e0 +- e1, x2, x6 = e2 +- e3.  Odd half
  // with s folded: x1, x5 = z4 +- s z5', x3, x7 = z6 +- r(s z7'), r = multiplication by +i (forward: r z = (-z.im, z.re))
  // / -i (inverse: r z = (z.im, -z.re))
  template <int E>
  __device__ __forceinline__ void out(double& re, double& im) const {
    if constexpr (E == 0) { re = e0r + e1r; im = e0i + e1i; }
    if constexpr (E == 4) { re = e0r - e1r; im = e0i - e1i; }
    if constexpr (E == 2) { re = e2r + e3r; im = e2i + e3i; }
    if constexpr (E == 6) { re = e2r - e3r; im = e2i - e3i; }
    if constexpr (E == 1) { re = __builtin_fma(SQRT1_2, z5r, z4r); im = __builtin_fma(SQRT1_2, z5i, z4i); }
    if constexpr (E == 5) { re = __builtin_fma(-SQRT1_2, z5r, z4r); im = __builtin_fma(-SQRT1_2, z5i, z4i); }
    constexpr double S3 = INV ? SQRT1_2 : -SQRT1_2;
    if constexpr (E == 3) { re = __builtin_fma(S3, z7i, z6r); im = __builtin_fma(-S3, z7r, z6i); }
    if constexpr (E == 7) { re = __builtin_fma(-S3, z7i, z6r); im = __builtin_fma(S3, z7r, z6i); }
  }
};

template <bool INV>
__device__ __forceinline__ void dft8(double (&xr)[8], double (&xi)[8]) {
  Dft8<INV> d;
  d.stage1(xr, xi);
  d.odd_u();
  d.odd_z57();
  d.odd_z46();
  d.even2();
  d.template out<0>(xr[0], xi[0]);
  d.template out<4>(xr[4], xi[4]);
  d.template out<2>(xr[2], xi[2]);
  d.template out<6>(xr[6], xi[6]);
  d.template out<1>(xr[1], xi[1]);
  d.template out<5>(xr[5], xi[5]);
  d.template out<3>(xr[3], xi[3]);
  d.template out<7>(xr[7], xi[7]);
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
// pair kernel's, with pass A's and pass B's twiddles in registers and each transpose fused with the DFT8 in front of it and placed by hand (dft8_xpose_p below).
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

// A DFT8 and the transpose behind it as one, with the twiddles w[e] in registers and the LDS traffic placed by hand
// (rounds 7 and 11): slots E0.. of the DFT8's output times w (INV: conj w), stores at Tw[WS e], reads from Tr[RS e].  Pure
// placement of stores, loads and waits: the f64 operations, their operands and their rounding are those of dft8 and the
// plain transposes above.
//   * The DFT8's head (stage 1 and the even half's stage 2, 24 f64 instructions) is hipcc's to schedule.  Then, output by
//     output in the order the operands become final -- 0, 4, 2, 6, then 1, 5, 3, 7 -- the output's two last-stage
//     instructions, its twiddle multiply and its ds_write_b128, the order pinned; the odd half's middle (u5 / u7, z5 / z7,
//     z4 / z6: 4 f64 each) sits between the even half's stores.  Consecutive stores are 10, 10, 10, 6, 6, 6, 6 f64
//     instructions apart.  A ds_write_b128 occupies the LDS pipe for ~14 cycles per wave-instruction and the four waves
//     of a workgroup reach their transposes together; round 7's form (the whole DFT8, then per slot the multiply and the
//     store: 4 f64, ~20 cycles, apart) backed the train up at issue, and the reads behind it.  hipcc's own schedule is
//     all eight multiplies, a full drain, then eight stores back to back.
//   * No s_waitcnt between the stores and the reads of the same private area (DS operations of one wave execute in issue
//     order; the ordering left is compiler-only), the eight reads pinned as ONE group in the order the next DFT8's first
//     stage consumes them (0, 4, 1, 5, 2, 6, 3, 7) and consumed under hipcc's counted lgkmcnt waits.  (A compiler-only
//     fence in lds_order lost because it left the reads free to scatter.)
// Measured on MI355X, interleaved rounds on one box per run, ms per 4096-PBS blind rotation.  Round 7
// (profiles/r07b_ab_steps.txt): the pinned per-slot stores and the undrained pinned reads pay only TOGETHER,
// 22.73 -> 22.61.  Round 11 (profiles/r11_ab_dft8_stores.txt): the stores fed from the last stage, 21.70 -> 21.17
// (-2.4 %), 22.36 -> 22.13, 21.81 -> 21.46 and, the final tree, 21.94 -> 21.38 in four runs.  Measured on top and not kept
// (tools/ab_patches/r11_store_steps.patch): consecutive stores from alternating register quadruples (+0.01), the
// inverse's eight pass-B' twiddle reads pinned as one group in store order (+0.03; round 7's
// tools/ab_patches/r07_twi_group.patch lost too), the accumulator update fed from the inverse's last DFT8 the same way
// (+0.07).
template <bool INV, int E0, int WS, int RS>
__device__ __forceinline__ void dft8_xpose_p(double (&xr)[8], double (&xi)[8], const double2 (&w)[8], double2* Tw,
                                             const double2* Tr) {
  Dft8<INV> d;
  d.stage1(xr, xi);
  d.even2();
  auto put = [&](auto ec) {
    constexpr int e = decltype(ec)::value;
    double re, im;
    d.template out<e>(re, im);
    if (e >= E0) cmul<INV>(re, im, w[e]);
    Tw[WS * e] = make_double2(re, im);
    __builtin_amdgcn_sched_barrier(0);
  };
  put(std::integral_constant<int, 0>{});
  d.odd_u();
  put(std::integral_constant<int, 4>{});
  d.odd_z57();
  put(std::integral_constant<int, 2>{});
  d.odd_z46();
  put(std::integral_constant<int, 6>{});
  put(std::integral_constant<int, 1>{});
  put(std::integral_constant<int, 5>{});
  put(std::integral_constant<int, 3>{});
  put(std::integral_constant<int, 7>{});
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

// the twist and passes A and B ride in the two fused transposes; wb[0] is unused
__device__ __forceinline__ void dft512_fwd_rab_p(double (&xr)[8], double (&xi)[8], double2* T, int lane, TBase tb,
                                                 const double2 (&wa)[8], const double2 (&wb)[8]) {
  twist_slots<false>(xr, xi);
  dft8_xpose_p<false, 0, S1, 8>(xr, xi, wa, T + lane, T + tb.b1);
  dft8_xpose_p<false, 1, S2, 1>(xr, xi, wb, T + lane, T + tb.b2);
  dft8<false>(xr, xi);
}

// pass C' from wb, pass B' from the LDS table twI
__device__ __forceinline__ void dft512_inv_rb_p(double (&xr)[8], double (&xi)[8], double2* T, int lane, TBase tb,
                                                const double2 (&wb)[8], const double2* twI) {
  dft8_xpose_p<true, 1, 1, S2>(xr, xi, wb, T + tb.b2, T + lane);
  double2 wi[8];  // pass B' twiddles: a constant LDS table, read where hipcc places them (in the DFT8's head)
#pragma unroll
  for (int e = 0; e < 8; e++) wi[e] = twI[64 * e + lane];
  dft8_xpose_p<true, 0, 8, S1>(xr, xi, wi, T + tb.b1, T + lane);
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
