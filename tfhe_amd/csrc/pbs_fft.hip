// pbs_fft.hip — the FFT64 transform of the PBS hot path for gfx950 (P-GATE shape: N = 1024, k = 1,
// PBS 2^7 x 3): the external product computed the way tfhe-rs computes it, with an f64 negacyclic
// FFT over the native 2^64 torus, instead of the Goldilocks NTT of pbs_kernels.hip.
//
// Why: MI355X runs f64 add / mul / fma at the full VALU rate (~6 cycles per wave-instruction, the
// same as a 32-bit integer op, tools/microbench/f64_rates.hip), and a complex radix-2 butterfly is ~8
// such instructions where a Goldilocks butterfly is ~30 integer ones.  Same BSK bytes (N/2 complex
// doubles = N u64 per polynomial); the batch kernel walks the CMUX loop with 4 ciphertexts x 2 component
// waves per workgroup in lockstep, the BSK level steps streamed once per workgroup into LDS by
// global_load_lds, double-buffered.
//
// Arithmetic (one fixed f64 operation sequence, restated in oracle/fft_oracle.c, which this file
// reproduces bit-for-bit — every product is written as an explicit fma or a lone multiply, and
// contraction is off for the whole file):
//   fold + twist  z_j = (a_j + i a_{j+512}) * zeta^j,   zeta = e^{i pi / 1024}
//   DFT           Z_k = sum_j z_j e^{+2 pi i jk / 512}: 3 radix-8 passes over the wave's 64 lanes
//                 x 8 registers, natural order in, DEVICE ORDER out (slot e of lane L holds
//                 k = (L >> 3) + 8 (L & 7) + 64 e); the inverse runs the passes reversed (DIT), device
//                 order in, natural order out.  Two LDS transposes each way with plain padded rows
//                 (strides 72 and 65 complex): every ds_write_b128 / ds_read_b128 is conflict-free and
//                 every address is a per-lane base plus an immediate offset
//   MAC           O_j += D_(c,l) (.) BSK_i[(c,l)][j], 4 fma per complex; c ascending, levels least
//                 significant first (each level's digits come off a running carry state, so the device
//                 BSK stores the level rows of each component reversed)
//   inverse       conjugate passes, untwist by conj(zeta^j), rint, mod 2^64, add to the accumulator
// Coefficient 64 e + L of a u64 register polynomial (slot e of lane L, e < 16) meets coefficient
// 64 (e + 8) + L in the same lane, so folding and unfolding move no data.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <type_traits>

#include "fft512.h"
#include "gl64.h"
#include "ntt1024.h"
#include "pbs_kernels.h"

namespace tfhe {
namespace fftk {

// forward transform of a real polynomial held as 16 doubles per lane (slot e <-> coefficient 64 e + L)
// (twist: slot constants here, the lane part inside pass A — fft512.h, "N = 1024 merged twist")
__device__ __forceinline__ void fft_fwd_real(const double (&a)[16], double (&xr)[8], double (&xi)[8], double2* T,
                                             int lane, const double2* tw) {
#pragma unroll
  for (int e = 0; e < 8; e++) {
    xr[e] = a[e];
    xi[e] = a[e + 8];
  }
  dft512_fwd(xr, xi, T, lane, TBase(lane), tw);  // the slot twist inside pass A (twist_dft8_fwd)
}

// inverse transform (no 1/M) + untwist: slot e -> coefficient 64 e + L (re), 64 (e + 8) + L (im)
__device__ __forceinline__ void fft_inv_real(double (&xr)[8], double (&xi)[8], double2* T, int lane, TBase tb,
                                             const double2* tw) {
  dft512_inv(xr, xi, T, lane, tb, tw);
  twist_slots<true>(xr, xi);  // the lane part of the untwist rode in pass B''s table
}

__device__ __forceinline__ int ms2048(u64 x) { return (int)((((x >> 52) + 1) >> 1) & 2047u); }

// tfhe-rs SignedDecomposer 2^7 x 3 (closest_representable at 21 bits, balanced digits, carry
// rule carry = (((res - 1) | state) & res) >> 6), restated as one step per level, least significant
// first, on the running state st (21 bits to start; == or_decompose for every state, tests/test_fft.py):
//   b = bit 13 of st (level 2 and 1; 0 for the top level), W = st + 63 + b,
//   digit = (W & 127) - 63 - b, st' = W >> 7
__device__ __forceinline__ u32 decomp_state(u64 x) { return ((u32)(x >> 32) + 1024u) >> 11; }
// bmask = 1 below the top level, 0 at the top level
// (W & 127) - 63 - b = st - (W & ~127): the digit is the old state minus the new one shifted back
// The digit as st - 128 st' in one v_mad_i32_i24 (st < 2^22, st' < 2^15 fit the 24-bit operands): 4 VALU per digit
// instead of the 5 of st - (W & ~127) (round 5; hipcc turns the multiply into a shift + subtract, hence the asm; -128 is
// not a VOP3 inline constant on gfx9, so it rides in an SGPR)
__device__ __forceinline__ int decomp_step(u32& st, u32 bmask) {
  const u32 b = __builtin_amdgcn_ubfe(st, 13, bmask);
  const u32 W = st + 63u + b;
  const u32 stn = W >> 7;
  int d;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "v"(stn), "s"(-128), "v"(st));
  st = stn;
  return d;
}
// decomp_state of the complement: for S = ~x the high word is h = ~hi(x), and ~h + 1024 = 1023 - h (mod 2^32)
__device__ __forceinline__ u32 decomp_state_not(u64 S) { return (1023u - (u32)(S >> 32)) >> 11; }
// the top level (b = 0, no next state), as a double: 2 integer VALU per digit.  A top state is 0 <= st <= 128, and there
// st - ((st + 63) & ~127) = -sext7(-st) (every st checked in tests/test_pair_int_forms.py): v_sub_u32, v_bfe_i32, the
// conversion, and a negation that rides in the source modifiers of the f64 consumers.  (In inline asm: hipcc's known-bits
// have mis-folded an sbfe builtin in rotation_states below.)  The one difference from (double)(int) is a zero digit, -0.0
// here: it can change only the sign of exact zeros downstream (mac_first's argument: a sum or an fma with a non-zero
// term does not see the sign of a zero term, products and sums of zeros stay zeros), and the accumulator update
// (torus_acc_add_y) takes floor(y), y - floor(y) and the words of both plus non-zero magic numbers, which are the same
// for y = -0.0 and +0.0
__device__ __forceinline__ double decomp_top(u32 st) {
  int t;
  asm("v_bfe_i32 %0, %1, 0, 7" : "=v"(t) : "v"(0u - st));
  return -(double)t;
}

// o = D (.) K as the first term of an fma chain: a multiply where the chain would add to +0 (the oracle's
// first term; the two differ only in the sign of an exact zero, which no later step can turn into a non-zero)
__device__ __forceinline__ void mac_first(double& re, double& im, double dr, double di, double2 k) {
  re = dr * k.x;
  re = __builtin_fma(-di, k.y, re);
  im = dr * k.y;
  im = __builtin_fma(di, k.x, im);
}
__device__ __forceinline__ void mac_next(double& re, double& im, double dr, double di, double2 k) {
  re = __builtin_fma(dr, k.x, re);
  re = __builtin_fma(-di, k.y, re);
  im = __builtin_fma(dr, k.y, im);
  im = __builtin_fma(di, k.x, im);
}

// ---------------------------------------------------------------------------------------------
// BSK conversion: one wavefront per polynomial; [i][r][j] order kept, 512 complex natural, x 2^-41 (2^-9 for the
// transform's scale, 2^-32 so that the blind rotations update their accumulators from y = x 2^-32, fft512.h
// torus_acc_add_y; round 5)
constexpr double BSK_SCALE = 0x1p-41;
__global__ __launch_bounds__(64) void bsk_to_fourier_kernel(const u64* __restrict__ bsk_std,
                                                            double2* __restrict__ bsk_f,
                                                            const double2* __restrict__ tw) {
  __shared__ __attribute__((aligned(16))) double2 T[T_C64];
  const int lane = threadIdx.x;
  const size_t q = blockIdx.x;  // standard layout [i][c*3 + l][j]
  const u64* src = bsk_std + q * N1K;
  double a[16], xr[8], xi[8];
#pragma unroll
  for (int e = 0; e < 16; e++) a[e] = i64_to_f64(src[64 * e + lane]);
  fft_fwd_real(a, xr, xi, T, lane, tw);
  const size_t j = q % 2, r = (q / 2) % 6, i = q / 12;  // device layout [i][c*3 + (2 - l)][j]
  double2* dst = bsk_f + ((i * 6 + (r / 3) * 3 + (2 - r % 3)) * 2 + j) * M;
#pragma unroll
  for (int e = 0; e < 8; e++) dst[64 * e + lane] = make_double2(xr[e] * BSK_SCALE, xi[e] * BSK_SCALE);
}

// natural-order transforms for the parity tests (one wavefront per polynomial)
__global__ __launch_bounds__(64) void fft_fwd_kernel(const u64* __restrict__ in, double2* __restrict__ out,
                                                     const double2* __restrict__ tw) {
  __shared__ __attribute__((aligned(16))) double2 T[T_C64];
  const int lane = threadIdx.x;
  const u64* src = in + (size_t)blockIdx.x * N1K;
  double a[16], xr[8], xi[8];
#pragma unroll
  for (int e = 0; e < 16; e++) a[e] = i64_to_f64(src[64 * e + lane]);
  fft_fwd_real(a, xr, xi, T, lane, tw);
  double2* dst = out + (size_t)blockIdx.x * M;
#pragma unroll
  for (int e = 0; e < 8; e++) dst[64 * e + lane] = make_double2(xr[e], xi[e]);
}

__global__ __launch_bounds__(64) void fft_inv_kernel(const double2* __restrict__ in, double* __restrict__ out,
                                                     const double2* __restrict__ tw) {
  __shared__ __attribute__((aligned(16))) double2 T[T_C64];
  const int lane = threadIdx.x;
  const double2* src = in + (size_t)blockIdx.x * M;
  double xr[8], xi[8];
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const double2 v = src[64 * e + lane];
    xr[e] = v.x;
    xi[e] = v.y;
  }
  fft_inv_real(xr, xi, T, lane, TBase(lane), tw);
  double* dst = out + (size_t)blockIdx.x * N1K;
#pragma unroll
  for (int e = 0; e < 8; e++) {
    dst[64 * e + lane] = xr[e];
    dst[64 * (e + 8) + lane] = xi[e];
  }
}

// ---------------------------------------------------------------------------------------------
// The waves' base priority (what each level step drops back to after its MAC phase): the workgroups of the odd dispatch
// half-rounds -- on 256 CUs bit 8 of blockIdx: the second workgroup each CU receives, then every other half-round -- run at
// base priority 1.  The hardware arbitrates oldest-first, so of the two workgroups that share a CU the older always ran
// ahead: in a 4096 launch one slot of every CU finished its four workgroups 2.4 ms before the other and idled
// (profiles/r06d_wgt_4096.json, per-workgroup s_memrealtime stamps, tools/wg_timeline.py).  With the alternation the two
// slots end 0.33 ms apart and the CU-slot busy fraction rises 0.945 -> 0.980: 24.04 -> 23.04 ms per 4096, C2 6.45 -> 6.24
// ms (same box, three boxes; profiles/r06e_ab_prio.txt).  Round 4 had measured this scheme "neutral" -- with a
// C-level branch around s_setprio that made hipcc spill (base_prio below).
// The dispatch half-round of a workgroup on a part with `cus` compute units and two workgroups per CU: 0 = the first
// workgroup each CU receives, 1 = the second, 2, 3 = the next round's.  The base priority raises the odd half-rounds,
// the start-up stagger delays half-round 1.  One division per workgroup, outside the CMUX loop.
constexpr unsigned dispatch_half(unsigned wg, unsigned cus) { return wg / cus; }
constexpr bool wg_prio_hi(unsigned wg, unsigned cus) { return dispatch_half(wg, cus) & 1u; }
constexpr bool wg_staggered(unsigned wg, unsigned cus) { return dispatch_half(wg, cus) == 1u; }
namespace dh_check {
// on 256 CUs (MI355X): exactly rounds 1 to 6's bit 8 of the workgroup index and the range [256, 512)
constexpr bool same_as_bit8(unsigned n) {
  for (unsigned w = 0; w < n; w++)
    if (wg_prio_hi(w, 256) != (((w >> 8) & 1u) != 0) || wg_staggered(w, 256) != (w < 512 && ((w >> 8) & 1u))) return false;
  return true;
}
static_assert(same_as_bit8(4096), "dispatch_half(., 256) must reproduce the 256-CU split");
static_assert(!wg_prio_hi(31, 32) && wg_prio_hi(32, 32) && wg_prio_hi(63, 32) && !wg_prio_hi(64, 32) && wg_prio_hi(96, 32), "32 CUs");
static_assert(!wg_staggered(31, 32) && wg_staggered(32, 32) && wg_staggered(63, 32) && !wg_staggered(64, 32) && !wg_staggered(96, 32), "32 CUs");
static_assert(!wg_prio_hi(303, 304) && wg_prio_hi(304, 304) && wg_prio_hi(607, 304) && !wg_prio_hi(608, 304) && wg_prio_hi(912, 304), "304 CUs");
static_assert(!wg_staggered(303, 304) && wg_staggered(304, 304) && wg_staggered(607, 304) && !wg_staggered(608, 304) && !wg_staggered(912, 304), "304 CUs");
}  // namespace dh_check

// Component-pair batch kernel (round 3, the default above the latency range): workgroup = CTS ciphertexts x 2
// waves, wave (p, c) owns COMPONENT c of ciphertext p.  Per CMUX i:
//   rotate + decompose acc_c (wave-local: the wave's own transpose area holds the rotation image)
//   level steps q = 0, 1, 2 (least significant first): digits -> twist -> DFT -> MAC into BOTH outputs'
//     partial sums  O_j^c = fma chain over q of D_(c,q) (.) BSK_i[(c, q)][j]      (j = 0, 1)
//     q = 1, 2: one step's chunk = rows (0, q) and (1, q) of BSK_i (32 KB), streamed once per workgroup by LDS DMA
//     into one buffer (q = 1's issued behind step 0's MAC, q = 2's at its step's start); q = 0: the wave's own two
//     rows (c, 0) straight from L2 into registers, no LDS and no barrier (round 12, load_step0_keys)
//   exchange: wave c publishes O_(1-c)^c in its transpose area and takes O_c^(1-c) from its partner's:
//     O_c = O_c^c + O_c^(1-c)  (= O_c^0 + O_c^1: f64 addition commutes, the oracle's split order)
//   ONE inverse transform: acc_c += rint(iFFT(O_c)) mod 2^64
// Against round 2's 8-ciphertext kernel (one wave per ciphertext, retired in round 4): the same transforms per
// ciphertext, half of them per wave, 1/2 the accumulator / partial-sum registers per wave, and twice the waves
// per ciphertext -- a batch of 1024 fills all 256 CUs at 2 waves / SIMD.
// The MAC order (per-component chains, then one add) is restated in oracle/fft_oracle.c.
constexpr int STEP_C64 = 4 * M;                    // rows (0, q), (1, q), j = 0, 1
// CTS = ciphertexts per workgroup, 2 since round 4: 4 waves, TWO independent workgroups per CU (76 KB of LDS each: the
// inverse's TW_I table 8 KB | one 32 KB chunk, level steps 1 and 2 in turn | 4 x 9 KB transpose areas; passes A / B come
// from registers, and so do level step 0's key words since round 12), so the
// two workgroups drift apart and one's LDS phases overlap the other's VALU phases on every SIMD: 27.01 -> 26.63 ms per
// 4096 on the same box against round 3's 8 waves with all tables in LDS and double-buffered level steps
// (profiles/r04a_cts_ab.txt, two rounds).  Holding pass A's and pass B's twiddles in registers across the CMUX loop is
// the round-2 ablation's -4 %.
template <int CTS>
struct FpShared {
  double2 twI[M];                                  // TW_I only (passes A, B: registers, loaded from global)
  double2 K[1][STEP_C64];
  double2 T[2 * CTS][T_C64];
};
typedef __attribute__((address_space(3))) u64 lds_u64;

// (X^a v - v), v = this wave's polynomial (slot e <-> coefficient 64 e + L), to decomposition states.  The rotation
// image is the wave's transpose area, and the rotation is split so that every per-slot decision is wave-uniform (round 5).
// a (uniform) = 1024 s + 64 A + r.  The image written is W = X^r v (lane part: each lane writes at +r, only slot 15
// of the lanes L + r >= 64 wraps, negated, to the image start); the reads take (X^(64 A) W)[L + 64 e] = W[L + 64 (e -
// A)] for e >= A and -W[L + 64 (e - A + 16)] for e < A, so slot e's base (two per-lane bases 8 KB apart) and sign
// (xor s) depend only on the SGPR comparison e < A.  Per slot 8 VALU instead of the 10 of a per-lane compare and
// negate-and-select (y = (x ^ M) - (v + M), M = 0 or all ones); the values are the same, so no operation order changes.
// Since round 8 the difference is taken as the complement of a sum, 7 VALU per slot (below).
// In two halves since round 10 (one function, rotate_states, until then): the image stores
// (rotation_store_pair) and the reads with the differences (rotation_states).  The stores of CMUX i + 1's image go out slot pair by slot pair under the accumulator update of
// CMUX i, whose amount a is an SGPR from level step 0 of CMUX i on; as one group behind the update they were a burst of
// nine DS stores and a full drain at every CMUX's head with the wave issuing nothing else.
// The write base of the image for the amount a: word L + r of the area; w15 = this lane's slot 15 wraps.  Slots 0..14
// end at word 63 + 63 + 896 = 1022 and slot 15 lands at L + r + 960 <= 1023 or wraps to L + r - 64 >= 0: inside the
// area's 1152 words for every a, also for an amount nobody rotates by (the body word's, behind the last CMUX)
struct RotW {
  u32 wb;
  bool w15;
  __device__ __forceinline__ RotW(int a, int lane, double2* T)
      : wb((u32)(uintptr_t)(lds_u64*)&((u64*)T)[lane + (a & 63)]), w15(lane + (a & 63) >= 64) {}
};
// slots E and E + 1 of the image (two words 512 B apart: one ds_write2st64_b64); slot 15 keeps its per-lane wrap
// (coefficient 960 + L + r >= 1024: to L + r - 64, negated)
template <int E>
__device__ __forceinline__ void rotation_store_pair(u64 v0, u64 v1, RotW w) {
  ((lds_u64*)(uintptr_t)w.wb)[64 * E] = v0;
  if constexpr (E < 14) {
    ((lds_u64*)(uintptr_t)w.wb)[64 * (E + 1)] = v1;
  } else {
    const u32 a15 = w.w15 ? w.wb + 960u * 8u - 8192u : w.wb + 960u * 8u;
    *(lds_u64*)(uintptr_t)a15 = w.w15 ? 0 - v1 : v1;
  }
}
// the whole image at once (the prologue: CMUX 0's)
__device__ __forceinline__ void rotation_store(const u64 (&v)[16], int a, int lane, double2* T) {
  const RotW w(a, lane, T);
  rotation_store_pair<0>(v[0], v[1], w);
  rotation_store_pair<2>(v[2], v[3], w);
  rotation_store_pair<4>(v[4], v[5], w);
  rotation_store_pair<6>(v[6], v[7], w);
  rotation_store_pair<8>(v[8], v[9], w);
  rotation_store_pair<10>(v[10], v[11], w);
  rotation_store_pair<12>(v[12], v[13], w);
  rotation_store_pair<14>(v[14], v[15], w);
}
// The reads of the image stored for the amount a (uniform: an SGPR), the differences and the states.  No drain between
// the wave's own stores and these reads (DS operations of one wave execute in issue order): a compiler-level fence, and
// the sixteen reads pinned as one group and consumed under counted waits, as dft8_xpose_p's are
__device__ __forceinline__ void rotation_states(const u64 (&v)[16], int a, int lane, double2* T, u32 (&st)[16]) {
  u64* Tu = (u64*)T;
  const int A = (a >> 6) & 15;
  const bool sgn = a >= 1024;
  const u32 rb = (u32)(uintptr_t)(lds_u64*)&Tu[lane] - 512u * (u32)A;  // >= T - 7.5 KB: inside the block
  // bit e of wmask: slot e reads the wrapped part (e < A); bit e of mbits: slot e negated.  Bit-field extracts of
  // these SGPR words keep every per-slot decision scalar (a compare would be rebuilt as a per-lane select)
  const u32 wmask = (1u << A) - 1u;
  const u64 mbits = (u32)__builtin_amdgcn_readfirstlane(wmask ^ (sgn ? ~0u : 0u));
  u64 x[16];
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int e = 0; e < 16; e++)
    x[e] = ((const lds_u64*)(uintptr_t)(rb + (__builtin_amdgcn_ubfe(wmask, e, 1) << 13)))[64 * e];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int e = 0; e < 16; e++) {
    // s_bfe_i64 (0 or all ones, both words in ONE scalar instruction) in inline asm: hipcc's known-bits treat the
    // width-1 sbfe builtin as non-negative and drop the sign extension (a probe kernel stores hi = 0 for it).  The
    // scalar instructions of this loop are not free: the form with a separate ~M (an s_bfe_i32 and an s_ashr_i32 for
    // each mask, 32 more scalar instructions per CMUX) ran 0.16 ms per 4096 SLOWER than the subtracting code it
    // replaced, this one 0.19 ms faster
    u64 M;
    asm("s_bfe_i64 %0, %1, %2" : "=s"(M) : "s"(mbits), "i"(e | (1 << 16)));
    // (x ^ M) - (v + M) = ~((x ^ ~M) + (v + M)), exact in all 64 bits (-(x ^ ~M) = (x ^ M) + 1): two 64-bit adds (one
    // v_lshl_add_u64 each) instead of an add and a two-instruction subtract; the complement folds into the state.
    // x ^ ~M = ~(x ^ M) is one v_xnor_b32 per word
    st[e] = decomp_state_not(~(x[e] ^ M) + (v[e] + M));
  }
  lds_order();
}

// the partial-sum exchange of wave c (compile-time): publish O_(1-c)^c in this wave's area, add O_c^(1-c) from
// the partner's (two workgroup barriers)
// The eight reads of the partner's area are pinned as one group (round 7: the published half of the partial sums has
// just died, so their registers are free) and added under counted waits; hipcc's own schedule for C = 1 reads two, waits,
// adds, four times over
template <int C>
__device__ __forceinline__ void exchange_partials(const double (&o0r)[8], const double (&o0i)[8], const double (&o1r)[8],
                                                  const double (&o1i)[8], double (&xr)[8], double (&xi)[8], double2* T,
                                                  const double2* Tp, int lane) {
#pragma unroll
  for (int e = 0; e < 8; e++) {
    T[64 * e + lane] = C ? make_double2(o0r[e], o0i[e]) : make_double2(o1r[e], o1i[e]);
    xr[e] = C ? o1r[e] : o0r[e];
    xi[e] = C ? o1i[e] : o0i[e];
  }
  __syncthreads();
  double2 w[8];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int e = 0; e < 8; e++) w[e] = Tp[64 * e + lane];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int e = 0; e < 8; e++) {
    xr[e] = xr[e] + w[e].x;
    xi[e] = xi[e] + w[e].y;
  }
  __syncthreads();  // the partner has read this wave's area before the inverse overwrites it
}

// Level step g = 3 i + q, q = 1 or 2 (step 0 uses no chunk: load_step0_keys): 32 KB in 1 KB blocks; wave w of NW loads
// blocks (32 / NW) w .. (16 per component row) through buffer_load_dwordx4 ... lds with the BSK as a buffer resource:
// the per-load byte offset is an SGPR (soffset) and the lane offset one VGPR, so the 16 pieces of a CMUX cost no VALU
// (round 5; global_load_lds needs a 64-bit VALU address add per load).  The wave's blocks go in groups of four
// consecutive ones (NW = 4: one component row, 8 KB in a row, in the BSK and in the chunk), pieces 1..3 of a group on
// the instruction's immediate offset, which advances the buffer address AND the LDS address: two M0 values and two
// soffsets per wave and level step instead of eight of each (round 9).  Measured and not shipped: the
// level-step buffer as a __shared__ object of its own and its pieces issued from asm statements that hipcc's wait
// bookkeeping does not see (tools/ab_patches/r09_k_own_dma_asm.patch); the pieces of level steps 0 and 2 issued one
// per iteration of the digit loop (tools/ab_patches/r09_dma_spread.patch, round 9: step 0 had a chunk then).
template <int NW>
__device__ __forceinline__ void load_step_buf4(__amdgpu_buffer_rsrc_t bsr, int g, double2* dst, int wave_s, int voff) {
  static_assert((32 / NW) % 4 == 0 && 16 % (32 / NW) == 0, "groups of four blocks inside one component row");
  const int i = g / 3, q = g - 3 * (g / 3);
#pragma unroll
  for (int h = 0; h < 32 / NW; h += 4) {
    const int blk = wave_s * (32 / NW) + h;
    const int c = blk >> 4;
    const int soff = ((i * 6 + c * 3 + q) * (2 * M)) * (int)sizeof(double2) + (blk & 15) * 1024;  // < 2^31: BSK < 2 GB
    auto* ld = (__attribute__((address_space(3))) void*)((char*)dst + blk * 1024);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(bsr, ld, 16, voff, soff, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(bsr, ld, 16, voff, soff, 1024, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(bsr, ld, 16, voff, soff, 2048, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(bsr, ld, 16, voff, soff, 3072, 0);
  }
}

// Level step 0 takes its key words from L2 into registers, not through the chunk (round 12): wave (p, c)
// needs only rows (c, 0, j = 0, 1) of BSK_i, 16 KB contiguous in the device layout, and the 64 VGPRs of the partial sums
// are free until that step's MAC, which turns each key word into the partial sum that takes its registers.  Slots
// E0 .. E1 - 1 as buffer_load_dwordx4 into registers: the row offset in SGPRs (one per 4 KB), the lane offset the loop's
// voff, the slot on the immediate offset; no VALU.  The rows end at byte (6 i + 3 c + 1) 16 KB <= 6 n 16 KB, the
// buffer's num_records.  Slot e's two words go out together, in the order the MAC consumes them under counted vmcnt
// waits (vector loads return in order).  The two waves of a workgroup with the same c fetch the same 16 KB: key bytes
// from L2 / L1 per workgroup and CMUX 96 -> 128 KB.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <int E0, int E1>
__device__ __forceinline__ void load_step0_keys(__amdgpu_buffer_rsrc_t bsr, int i, int c_s, int voff, double2 (&ku)[8],
                                                double2 (&kv)[8]) {
  const int soff = ((i * 6 + c_s * 3) * (2 * M)) * (int)sizeof(double2);  // < 2^31: BSK < 2 GB
#pragma unroll
  for (int e = E0; e < E1; e++) {
    const int so = soff + (e >> 2) * 4096, vo = voff + (e & 3) * 1024;
    ku[e] = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(bsr, vo, so, 0));
    kv[e] = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(bsr, vo, so + M * (int)sizeof(double2), 0));
  }
}

#ifndef FFT_DMASTAMP
#define FFT_DMASTAMP 0
#endif
#if FFT_DMASTAMP
// diagnostic build only (tools/dma_stamps.py): shader-clock cycles (s_memtime) a wave spends issuing the eight pieces of
// a level step, summed over the CMUX loop per site q = 0, 1, 2; [3] = the whole loop.  Workgroups 0..63 x wave.  The
// stamps pin the pieces at the step's start (a sched_barrier on either side).
__device__ unsigned long long g_dmast[64 * 4 * 4];
#endif

#ifndef FFT_WGTIME
#define FFT_WGTIME 0
#endif
#if FFT_WGTIME
// diagnostic build only: per-workgroup start / end (s_memrealtime, 100 MHz), HW_ID and XCC_ID of the last launch
__device__ unsigned long long g_wgt[4 * 16384];
#endif
template <int CTS, bool WRITE_ACC, bool WRITE_BIG>
__global__ __launch_bounds__(128 * CTS, 4 / CTS) void blind_rotate_fft_pair_kernel(
    const u64* __restrict__ lwe_in, int n, size_t B, const u64* __restrict__ luts, const u32* __restrict__ lut_index,
    int n_lut, const double2* __restrict__ bsk, const double2* __restrict__ tw_g, u64* __restrict__ out_big,
    u64* __restrict__ out_acc, int n_cus) {
  constexpr int NW = 2 * CTS;
  __shared__ __attribute__((aligned(16))) FpShared<CTS> sh;
#if FFT_WGTIME
  const unsigned long long wg_t0 = __builtin_amdgcn_s_memrealtime();
#endif
  const int wave = threadIdx.x >> 6;
  int lane = threadIdx.x & 63;
  const int c = wave & 1;
  const size_t b_raw = (size_t)blockIdx.x * CTS + (wave >> 1);
  const bool live = b_raw < B;
  const size_t b = live ? b_raw : B - 1;  // padding pairs run a copy of the last ciphertext, store nothing
  const u64* ct = lwe_in + b * (size_t)(n + 1);
  double2* T = sh.T[wave];
  const double2* Tp = sh.T[wave ^ 1];
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const int c_s = wave_s & 1;

  // the BSK as a raw buffer (num_records = its byte size; gfx9 dword 3 = 0x00020000, as composable_kernel uses on gfx9)
  const __amdgpu_buffer_rsrc_t bsr =
      __builtin_amdgcn_make_buffer_rsrc((void*)bsk, (short)0, n * 6 * 2 * M * (int)sizeof(double2), 0x00020000);
  int voff = lane * 16;
  for (int q = threadIdx.x; q < M; q += 64 * NW) sh.twI[q] = tw_g[TW_I + q];

  // acc_c: A = 0, B = X^{-b~} * lut (LUT values in the Z_p encoding, mapped to the torus first)
  u64 acc[16];
  {
    int li = lut_index ? (int)lut_index[b] : 0;
    li = (li < 0 || li >= n_lut) ? 0 : li;
    const u64* lut = luts + (size_t)li * N1K;
    const int s = (2048 - ms2048(ct[n])) & 2047;
#pragma unroll
    for (int e = 0; e < 16; e++) {
      int d = 64 * e + lane - s;
      bool neg = false;
      if (d < 0) { d += N1K; neg = !neg; }
      if (d < 0) { d += N1K; neg = !neg; }
      const u64 v = gl_to_torus(lut[d]);
      acc[e] = c ? (neg ? 0 - v : v) : 0;
    }
  }

  const TBase tb(lane);
  const double2* twA = tw_g + TW_A;
  const double2* twI = sh.twI;
  const double2* twB = twA + M;
  double2 wa[8];  // pass A's twiddles (twist merged) for the whole CMUX loop: 8 LDS reads fewer per transform
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 8; e++) wa[e] = twA[64 * e + lane];
  double2 wb[8];  // and pass B's (the inverse's pass C' conjugates the same table): 7 more per forward, 7 per inverse
#pragma unroll
  for (int e = 1; e < 8; e++) wb[e] = twB[64 * e + lane];
  wb[0] = make_double2(1.0, 0.0);
  // the wave's base priority, also what each level step drops back to after its MAC phase: with two workgroups per
  // CU, one of them (by dispatch half-round) at the higher priority: bit 8 of the workgroup index on a 256-CU part
  // (MI355X), the same half-rounds on any other CU count
  const bool prio_hi = wg_prio_hi(blockIdx.x, (unsigned)n_cus);
  // a runtime (wave-uniform) priority as ONE asm block with its own scalar branch: a C-level branch around the two
  // s_setprio forms splits every level step into basic blocks and hipcc then spills ~195 VGPRs (measured 71 ms)
  const unsigned prio_flag = __builtin_amdgcn_readfirstlane(prio_hi ? 1u : 0u);
  auto base_prio = [&]() {
    asm volatile(
        "s_cmp_lg_u32 %0, 0\n\ts_cbranch_scc0 .Lbp0_%=\n\ts_setprio 1\n\ts_branch .Lbp1_%=\n"
        ".Lbp0_%=:\n\ts_setprio 0\n.Lbp1_%=:" ::"s"(prio_flag) : "scc");
  };
  base_prio();
  // round 6: the second workgroup of each CU in the first dispatch round (dispatch half-round 1) starts ~3.4 us late,
  // so the two workgroups of a CU do not run their phases in lockstep from the start (on top of the base priority: 23.04
  // -> 22.97 ms per 4096, C2 6.24 -> 6.19 ms; alone 24.04 -> 23.87 ms; 2 and 4 x 3.4 us: neutral)
  if (wg_staggered(blockIdx.x, (unsigned)n_cus)) __builtin_amdgcn_s_sleep(127);
#if FFT_DMASTAMP
  unsigned long long dma_cyc[3] = {0, 0, 0};
  const unsigned long long loop_t0 = __builtin_amdgcn_s_memtime();
#endif
  // The mask word of CMUX i + 1 is loaded during CMUX i (after the rotation, ahead of level step 0's key loads) and
  // becomes the scalar ms2048 value in front of level step 0's MAC, behind a counted wait that the key words' own waits
  // follow, so no CMUX opens with a global load and a full wait (round 9; round 12, 3q).  Only the word's
  // high half is loaded (ms2048 reads bits 52..63); the row is n + 1 words long, so CMUX n - 1 prefetches the body word
  // and ignores it.
  // ms2048 from a word's high half; the high halves of the row
  auto ms2048_hi = [](u32 hi) { return (int)((((hi >> 20) + 1u) >> 1) & 2047u); };
  const u32* ct_hi = (const u32*)ct + 1;
  int a_s = __builtin_amdgcn_readfirstlane(ms2048_hi(ct_hi[0]));
  rotation_store(acc, a_s, lane, T);  // CMUX 0's image; every later one is stored under the update before it
  for (int i = 0; i < n; i++) {
    // (X^a acc_c - acc_c), decomposed: the rotation image in this wave's own transpose area (its previous
    // user, the last inverse, is this wave: DS operations of a wave run in order)
    u32 st[16];
    rotation_states(acc, a_s, lane, T, st);
    // opaque per CMUX: hipcc otherwise hoists voff + 1024, + 2048, + 3072 of the key loads into three loop-long VGPRs
    // instead of the loads' immediate offsets
    asm volatile("" : "+v"(voff));
    // the next CMUX's mask word (i = n - 1: the body word, ignored), issued ahead of level step 0's key loads and
    // consumed in front of that step's MAC
    u32 ct_next = ct_hi[2 * (size_t)(i + 1)];
    double o0r[8], o0i[8], o1r[8], o1i[8];
    // level steps q = 0, 1, 2 (least significant first), each specialised at compile time: q = 0 starts the two
    // fma chains with a multiply (no zeroed partial sums), q = 2 takes the top digit (no carry bit, no next state)
    auto level = [&](auto qc) {
      constexpr int q = decltype(qc)::value;
      const int g = 3 * i + q;
      if (q > 0) base_prio();  // the previous step's MAC ran at the top priority (below)
      // One key buffer, used by level steps 1 and 2.  Step 1's chunk is issued behind step 0's MAC with no barrier in
      // front of it: the buffer's last readers were the q = 2 MACs of CMUX i - 1 in all four waves, each of which has
      // its key words in registers (consumed by its fma) before it reaches the exchange's first barrier, and a wave
      // issues these pieces only behind the exchange's second barrier (in CMUX 0 nothing has read the buffer yet).
      // Its arrival is published by step 1's glds_barrier as before.  Step 2 overwrites what step 1's MACs read, so it
      // keeps its barrier: every wave is done with step 1's chunk.
      if (q == 1) __builtin_amdgcn_sched_barrier(0);  // no barrier opens this step: keep its work behind the priority drop
      if (q == 2) __syncthreads();
      // step 0's key words: slots 0..3 here, slots 4..7 behind the digits (sixteen loads back to back at either point,
      // or two per digit pair, measured slower: DESIGN 3q, tools/ab_patches/r12_k0_issue_points.patch)
      double2 ku0[8], kv0[8];
      if constexpr (q == 0) {
        __builtin_amdgcn_sched_barrier(0);
        load_step0_keys<0, 4>(bsr, i, c_s, voff, ku0, kv0);
        __builtin_amdgcn_sched_barrier(0);
      }
#if FFT_DMASTAMP
      __builtin_amdgcn_sched_barrier(0);
      const unsigned long long dma_t0 = __builtin_amdgcn_s_memtime();
#endif
      if (q == 2) load_step_buf4<NW>(bsr, g, sh.K[0], wave_s, voff);
#if FFT_DMASTAMP
      dma_cyc[q] += __builtin_amdgcn_s_memtime() - dma_t0;
      __builtin_amdgcn_sched_barrier(0);
#endif
      double xr[8], xi[8];
#pragma unroll
      for (int e = 0; e < 8; e++) {
        if constexpr (q == 2) {
          xr[e] = decomp_top(st[e]);
          xi[e] = decomp_top(st[e + 8]);
        } else {
          xr[e] = (double)decomp_step(st[e], 1u);
          xi[e] = (double)decomp_step(st[e + 8], 1u);
        }
      }
      if constexpr (q == 0) {
        __builtin_amdgcn_sched_barrier(0);
        load_step0_keys<4, 8>(bsr, i, c_s, voff, ku0, kv0);
        __builtin_amdgcn_sched_barrier(0);
      }
      // the slot twist rides in pass A's twisted DFT8 (twist_dft8_fwd)
      dft512_fwd_rab_p(xr, xi, T, lane, tb, wa, wb);
      // Each level step's MAC runs at the top wave priority (back to the base priority when the next step starts and
      // after the last), so the short MAC phase of one workgroup is not stalled behind the other workgroup's transforms
      // on the same SIMD: 26.62 -> 25.26 ms per 4096 on the same box, 152.2k -> 160.4k PBS/s (late round 4,
      // profiles/r04k_pgate_macprio_ab.txt)
      if constexpr (q == 0) {
        // no chunk and no barrier in this step.  The mask word went out ahead of the key loads, so the wait for it
        // (hipcc's, counted) passes before the first key word's does: from here it is the scalar a of the next CMUX
        asm volatile("" : "+v"(ct_next));
        a_s = ms2048_hi(__builtin_amdgcn_readfirstlane(ct_next));
        __builtin_amdgcn_s_setprio(3);
        // the key word and the partial sum it starts share registers: slot e's two words die in its eight instructions
#pragma unroll
        for (int e = 0; e < 8; e++) {
          mac_first(o0r[e], o0i[e], xr[e], xi[e], ku0[e]);
          mac_first(o1r[e], o1i[e], xr[e], xi[e], kv0[e]);
        }
        // no barrier ends this step: keep the MAC in it, at its priority; then step 1's chunk (above), behind the MAC's
        // waits, which hipcc would otherwise turn into vmcnt(0)
        __builtin_amdgcn_sched_barrier(0);
#if FFT_DMASTAMP
        const unsigned long long dma_t1 = __builtin_amdgcn_s_memtime();
#endif
        load_step_buf4<NW>(bsr, g + 1, sh.K[0], wave_s, voff);
#if FFT_DMASTAMP
        dma_cyc[1] += __builtin_amdgcn_s_memtime() - dma_t1;
#endif
        __builtin_amdgcn_sched_barrier(0);
        return;
      }
      glds_barrier();  // step g's chunk has landed
      __builtin_amdgcn_s_setprio(3);
      const double2* k0 = sh.K[0] + c * (2 * M) + lane;
      const double2* k1 = k0 + M;
      // The key words of level steps q = 1 and q = 2 software-pipelined (round 7): a rotating window of D slots' key
      // words ahead of the slot being consumed, the order pinned: the reads of slot e + D go out before slot e's eight
      // fma, which wait (counted) for slot e's pair only.  hipcc's own schedule reads one slot's two words into the
      // same registers eight times per level and waits for each pair (eight exposed LDS round trips per level, at the
      // MAC's raised priority and right before a workgroup barrier).  One slot ahead at q = 1 and two at q = 2 (the 16
      // decomposition states are dead there) is what 256 VGPRs hold.  Measured alone 22.90 -> 22.73 ms per 4096-PBS
      // blind rotation, and 0.29 ms of the round-7 default's gain when taken out of it (same box, three interleaved
      // rounds each, profiles/r07b_ab_steps.txt).
      constexpr int D = q == 2 ? 2 : 1;
      double2 ku[8], kv[8];
#pragma unroll
      for (int e = 0; e < D; e++) {
        ku[e] = k0[64 * e];
        kv[e] = k1[64 * e];
      }
#pragma unroll
      for (int e = 0; e < 8; e++) {
        if (e + D < 8) {
          ku[e + D] = k0[64 * (e + D)];
          kv[e + D] = k1[64 * (e + D)];
        }
        __builtin_amdgcn_sched_barrier(0);
        mac_next(o0r[e], o0i[e], xr[e], xi[e], ku[e]);
        mac_next(o1r[e], o1i[e], xr[e], xi[e], kv[e]);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    level(std::integral_constant<int, 0>{});
    level(std::integral_constant<int, 1>{});
    level(std::integral_constant<int, 2>{});
    base_prio();
    // exchange the partial sums: publish O_(1-c)^c, take O_c^(1-c) (c wave-uniform: a scalar branch, no selects)
    double xr[8], xi[8];
    if (c_s) exchange_partials<1>(o0r, o0i, o1r, o1i, xr, xi, T, Tp, lane);
    else exchange_partials<0>(o0r, o0i, o1r, o1i, xr, xi, T, Tp, lane);
    dft512_inv_rb_p(xr, xi, T, lane, tb, wb, twI);
    twist_slots<true>(xr, xi);
    {
      // the image of CMUX i + 1 (a_s is its amount since level step 0), each slot pair stored as its words become
      // final; the area's last user, the inverse's second transpose, has been read
      const RotW w(a_s, lane, T);
      auto upd = [&](auto ec) {
        constexpr int e = decltype(ec)::value;
        acc[e] = torus_acc_add_y(acc[e], e < 8 ? xr[e & 7] : xi[e & 7]);
        acc[e + 1] = torus_acc_add_y(acc[e + 1], e < 8 ? xr[(e + 1) & 7] : xi[(e + 1) & 7]);
        rotation_store_pair<e>(acc[e], acc[e + 1], w);
        __builtin_amdgcn_sched_barrier(0);
      };
      __builtin_amdgcn_sched_barrier(0);
      upd(std::integral_constant<int, 0>{});
      upd(std::integral_constant<int, 2>{});
      upd(std::integral_constant<int, 4>{});
      upd(std::integral_constant<int, 6>{});
      upd(std::integral_constant<int, 8>{});
      upd(std::integral_constant<int, 10>{});
      upd(std::integral_constant<int, 12>{});
      upd(std::integral_constant<int, 14>{});
    }
  }
#if FFT_DMASTAMP
  if (lane == 0 && blockIdx.x < 64 && wave < 4) {
    unsigned long long* o = g_dmast + (blockIdx.x * 4 + wave) * 4;
    o[0] = dma_cyc[0];
    o[1] = dma_cyc[1];
    o[2] = dma_cyc[2];
    o[3] = __builtin_amdgcn_s_memtime() - loop_t0;
  }
#endif
#if FFT_WGTIME
  if (threadIdx.x == 0 && blockIdx.x < 16384) {
    const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
    g_wgt[4 * blockIdx.x] = wg_t0;
    g_wgt[4 * blockIdx.x + 1] = t1;
    g_wgt[4 * blockIdx.x + 2] = (unsigned)__builtin_amdgcn_s_getreg(4 | (31 << 11));    // HW_ID
    g_wgt[4 * blockIdx.x + 3] = (unsigned)__builtin_amdgcn_s_getreg(20 | (31 << 11));   // XCC_ID
  }
#endif

  if (!live) return;
  // the output's row and component from wave-uniform values and the lane counted anew (mbcnt over an opaque zero, so
  // that it is not the prologue's value): hipcc otherwise keeps the prologue's per-lane b, c, L and 64 e + L alive
  // through the loop, which has no register left for them
  const size_t bo = (size_t)blockIdx.x * CTS + (size_t)(wave_s >> 1);  // = b: the wave is live
  const int co = c_s;
  {
    u32 z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
  }
  if (WRITE_ACC) {
    u64* oa = out_acc + bo * 2048 + co * N1K;
#pragma unroll
    for (int e = 0; e < 16; e++) oa[64 * e + lane] = acc[e];
  }
  if (WRITE_BIG) {
    // sample extraction at degree 0 (computations.rs:109-132): a'_0 = A[0], a'_j = -A[N-j], b' = B[0]
    u64* ob = out_big + bo * (size_t)(N1K + 1);
    if (co == 0) {
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int idx = 64 * e + lane;
        if (idx == 0) ob[0] = acc[e];
        else ob[N1K - idx] = 0 - acc[e];
      }
    } else if (lane == 0) {
      ob[N1K] = acc[0];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Latency-mode blind rotation (small batches): ONE ciphertext per workgroup of 8 waves.  Per CMUX:
//   A  waves 0..5: wave r = chain position (c, q) (c = r / 3; q = 0, 1, 2: levels least significant
//      first) rotates + decomposes accumulator polynomial c, keeps step q's digits and transforms
//      them -> F[r]                                                     (6 transforms in parallel)
//   B  all 8 waves: O_j = O_j^0 + O_j^1, O_j^c = fma chain over r = 3c .. 3c + 2 of F[r] (.) BSK_i[r][j]
//      (the oracle's split order) on 2 of the 8 slots each (j = wave >> 2); the BSK words come straight from L2, loaded into
//      registers before phase A so their latency hides behind the transforms
//   C  waves 0, 1: inverse transform of O_j, acc_j += rint mod 2^64      (2 transforms in parallel)
// Three barriers per CMUX; the critical path is 1 forward + 1 inverse transform + 1/4 of the MAC
// instead of 6 + 2 + all of it.  LDS (tables first: small DS immediates): tw 32 KB | acc 16 KB |
// F 48 KB | 6 transpose areas 54 KB (O_0, O_1 alias areas 2, 3, dead after phase A) = 150 KB.
constexpr int FL_THREADS = 512;
constexpr int FL_MAXN = 1024;  // rotation amounts staged in LDS up to this LWE dimension (global reads above)
struct FftLatShared {
  double2 tw[TW_C64];
  u64 A[2][N1K];
  double2 F[6][M];
  double2 T[6][T_C64];
  unsigned short ab[FL_MAXN];  // ms2048(ct[i]) for every CMUX
};

__device__ __forceinline__ void lat_load_key(const double2* __restrict__ bsk, int i, int j, int s0, int lane,
                                             double2 (&kv)[6][2]) {
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int t = 0; t < 2; t++) kv[r][t] = bsk[((size_t)(i * 6 + r) * 2 + j) * M + 64 * (s0 + t) + lane];
}

// The latency kernel's three barriers per CMUX wait for LDS only (s_waitcnt lgkmcnt(0) + s_barrier; round 6).  Every
// cross-wave exchange of the kernel goes through LDS; __syncthreads also drains vmcnt, which made the first barrier of
// CMUX i wait for the key words of CMUX i + 1 that the kernel's prefetch had just requested (an L2 / HBM round trip on
// the critical path of every CMUX) -- with LDS-only barriers they stay in flight for a whole CMUX.
__device__ __forceinline__ void lat_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// one CMUX of the latency kernel (phases A, B, C and their three barriers)
#ifndef FFT_LATSTAMP
#define FFT_LATSTAMP 0
#endif
#if FFT_LATSTAMP
// diagnostic build only: per-CMUX phase times of the latency kernel (s_memrealtime, 100 MHz), summed per wave:
// [0] CMUX start -> this wave done with phase A (before barrier 1), [1] -> past barrier 1, [2] -> done with phase B,
// [3] -> past barrier 2, [4] -> done with phase C, [5] -> past barrier 3
struct LatStamp {
  unsigned long long acc[6] = {0, 0, 0, 0, 0, 0}, t0 = 0;
  __device__ __forceinline__ void start() { t0 = __builtin_amdgcn_s_memrealtime(); }
  __device__ __forceinline__ void mark(int k) { acc[k] += __builtin_amdgcn_s_memrealtime() - t0; }
};
__device__ unsigned long long g_latst[8 * 8 * 6];  // workgroup 0..7 x wave x phase mark
#define LS_START(st) st.start()
#define LS_MARK(st, k) st.mark(k)
#else
struct LatStamp {};
#define LS_START(st)
#define LS_MARK(st, k)
#endif
__device__ __forceinline__ void lat_cmux(FftLatShared& sh, const u64* __restrict__ ct, int i, int wave, int lane,
                                         TBase tb, int j, int s0, const double2 (&kv)[6][2], LatStamp& ls) {
  LS_START(ls);
  const int a = i < FL_MAXN ? (int)sh.ab[i] : ms2048(ct[i]);
  if (wave < 6) {  // phase A
    const int c = wave / 3, q = wave % 3;
    const u64* acc = sh.A[c];
    u32 st[16];
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const int t = 64 * e + lane - a + 2 * N1K;
      const u64 x = acc[t & (N1K - 1)];
      const u64 r = (t & N1K) ? 0 - x : x;
      st[e] = decomp_state(r - acc[64 * e + lane]);
    }
    int dg[16];
    for (int qq = 0; qq <= q; qq++) {
      const u32 bmask = qq < 2 ? 1u : 0u;
#pragma unroll
      for (int e = 0; e < 16; e++) dg[e] = decomp_step(st[e], bmask);
    }
    double xr[8], xi[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
      xr[e] = (double)dg[e];
      xi[e] = (double)dg[e + 8];
    }
    dft512_fwd(xr, xi, sh.T[wave], lane, tb, sh.tw);
#pragma unroll
    for (int e = 0; e < 8; e++) sh.F[wave][64 * e + lane] = make_double2(xr[e], xi[e]);
  }
  LS_MARK(ls, 0);
  lat_barrier();
  LS_MARK(ls, 1);
  {  // phase B
    double2* O = sh.T[2 + j];
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const int e = s0 + t;
      double re[2], im[2];  // per-component chains (the first term a multiply), then one add (oracle order)
#pragma unroll
      for (int r = 0; r < 6; r++) {
        const double2 D = sh.F[r][64 * e + lane], K = kv[r][t];
        const int cc = r / 3;
        if (r % 3 == 0) mac_first(re[cc], im[cc], D.x, D.y, K);
        else mac_next(re[cc], im[cc], D.x, D.y, K);
      }
      O[64 * e + lane] = make_double2(re[0] + re[1], im[0] + im[1]);
    }
  }
  LS_MARK(ls, 2);
  lat_barrier();
  LS_MARK(ls, 3);
  if (wave < 2) {  // phase C
    const double2* O = sh.T[2 + wave];
    double xr[8], xi[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const double2 v = O[64 * e + lane];
      xr[e] = v.x;
      xi[e] = v.y;
    }
    fft_inv_real(xr, xi, sh.T[wave], lane, tb, sh.tw);
    u64* acc = sh.A[wave];
#pragma unroll
    for (int e = 0; e < 8; e++) {
      acc[64 * e + lane] = torus_acc_add_y(acc[64 * e + lane], xr[e]);
      acc[64 * (e + 8) + lane] = torus_acc_add_y(acc[64 * (e + 8) + lane], xi[e]);
    }
  }
  LS_MARK(ls, 4);
  lat_barrier();
  LS_MARK(ls, 5);
}

template <bool WRITE_ACC, bool WRITE_BIG>
__global__ __launch_bounds__(FL_THREADS, 1) void blind_rotate_fft_lat_kernel(
    const u64* __restrict__ lwe_in, int n, size_t B, const u64* __restrict__ luts, const u32* __restrict__ lut_index,
    int n_lut, const double2* __restrict__ bsk, const double2* __restrict__ tw_g, u64* __restrict__ out_big,
    u64* __restrict__ out_acc) {
  __shared__ __attribute__((aligned(16))) FftLatShared sh;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t b = blockIdx.x;
  const u64* ct = lwe_in + b * (size_t)(n + 1);
  const TBase tb(lane);

  for (int q = threadIdx.x; q < TW_C64; q += FL_THREADS) sh.tw[q] = tw_g[q];
  for (int q = threadIdx.x; q < n && q < FL_MAXN; q += FL_THREADS) sh.ab[q] = (unsigned short)ms2048(ct[q]);
  {
    int li = lut_index ? (int)lut_index[b] : 0;
    li = (li < 0 || li >= n_lut) ? 0 : li;
    const u64* lut = luts + (size_t)li * N1K;
    const int s = (2048 - ms2048(ct[n])) & 2047;
    for (int q = threadIdx.x; q < N1K; q += FL_THREADS) {
      int d = q - s;
      bool neg = false;
      if (d < 0) { d += N1K; neg = !neg; }
      if (d < 0) { d += N1K; neg = !neg; }
      const u64 v = gl_to_torus(lut[d]);
      sh.A[0][q] = 0;
      sh.A[1][q] = neg ? 0 - v : v;
    }
  }
  __syncthreads();

  const int j = wave >> 2, s0 = (wave & 3) * 2;  // phase B: output j, slots s0, s0 + 1
  LatStamp ls;
  // key words one CMUX ahead (two register sets, the loop unrolled by two): a CMUX's row arrives while the
  // previous CMUX runs instead of behind this CMUX's phase A
  double2 kva[6][2], kvb[6][2];
  lat_load_key(bsk, 0, j, s0, lane, kva);
  for (int i = 0; i < n; i += 2) {
    if (i + 1 < n) lat_load_key(bsk, i + 1, j, s0, lane, kvb);
    lat_cmux(sh, ct, i, wave, lane, tb, j, s0, kva, ls);
    if (i + 1 >= n) break;
    if (i + 2 < n) lat_load_key(bsk, i + 2, j, s0, lane, kva);
    lat_cmux(sh, ct, i + 1, wave, lane, tb, j, s0, kvb, ls);
  }

#if FFT_LATSTAMP
  if (lane == 0 && b < 8)
    for (int k = 0; k < 6; k++) g_latst[(b * 8 + wave) * 6 + k] = ls.acc[k];
#endif
  if (WRITE_ACC) {
    u64* oa = out_acc + b * 2048;
    for (int q = threadIdx.x; q < 2 * N1K; q += FL_THREADS) oa[q] = sh.A[q >> 10][q & (N1K - 1)];
  }
  if (WRITE_BIG) {  // sample extraction at degree 0
    u64* ob = out_big + b * (size_t)(N1K + 1);
    for (int q = threadIdx.x; q <= N1K; q += FL_THREADS)
      ob[q] = q == N1K ? sh.A[1][0] : q == 0 ? sh.A[0][0] : 0 - sh.A[0][N1K - q];
  }
}

// ---------------------------------------------------------------------------------------------
// host: tables (fixed series in plain double, octant-reduced — the oracle's or_fft_twiddle)
static double fs_sin(double x) {
  double x2 = x * x, term = x, sum = 0.0;
  for (int i = 1; i <= 21; i += 2) { sum += term; term = -term * x2 / (double)((i + 1) * (i + 2)); }
  return sum;
}
static double fs_cos(double x) {
  double x2 = x * x, term = 1.0, sum = 0.0;
  for (int i = 0; i <= 20; i += 2) { sum += term; term = -term * x2 / (double)((i + 1) * (i + 2)); }
  return sum;
}
static void tw_octant(uint32_t t, uint32_t m, double* c, double* s) {
  const double x = (double)t * (6.28318530717958647692 / (double)m);
  *c = fs_cos(x);
  *s = fs_sin(x);
}
static void tw_quarter(uint32_t t, uint32_t m, double* c, double* s) {
  if (8 * t > m) {
    double cu, su;
    tw_octant(m / 4 - t, m, &cu, &su);
    *c = su;
    *s = cu;
  } else {
    tw_octant(t, m, c, s);
  }
}
static void twiddle(uint32_t t, uint32_t m, double* c, double* s) {
  t %= m;
  bool neg = false;
  if (2 * t > m) { t = m - t; neg = true; }
  double cc, ss;
  if (4 * t > m) {
    double cu, su;
    tw_quarter(t - m / 4, m, &cu, &su);
    cc = -su;
    ss = cu;
  } else {
    tw_quarter(t, m, &cc, &ss);
  }
  *c = cc;
  *s = neg ? -ss : ss;
}

}  // namespace fftk

void fft_twiddle(uint32_t t, uint32_t m, double* c, double* s) { fftk::twiddle(t, m, c, s); }

// N = 1024 tables with the twist merged into the passes (fft512.h, "N = 1024 merged twist"):
//   TW_A[e][L] = zeta^(L (1 + 4 e)),  TW_B as before,  TW_I[e][L] = zeta^((n0 + 8 e)(4 k0 + 1)) (L = n0 + 8 k0),
// zeta = e^(2 pi i / 2048); TW_TWIST keeps zeta^j (the slot constants are its entries j = 64 e)
// false: the compile-time slot constants differ from the table generator's zeta^(64 e) in some bit
static bool make_tables_f1k(u64* tw) {
  using namespace fftk;
  double* t = (double*)tw;
  for (uint32_t j = 0; j < (uint32_t)M; j++) twiddle(j, 4 * M, &t[2 * (TW_TWIST + j)], &t[2 * (TW_TWIST + j) + 1]);
  for (uint32_t e = 0; e < 8; e++)
    for (uint32_t L = 0; L < 64; L++) {
      twiddle((L * (1 + 4 * e)) % (4 * M), 4 * M, &t[2 * (TW_A + 64 * e + L)], &t[2 * (TW_A + 64 * e + L) + 1]);
      twiddle((8 * (L & 7) * e) % M, M, &t[2 * (TW_B + 64 * e + L)], &t[2 * (TW_B + 64 * e + L) + 1]);
      twiddle((((L & 7) + 8 * e) * (4 * (L >> 3) + 1)) % (4 * M), 4 * M, &t[2 * (TW_I + 64 * e + L)],
              &t[2 * (TW_I + 64 * e + L) + 1]);
    }
  for (int e = 0; e < 8; e++) {
    double c, s, c2, s2;
    twiddle(64u * e, 2048u, &c, &s);      // N = 1024
    twiddle(128u * e, 4096u, &c2, &s2);   // N = 2048
    if (c != ctw::SLOT[e].x || s != ctw::SLOT[e].y || c2 != c || s2 != s) return false;
  }
  return true;
}

static hipError_t convert_bsk_f1k(const u64* bsk_std, u64* bsk_f, size_t polys, const u64* tw, hipStream_t s) {
  if (polys == 0) return hipSuccess;
  hipLaunchKernelGGL(fftk::bsk_to_fourier_kernel, dim3((unsigned)polys), dim3(64), 0, s, bsk_std, (double2*)bsk_f,
                     (const double2*)tw);
  return hipGetLastError();
}

static hipError_t blind_rotate_f1k(const u64* lwe_in, size_t B, int n, const u64* luts, const u32* lut_index,
                                   int n_lut, const u64* bsk_f, const u64* tw, u64* out_big, u64* out_acc,
                                   bool latency, int n_cus, hipStream_t s) {
  using namespace fftk;
  if (B == 0) return hipSuccess;
  if (n_cus <= 0) n_cus = 256;
  const double2 *bk = (const double2*)bsk_f, *t = (const double2*)tw;
  if (latency)
    return launch_out_mode(out_acc, out_big, [&](auto wa, auto wb) {
      hipLaunchKernelGGL((blind_rotate_fft_lat_kernel<wa(), wb()>), dim3((unsigned)B), dim3(FL_THREADS), 0, s, lwe_in,
                         n, B, luts, lut_index, n_lut, bk, t, out_big, out_acc);
    });
  constexpr int CTS = 2;  // ciphertexts per workgroup (FpShared)
  return launch_out_mode(out_acc, out_big, [&](auto wa, auto wb) {
    hipLaunchKernelGGL((blind_rotate_fft_pair_kernel<CTS, wa(), wb()>), dim3((unsigned)((B + CTS - 1) / CTS)),
                       dim3(128 * CTS), 0, s, lwe_in, n, B, luts, lut_index, n_lut, bk, t, out_big, out_acc, n_cus);
  });
}

#if FFT_LATSTAMP
extern "C" int tfhe_hip_debug_latstamps(unsigned long long* out, size_t n) {
  if (n > 8 * 8 * 6) n = 8 * 8 * 6;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(fftk::g_latst), n * 8, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
#if FFT_DMASTAMP
extern "C" int tfhe_hip_debug_dmastamps(unsigned long long* out, size_t n) {
  if (n > 64 * 4 * 4) n = 64 * 4 * 4;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(fftk::g_dmast), n * 8, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
#if FFT_WGTIME
extern "C" int tfhe_hip_debug_wgtimes(unsigned long long* out, size_t n) {
  if (n > 4 * 16384) n = 4 * 16384;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(fftk::g_wgt), n * 8, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

static hipError_t fft_fwd_f1k(const u64* in, size_t count, u64* out, const u64* tw, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(fftk::fft_fwd_kernel, dim3((unsigned)count), dim3(64), 0, s, in, (double2*)out,
                     (const double2*)tw);
  return hipGetLastError();
}

static hipError_t fft_inv_f1k(const u64* in, size_t count, u64* out, const u64* tw, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(fftk::fft_inv_kernel, dim3((unsigned)count), dim3(64), 0, s, (const double2*)in, (double*)out,
                     (const double2*)tw);
  return hipGetLastError();
}

// latency crossover 256: the component-pair batch kernel runs any batch up to 1024 in one 6.7 ms round, the latency
// kernel 3.5-3.7 ms up to 256 and 7.1 ms from 257 (profiles/r03_latsweep.json, tools/latency_sweep.py)
#ifndef __HIP_DEVICE_COMPILE__  // a host object: the device pass would emit it with its pointers to host functions
const br_engine ENGINE_FFT1K = {true,
                                N1K,
                                256,
                                "blind_rotate_fft_lat_kernel",
                                "blind_rotate_fft_pair_kernel",
                                2 * fftk::TW_C64,
                                make_tables_f1k,
                                convert_bsk_f1k,
                                blind_rotate_f1k,
                                fft_fwd_f1k,
                                fft_inv_f1k};
#endif

}  // namespace tfhe
