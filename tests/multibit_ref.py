"""The multi-bit blind rotation (include/tfhe_hip.h, tfhe-rs LweMultiBitBootstrapKey) in EXACT arithmetic over Z_2^64,
and the rounding-error bound of the device's FFT64 group step against it (derivation: DESIGN.md §4o, next to §5b).

Reference.  Per group q the coefficient-domain bundle  K_eff[c][j] = sum_sigma (X^{t_sigma} - 1) K_{q,sigma}[c][j]  is
built by negacyclic rotations and wrapping adds, the SignedDecomposer digits (2^23 x 1) are taken from acc itself, and
    acc_j <- acc_j + sum_c digits(acc_c) (*) K_eff[c][j]
runs as four exact negacyclic products (the oracle's poly_mul_torus_exact: no floating point).
t_sigma = ms( sum_{i in sigma} a_{gq+i} mod 2^64 ): the sum first, then the switch.

Bound.  tests/fft_error_model.py's Higham-style worst case with the multi-bit step's extra operations.  With R = (k+1) L
digit polynomials, NS = 2^g - 1 stored GGSWs, u = 2^-53, mu the twiddle tables' error bound, alpha the transforms':
    eps_f   = mu + 2 u                 the factor f = w - 1: one more computed twiddle (|w^ - w| <= mu) and one
                                       subtraction (|f| <= 2, error <= 2 u), relative to the magnitude 2 that S1 carries
    chain   = 2 R NS + 1               fma terms per output component: 2 R per sigma in P, 2 per sigma in O += f P,
                                       (2 NS + 2 R <= 2 R NS + 1); a three-factor complex product's componentwise
                                       absolute sum is at most 2 |f| |D| |K|
    beta_mb = (1 + alpha)^2 (1 + eps_f) (1 + 2 gamma_chain) - 1
    |device - exact| <= sqrt(M) S1 (beta_mb + alpha (1 + beta_mb)) + 1/2
    S1 = sum_r ||d_r||_2 sum_{sigma: t_sigma != 0} 2 ||w_{sigma,r,j}||_2
(key polynomials w read as signed int64, as the transform reads them).  A term with t_sigma = 0 is exactly zero on the
device (w - 1 = (0, 0) from the table's exact entry 0), so a group whose t_sigma are all 0 is an exact identity.
"""
import math

import numpy as np

import fft_error_model as fem

N2 = 2048
BASE_LOG = 23
MASK = (1 << 64) - 1


def ms(x, two_n: int = 2 * N2) -> np.ndarray:
    """the classic rounding to 2N: round(x 2N / 2^64) mod 2N"""
    x = np.asarray(x, dtype=np.uint64)
    lg = int(two_n).bit_length() - 1
    return ((((x >> np.uint64(64 - lg - 1)) + np.uint64(1)) >> np.uint64(1)) & np.uint64(two_n - 1)).astype(np.int64)


def subset_switch(masks, two_n: int = 2 * N2) -> np.ndarray:
    """t_sigma, sigma = 1 .. 2^g - 1, of the g masks of one group (bit i of sigma <-> masks[i]): sum, THEN switch."""
    a = [int(v) for v in np.asarray(masks, dtype=np.uint64)]
    g = len(a)
    sums = [sum(a[i] for i in range(g) if (s >> i) & 1) & MASK for s in range(1, 1 << g)]
    return ms(np.array(sums, dtype=np.uint64), two_n)


def exponents() -> np.ndarray:
    """e[64 m1 + L]: the odd exponent of zeta = e^{2 pi i / 4096} at which point (slot m1, lane L) of fft1k's output
    order evaluates the polynomial: Z[k] = P(zeta^{1 + 4k}), k = (L & 3) + 4 (L >> 4) + 16 ((L >> 2) & 3) + 64 m1."""
    m1, L = np.divmod(np.arange(1024), 64)
    k = (L & 3) + 4 * (L >> 4) + 16 * ((L >> 2) & 3) + 64 * m1
    return (1 + 4 * k) % 4096


def digits(acc) -> np.ndarray:
    """tfhe-rs SignedDecomposer, 2^23 x 1: the closest multiple of 2^41, as a signed digit in (-2^22, 2^22]."""
    h = (np.asarray(acc, dtype=np.uint64) >> np.uint64(32)).astype(np.int64)
    half = (1 << (BASE_LOG - 1)) - 1
    return ((((h + 256) >> 9) + half) % (1 << BASE_LOG)) - half


def rotate(poly: np.ndarray, t: int) -> np.ndarray:
    """X^t poly mod X^N + 1 over Z_2^64, 0 <= t < 2N"""
    poly = np.asarray(poly, dtype=np.uint64)
    N = poly.shape[-1]
    if t >= N:
        return rotate(np.uint64(0) - poly, t - N)
    if t == 0:
        return poly.copy()
    return np.concatenate([np.uint64(0) - poly[..., N - t:], poly[..., :N - t]], axis=-1)


def key_view(bsk_mb, g: int, n: int, N: int = N2) -> np.ndarray:
    """[q][sigma - 1][row c][col j][N] (level 1)"""
    return np.asarray(bsk_mb, dtype=np.uint64).reshape(n // g, (1 << g) - 1, 2, 2, N)


def initial_acc(ct, lut, N: int = N2) -> np.ndarray:
    """A = 0, B = X^{-b~} lut, the LUT's Z_p-encoded values mapped to the torus (gl64.h gl_to_torus)"""
    lut = np.asarray(lut, dtype=np.uint64)
    v = lut + ((lut + np.uint64(0x80000000)) >> np.uint64(32))
    bt = int(ms(np.asarray(ct, dtype=np.uint64)[-1:], 2 * N)[0])
    return np.stack([np.zeros(N, dtype=np.uint64), rotate(v, (2 * N - bt) % (2 * N))])


def group_step(oracle_mod, key_q, t, acc):
    """One exact group step.  key_q [NS][2][2][N], t [NS], acc [2][N] -> (acc_out [2][N], s1 [2])."""
    key_q = np.asarray(key_q, dtype=np.uint64)
    acc = np.asarray(acc, dtype=np.uint64).reshape(2, -1)
    N = acc.shape[1]
    k_eff = np.zeros((2, 2, N), dtype=np.uint64)
    wnorm = np.zeros((2, 2))
    for s, ts in enumerate(np.asarray(t)):
        if int(ts) == 0:
            continue
        k_eff += rotate(key_q[s], int(ts)) - key_q[s]
        wnorm += 2 * np.sqrt((fem.signed(key_q[s]) ** 2).sum(axis=-1))
    d = digits(acc)
    dn = np.sqrt((d.astype(np.float64) ** 2).sum(axis=-1))
    out = acc.copy()
    for j in range(2):
        for c in range(2):
            out[j] += oracle_mod.poly_mul_torus_exact(d[c], k_eff[c][j])
    return out, (dn[:, None] * wnorm).sum(axis=0)


def blind_rotate_trace(oracle_mod, bsk_mb, g: int, ct, lut, acc0=None, N: int = N2):
    """-> (trace [n/g + 1][2N]: the accumulator before group 0 and after every group, s1 [n/g][2])"""
    ct = np.asarray(ct, dtype=np.uint64)
    n = ct.shape[0] - 1
    key = key_view(bsk_mb, g, n, N)
    acc = initial_acc(ct, lut, N) if acc0 is None else np.asarray(acc0, dtype=np.uint64).reshape(2, N)
    trace, s1 = [acc.reshape(-1).copy()], []
    for q in range(n // g):
        acc, s = group_step(oracle_mod, key[q], subset_switch(ct[g * q:g * q + g], 2 * N), acc)
        trace.append(acc.reshape(-1).copy())
        s1.append(s)
    return np.array(trace), np.array(s1).reshape(-1, 2)


def worst_case_bound(g: int, s1, N: int = N2, R: int = 2, mu: float = fem.MU_BOUND):
    """max |device - exact| per output coefficient of one group step, for norm sums s1 (array-like)"""
    M = N // 2
    ns = (1 << g) - 1
    eta = mu + 2 * math.sqrt(2) * fem.U * (1 + mu)
    alpha = (1 + eta) ** fem.STAGES - 1
    eps_f = mu + 2 * fem.U
    beta = (1 + alpha) ** 2 * (1 + eps_f) * (1 + 2 * fem.gamma(2 * R * ns + 1)) - 1
    return math.sqrt(M) * np.asarray(s1, dtype=np.float64) * (beta + alpha * (1 + beta)) + 0.5


def check_steps(g: int, got_next, exact_next, s1, N: int = N2):
    """Device states after a group step against the exact step of the same input: every coefficient within the bound,
    exactly equal where the step is an identity (s1 == 0).  -> the figures the tests print."""
    d = fem.signed(np.asarray(got_next, dtype=np.uint64) - np.asarray(exact_next, dtype=np.uint64)).reshape(-1, 2, N)
    s1 = np.asarray(s1, dtype=np.float64).reshape(-1, 2)
    bound = worst_case_bound(g, s1, N)
    err = np.abs(d).max(axis=2)
    live = s1 > 0
    stats = dict(steps=int(live.any(axis=1).sum()), max_err_log2=math.log2(max(float(err.max()), 1.0)))
    if live.any():
        stats["bound_log2_min"] = math.log2(float(bound[live].min()))
        stats["max_over_bound_log2"] = math.log2(max(float((err[live] / bound[live]).max()), 2.0 ** -60))
        stats["rms_err_log2"] = 0.5 * math.log2(max(float((d[live] ** 2).mean()), 2.0 ** -60))
        # the scale of the variance model: u x the rms size of the exact product's coefficients, taken from s1
        rms = math.sqrt(float((d[live] ** 2).mean()))
        stats["rms_over_u_s1"] = rms / (fem.U * float(s1[live].mean()) / math.sqrt(N))
    print(f"multi-bit g = {g}: {stats}")
    assert np.all(err[~live] == 0), "a group step whose t_sigma are all zero must be exact"
    assert np.all(err <= bound), f"FFT error above the derived bound: {np.max(err / bound):.3g} x"
    return stats
