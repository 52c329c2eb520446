"""The 128-bit packing keyswitch and its stored form in Python integers, written from the rule stated in
include/tfhe_hip.h (tfhe_sns_pks_params) and not from the C++: digits, pack, compress, extract.  Also the
parameter sets, inputs and cached references shared by tests/test_sns_compression.py (CPU) and
tests/test_gpu_sns_compression.py (device).

Words of Z_2^128 are Python ints here.  An LWE array is (count, in_dim + 1, 2) u64 pairs (lo, hi); a GLWE array is
(out_k + 1, 2, N) u64 planes; a key is [j][l][c][lo, hi][N]."""
import functools
import math

import numpy as np

from tfhe_amd import sns_compression as SC

U64 = (1 << 64) - 1
U128 = (1 << 128) - 1
SEED = 0x5C0128
NOISE_LOG2 = -62                     # the preset's key noise, std 4

# name -> (in_dim, out_k, out_N, base_log, level, lwe_per_glwe, storage_log)
SETS = {
    "A": (64, 1, 32, 61, 1, 32, 128),
    "B": (48, 2, 64, 20, 3, 20, 75),     # three column tiles, a partial-N group, stored values straddling words
    "C": (80, 1, 64, 63, 2, 64, 64),     # widest digit, prec 126
    "D": (512, 6, 1024, 61, 1, 128, 128),  # the preset's GLWE shape; device only
}


def make_params(name) -> SC.SnsPksParams:
    return SC.SnsPksParams(*SETS[name], NOISE_LOG2)


def counts(pp):
    lpg = pp.lwe_per_glwe
    return (1, lpg - 1, lpg, lpg + 1, 2 * lpg + 5)


# ---- conversions ----------------------------------------------------------------------------------------------
def pairs_to_ints(a) -> np.ndarray:
    """(..., 2) u64 pairs (lo, hi) -> object array of ints"""
    a = np.asarray(a, dtype=np.uint64)
    return a[..., 0].astype(object) | (a[..., 1].astype(object) << 64)


def ints_to_pairs(w) -> np.ndarray:
    w = np.asarray(w, dtype=object)
    return np.stack([(w & U64).astype(np.uint64), (w >> 64).astype(np.uint64)], axis=-1)


def planes_to_ints(g) -> np.ndarray:
    """(..., 2, N) u64 planes -> (..., N) ints"""
    g = np.asarray(g, dtype=np.uint64)
    return g[..., 0, :].astype(object) | (g[..., 1, :].astype(object) << 64)


def ints_to_planes(w) -> np.ndarray:
    w = np.asarray(w, dtype=object)
    return np.stack([(w & U64).astype(np.uint64), (w >> 64).astype(np.uint64)], axis=-2)


def key_rows(pp, pksk) -> np.ndarray:
    """the key as ints [in_dim * level][(out_k + 1) * N]"""
    K = pp.in_dim * pp.level
    return planes_to_ints(np.asarray(pksk, dtype=np.uint64).reshape(K, pp.out_k + 1, 2, pp.out_N)).reshape(K, -1)


# ---- the rule -------------------------------------------------------------------------------------------------
def digits(a: int, base_log: int, level: int) -> list:
    """balanced digits of a mask word, digit[0] most significant"""
    prec, B = base_log * level, 1 << base_log
    state = (((a >> (128 - prec - 1)) + 1) >> 1) & ((1 << prec) - 1)
    out = [0] * level
    for l in range(level - 1, -1, -1):
        res = state & (B - 1)
        state >>= base_log
        carry = ((((res - 1) | state) & res) >> (base_log - 1)) & 1
        state += carry
        out[l] = res - carry * B
    return out


def pack(pp, rows: np.ndarray, lwes) -> np.ndarray:
    """rows: key_rows(); lwes (count, in_dim + 1, 2) -> GLWE planes (groups, out_k + 1, 2, N)"""
    w = pairs_to_ints(np.asarray(lwes, dtype=np.uint64).reshape(-1, pp.in_dim + 1, 2))
    count, N, k, lpg = w.shape[0], pp.out_N, pp.out_k, pp.lwe_per_glwe
    Nc = (k + 1) * N
    out = []
    for first in range(0, count, lpg):
        cnt = min(lpg, count - first)
        acc = np.zeros(Nc, dtype=object)
        for d in range(cnt):
            T = np.zeros(Nc, dtype=object)
            for j in range(pp.in_dim):
                for l, dg in enumerate(digits(int(w[first + d, j]), pp.base_log, pp.level)):
                    if dg:
                        T = T + dg * rows[j * pp.level + l]
            term = -T
            term[k * N] += int(w[first + d, pp.in_dim])          # (0, ..., 0, b_d) - T_d
            term = term.reshape(k + 1, N)
            # X^d * term, negacyclic: coefficient t comes from t - d, negated when it wraps
            rot = np.concatenate([-term[:, N - d:], term[:, :N - d]], axis=1) if d else term
            acc = acc + rot.reshape(-1)
        out.append(ints_to_planes((acc & U128).reshape(k + 1, N)))
    return np.stack(out) if out else np.zeros((0, k + 1, 2, N), dtype=np.uint64)


def stored_values(pp, glwe, bodies: int) -> list:
    """the out_k * N mask coefficients, then `bodies` body coefficients, switched to storage_log bits"""
    w = planes_to_ints(np.asarray(glwe, dtype=np.uint64).reshape(pp.out_k + 1, 2, pp.out_N)).reshape(-1)
    s = pp.storage_log
    vals = [int(x) for x in w[:pp.out_k * pp.out_N + bodies]]
    if s < 128:
        vals = [(((x >> (128 - s - 1)) + 1) >> 1) % (1 << s) for x in vals]
    return vals


def packed_words(pp, bodies: int) -> int:
    return -(-(pp.out_k * pp.out_N + bodies) * pp.storage_log // 64)


def compress(pp, glwe, bodies: int) -> np.ndarray:
    """LSB-first bit packing of the stored values into u64 words"""
    big = 0
    for i, v in enumerate(stored_values(pp, glwe, bodies)):
        big |= v << (i * pp.storage_log)
    return np.array([(big >> (64 * i)) & U64 for i in range(packed_words(pp, bodies))], dtype=np.uint64)


def extract(pp, packed, bodies: int) -> np.ndarray:
    s = pp.storage_log
    big = sum(int(x) << (64 * i) for i, x in enumerate(np.asarray(packed, dtype=np.uint64)))
    w = np.zeros((pp.out_k + 1) * pp.out_N, dtype=object)
    for i in range(pp.out_k * pp.out_N + bodies):
        w[i] = ((big >> (i * s)) & ((1 << s) - 1)) << (128 - s)
    return ints_to_planes(w.reshape(pp.out_k + 1, pp.out_N))


def phase(pp, out_key, glwe) -> list:
    """body - sum_c mask_c * S_c (negacyclic) of one GLWE, in Python ints (slow: small N only)"""
    N, k = pp.out_N, pp.out_k
    w = planes_to_ints(np.asarray(glwe, dtype=np.uint64).reshape(k + 1, 2, N))
    ph = [int(x) for x in w[k]]
    for c in range(k):
        for u in range(N):
            if not out_key[c * N + u]:
                continue
            for i in range(N):
                if i + u < N:
                    ph[i + u] -= int(w[c][i])
                else:
                    ph[i + u - N] += int(w[c][i])
    return [x & U128 for x in ph]


# ---- inputs ---------------------------------------------------------------------------------------------------
def special_masks(pp) -> list:
    prec = pp.base_log * pp.level
    return [0, 1 << 127, U128, 1 << (127 - prec)]       # the last: the rounding tie of the decomposition


def _uniform(pp, count, rng) -> np.ndarray:
    return rng.integers(0, 2 ** 64, size=(count, pp.in_dim + 1, 2), dtype=np.uint64)


def inputs(pp, count, seed=7) -> list:
    """Input arrays for one count: uniformly random 128-bit words, with the four special rows (mask all 0, all 2^127,
    all ones, all exactly the rounding tie 2^(127 - prec); bodies random) as the last rows.  A count below four gets
    one array per special row instead, each with that row last, after the all-random array."""
    rng = np.random.default_rng([seed, count, pp.in_dim, pp.base_log])
    sp = [ints_to_pairs(np.full(pp.in_dim, m, dtype=object)) for m in special_masks(pp)]
    if count >= len(sp):
        x = _uniform(pp, count, rng)
        for i, s in enumerate(sp):
            x[count - 1 - i, :pp.in_dim] = s
        return [x]
    out = [_uniform(pp, count, rng)]
    for s in sp:
        x = _uniform(pp, count, rng)
        x[count - 1, :pp.in_dim] = s
        out.append(x)
    return out


def encrypt(pp, in_key, msgs, msg_modulus=16, seed=11) -> np.ndarray:
    """Valid noiseless encryptions built here: mask uniform, b = <a, s> + delta * m, delta = 2^127 / msg_modulus."""
    rng = np.random.default_rng([seed, len(msgs)])
    x = rng.integers(0, 2 ** 64, size=(len(msgs), pp.in_dim + 1, 2), dtype=np.uint64)
    a = pairs_to_ints(x[:, :pp.in_dim])
    delta = (1 << 127) // msg_modulus
    s = np.asarray(in_key, dtype=np.uint64).astype(bool)
    for q, m in enumerate(msgs):
        b = (int(a[q][s].sum()) + delta * int(m)) & U128
        x[q, pp.in_dim] = (b & U64, b >> 64)
    return x


def error_bound(pp, cnt: int) -> float:
    """Per-coefficient decryption error after pack (and the stored form): worst-case rounding of the decomposition,
    the key noise at 8 sigma, and the storage rounding when storage_log < 128."""
    prec = pp.base_log * pp.level
    b = pp.in_dim * 2.0 ** (127 - prec)
    b += 8 * 2.0 ** (64 + pp.noise_log2) * 2.0 ** (pp.base_log - 1) * math.sqrt(cnt * pp.in_dim * pp.level)
    if pp.storage_log < 128:
        b += (pp.out_k * pp.out_N + 1) * 2.0 ** (127 - pp.storage_log)
    return b


def centered(x: int) -> int:
    x &= U128
    return x - (1 << 128) if x >> 127 else x


# ---- shared, cached material -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def keys(name):
    """(params, SquashedCompressionKey) of a set, for a random binary input key"""
    pp = make_params(name)
    in_key = np.random.default_rng(sum(map(ord, name))).integers(0, 2, pp.in_dim).astype(np.uint64)
    return pp, SC.SquashedCompressionKey(pp, SEED, in_key)


@functools.lru_cache(maxsize=None)
def _rows(name):
    pp, key = keys(name)
    return key_rows(pp, key.pksk)


@functools.lru_cache(maxsize=None)
def case(name, count):
    """[(lwes, reference GLWEs)] of a set and count; computed once, shared by the CPU and the device tests"""
    pp, _ = keys(name)
    out = []
    for x in inputs(pp, count):
        x.setflags(write=False)
        ref = pack(pp, _rows(name), x)
        ref.setflags(write=False)
        out.append((x, ref))
    return out
