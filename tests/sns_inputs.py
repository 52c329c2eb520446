"""Inputs shared by the noise-squashing tests (tests/test_sns.py on the CPU, tests/test_gpu_sns_edges.py on the
device): product and oracle keys at a small LWE dimension, ciphertext words on the edges of the modulus switch to
2N = 4096, synthetic key words on the edges of the load rounding, the limb split and the 72-bit decomposition, and
the Python restatement of that decomposition which certifies that the inputs reach the edges they aim at."""
import copy
import os

import numpy as np

from tfhe_amd import sns as S

U64 = (1 << 64) - 1
U128 = (1 << 128) - 1
TIE_SEED, TIE_N = 0x71E5, 3       # the synthetic "ties" key of the CPU tie count and of the device test
KINDS = ("ties", "limb_edges", "uniform")


def chunk_size() -> int:
    """Ciphertexts per pass of the device's host loop, read the way sns_api.cpp reads it."""
    try:
        x = int(os.environ.get("TFHE_HIP_SNS_CHUNK", "0"))
    except ValueError:
        x = 0
    return x if x > 0 else 512


def small_params(oracle_mod, n):
    sp, osp = S.SnsParams.preset(0), oracle_mod.sns_params(0)
    sp.n = osp.n = n
    return sp, osp


def small_keys(oracle_mod, n, seed):
    """(sp, osp, product SquashedKey, oracle SnsKeys) at the preset with n overridden, for a random binary LWE key."""
    sp, osp = small_params(oracle_mod, n)
    lwe_key = np.random.default_rng(seed).integers(0, 2, n).astype(np.uint64)
    key = S.SquashedKey(sp, seed, lwe_key)
    okeys = oracle_mod.SnsKeys(osp, seed, lwe_key)
    assert np.array_equal(key.bsk, okeys.bsk)
    return sp, osp, key, okeys


def mod_switch_4096(x) -> np.ndarray:
    """The switch to 2N = 4096: bits 52..63 kept, bit 51 rounds, 4096 wraps to 0."""
    x = np.asarray(x, dtype=np.uint64)
    return (((x >> np.uint64(51)) + np.uint64(1)) >> np.uint64(1)) & np.uint64(4095)


SWITCHED = (1, 2047, 2048, 2049, 4095)                     # values the masks and bodies must switch to ...
WRAP = (1 << 64) - (1 << 51)                               # ... and 0, by rounding up to 4096
RAW = (0, U64, (1 << 51) - 1, 1 << 51, (1 << 51) + 1, 3 << 51, WRAP)


def edge_inputs(n, B, seed) -> np.ndarray:
    """B x (n + 1) words.  Among uniformly random words, masks and bodies hold RAW (0, 2^64 - 1, the rounding ties of
    the switch from both sides, 2^64 - 2^51 which rounds up to 4096 and wraps to 0) and words that switch to each of
    SWITCHED, with random bits below the rounding bit.  From B = 2 the last row's mask is all 2^63 (a rotation by N
    in every CMUX), from B = 3 the row before it has an all-zero mask (no CMUX moves the accumulator)."""
    rng = np.random.default_rng(seed)
    cts = rng.integers(0, 2 ** 64, size=(B, n + 1), dtype=np.uint64)

    def specials():
        low = rng.integers(0, 1 << 51, len(SWITCHED), dtype=np.uint64)
        return np.concatenate([np.array(RAW, dtype=np.uint64),
                               (np.array(SWITCHED, dtype=np.uint64) << np.uint64(52)) + low])

    free_rows = B - (B >= 2) - (B >= 3)
    masks = cts[:free_rows, :n].reshape(-1).copy()
    pos = rng.permutation(masks.size)[:max(masks.size // 2, min(masks.size, len(RAW) + len(SWITCHED)))]
    for f in range(0, pos.size, len(RAW) + len(SWITCHED)):
        sp = specials()
        masks[pos[f:f + sp.size]] = sp[:pos.size - f]
    cts[:free_rows, :n] = masks.reshape(free_rows, n)
    sp = specials()
    rows = rng.permutation(B)[:sp.size]
    cts[rows, n] = sp[:rows.size]
    if B >= 2:
        cts[B - 1, :n] = np.uint64(1 << 63)
    if B >= 3:
        cts[B - 2, :n] = 0
    return cts


# ---- synthetic key words --------------------------------------------------------------------------------------
# edges of the load rounding (key_round16: nearest multiple of 2^16 of the signed word, ties up, wrapping at 2^127)
ROUND_EDGES = (1 << 15,            # rounds up to 2^16
               (1 << 15) - 1,      # rounds to 0
               (1 << 127) - 1,     # rounds up to 2^127 = -2^127
               U128,               # -1: rounds to 0
               1 << 127)           # -2^127, kept
TIE_WORD = 1 << 36                 # x (top digit m 2^19) = m 2^55: half of the decomposition's last kept bit
LIMB_BITS = (48, 16, 16, 16, 16)


def _planes(words, shape) -> np.ndarray:
    """Python-int words [polys][N] -> u64 planes [polys][lo, hi][N], flattened."""
    w = np.asarray(words, dtype=object).reshape(-1, shape[-1])
    lo = (w & U64).astype(np.uint64)
    hi = (w >> 64).astype(np.uint64)
    return np.stack([lo, hi], axis=1).reshape(-1)


def synthetic_key(sp, kind, seed) -> np.ndarray:
    """bsk words in the layout [i][c*L+l][j][lo, hi][N] that encrypt nothing:

    "ties": every polynomial has three monomials drawn from TIE_WORD and ROUND_EDGES, except (i = 0, row c = k,
        l = 0, j = 0), the single monomial TIE_WORD at a random degree.  With msg_modulus = 16 the first CMUX's
        difference words are multiples of 2^123, their only digits the top-level m 2^19, so accumulator 0 gains
        m 2^55 per coefficient: wherever the m of two coefficients differ in parity, the difference entering CMUX 2
        is an exact tie of the closest-representable rounding to 72 bits.  Every limb-0 value is at most 2^20 and at
        most 27 terms meet in a coefficient, so the low limb's products stay below 2^48: the small branch of
        f64_int_to_w128.
    "limb_edges": dense; after the rounding every limb of every word is at an end of its balanced range: limb 0 in
        {-2^47, 2^47 - 1}, limbs 1..3 in {-2^15, 2^15 - 1} (the ranges are half-open), the top remainder in
        {-2^15, 2^15 - 1, 2^15} (+2^15 only over a negative limb 3: otherwise the word would pass 2^127), signs random
        per coefficient and limb; the 16 bits below carry a random offset that rounds away.
    "uniform": uniformly random 128-bit words in every position, the bodies included."""
    rng = np.random.default_rng(seed)
    k, N, L = sp.k, sp.N, sp.level
    polys = sp.n * (k + 1) * L * (k + 1)
    if kind == "uniform":
        return rng.integers(0, 2 ** 64, size=polys * 2 * N, dtype=np.uint64)
    if kind == "ties":
        pool = (TIE_WORD,) + ROUND_EDGES
        w = np.zeros((polys, N), dtype=object)
        for p in range(polys):
            for t, c in zip(rng.choice(N, 3, replace=False), rng.integers(0, len(pool), 3)):
                w[p, t] = pool[c]
        # every word of the pool occurs in the first CMUX's live row (c = k, l = 0), all three outputs
        live = (k * L) * (k + 1)
        for j, words in ((1, pool[:3]), (2, pool[3:])):
            w[live + j] = 0
            for t, v in zip(rng.choice(N, 3, replace=False), words):
                w[live + j, t] = v
        w[live] = 0
        w[live, int(rng.integers(0, N))] = TIE_WORD
        return _planes(w, (polys, N))
    if kind == "limb_edges":
        neg = rng.integers(0, 2, size=(polys, N, 5)).astype(bool)
        rr = np.zeros((polys, N), dtype=object)
        shift = 0
        for t, bits in enumerate(LIMB_BITS):
            half = 1 << (bits - 1)
            if t < 4:
                lim = np.where(neg[:, :, t], -half, half - 1).astype(object)
            else:  # the remainder: +2^15 fits the signed 112 bits only when the limbs below sum to a negative value
                lim = np.where(neg[:, :, 4], -half, np.where(neg[:, :, 3], half, half - 1)).astype(object)
            rr = rr + lim * (1 << shift)
            shift += bits
        off = rng.integers(-(1 << 15), 1 << 15, size=(polys, N)).astype(object)
        return _planes((rr * 65536 + off) & U128, (polys, N))
    raise ValueError(kind)


def load_synthetic(okeys, bsk):
    """The oracle side of a synthetic key: the words replace the generated ones and the limb form is rebuilt
    (or_sns_bsk_round + or_sns_bsk_to_limb_ntt) on the next use."""
    okeys.bsk[:] = bsk
    okeys._bsk_limb = None
    return okeys


class KeyWords:
    """What Squasher.load_key reads of a key."""

    def __init__(self, bsk):
        self.bsk = bsk


# ---- the 72-bit decomposition, restated -----------------------------------------------------------------------
def digits72(y):
    """tfhe-rs SignedDecomposer on a 128-bit word (snsf::digits72, the oracle's decompose128): the closest multiple
    of 2^56 (half rounds up), then three balanced digits of 24 bits, d[0] most significant; a digit above 2^23, or
    equal to it over an odd rest, borrows 2^24 and carries one into the rest.  Returns (digits, carries)."""
    state = ((((y & U128) >> 55) + 1) >> 1) & ((1 << 72) - 1)
    d, carries = [0, 0, 0], [0, 0, 0]
    for l in (2, 1, 0):
        res = state & 0xFFFFFF
        state >>= 24
        carry = ((((res - 1) | state) & res) >> 23) & 1
        state += carry
        d[l], carries[l] = res - (carry << 24), carry
    return d, carries


def words128(planes) -> list:
    """(lo, hi) planes [2][N] -> Python ints [N]"""
    return [int(lo) | (int(hi) << 64) for lo, hi in zip(planes[0], planes[1])]


def tie_inputs(n=TIE_N, B=8, seed=0x7150) -> np.ndarray:
    """Ciphertext words for the "ties" key: random, the first mask word switched to 128 q + r with 0 < r < 128, so
    that the first CMUX's top digits take two neighbouring values m (one of them odd) along each LUT box."""
    rng = np.random.default_rng(seed)
    cts = rng.integers(0, 2 ** 64, size=(B, n + 1), dtype=np.uint64)
    a0 = 128 * rng.integers(0, 32, B) + rng.integers(1, 128, B)
    cts[:, 0] = (a0.astype(np.uint64) << np.uint64(52)) + rng.integers(0, 1 << 51, B, dtype=np.uint64)
    return cts


def cmux_differences(oracle_mod, osp, okeys, ct, lut, i):
    """Planes [k+1][lo, hi][N] of y = X^{a_i} acc - acc entering CMUX i + 1 (0-based mask word i): acc from the
    oracle's blind rotation over the first i mask words."""
    pre = copy.copy(osp)
    pre.n = i
    acc = oracle_mod.sns_blind_rotate(pre, okeys, np.concatenate([ct[:i], ct[-1:]]), lut)
    N = osp.N
    a = int(mod_switch_4096(ct[i]))
    out = np.zeros_like(acc)
    for c in range(acc.shape[0]):
        w = np.array(words128(acc[c]), dtype=object)
        t1 = (np.arange(N) - a) % (2 * N)
        rot = np.where(t1 >= N, (-w[t1 % N]) & U128, w[t1 % N])
        y = (rot - w) & U128
        out[c, 0] = (y & U64).astype(np.uint64)
        out[c, 1] = (y >> 64).astype(np.uint64)
    return out
