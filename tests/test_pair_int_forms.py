"""Integer forms of the pair kernel's rotation and top-level digit (pbs_fft.hip rotate_states, decomp_top),
restated in numpy and checked against the forms they replace and against the oracle's signed decomposer.

(a) The rotation difference y = (x ^ M) - (v + M), M = 0 or all ones, taken as the complement of a sum:
    S = (x ^ ~M) + (v + M), y = ~S, so decomp_state(y) = (hi(y) + 1024) >> 11 = (1023 - hi(S)) >> 11 in 32-bit words.
(b) The top-level digit st - ((st + 63) & ~127) as -sext7(-st) for the reachable top states 0 <= st <= 128.
"""
import numpy as np

U64 = np.uint64
MASK32 = (1 << 32) - 1
ONES = U64(2**64 - 1)


def _hi(x):
    return (x >> U64(32)).astype(np.uint32)


def _state_sub(x, v, M):
    """The subtracting form: decomp_state((x ^ M) - (v + M)), 64-bit wrap-around, 32-bit high word."""
    return (_hi((x ^ M) - (v + M)) + np.uint32(1024)) >> np.uint32(11)


def _state_add(x, v, M):
    """The adding form: (1023 - hi((x ^ ~M) + (v + M))) >> 11."""
    return (np.uint32(1023) - _hi((x ^ ~M) + (v + M))) >> np.uint32(11)


def _check(x, v):
    with np.errstate(over="ignore"):
        for M in (U64(0), ONES):
            a, s = _state_add(x, v, M), _state_sub(x, v, M)
            assert np.array_equal(a, s), f"M = {int(M):#x}: first mismatches at {np.flatnonzero(a != s)[:5]}"
            # the identity itself in all 64 bits: the low-word carry is exact, not approximated
            assert np.array_equal(~((x ^ ~M) + (v + M)), (x ^ M) - (v + M))


def test_rotation_sum_form_random_pairs():
    rng = np.random.default_rng(0x1D7)
    _check(rng.integers(0, 2**64, 1_000_000, dtype=U64), rng.integers(0, 2**64, 1_000_000, dtype=U64))


def test_rotation_sum_form_operand_edge_grid():
    """Operand words: high words 0, 2^32 - 1 and within +-1 of rounding boundaries, low words 0, 1, 2^32 - 1 in every
    combination, and equal low words."""
    his = {0, 1, MASK32 - 1, MASK32}
    for k in (0, 1, 2, 1 << 9, (1 << 20) - 1, 1 << 20, (1 << 21) - 2, (1 << 21) - 1):
        for b in (1023, 1024):
            his.update((2048 * k + b + d) & MASK32 for d in (-1, 0, 1))
    h = np.array(sorted(his), dtype=U64) << U64(32)
    hx, hv = (g.ravel() for g in np.meshgrid(h, h, indexing="ij"))
    xs, vs = [], []
    for lx in (0, 1, MASK32):
        for lv in (0, 1, MASK32):
            xs.append(hx | U64(lx))
            vs.append(hv | U64(lv))
    lo = np.random.default_rng(0x1D8).integers(0, 2**32, hx.size, dtype=U64)
    xs.append(hx | lo)
    vs.append(hv | lo)
    _check(np.concatenate(xs), np.concatenate(vs))


def test_rotation_sum_form_every_rounding_boundary():
    """The difference's high word within +-1 of EVERY rounding boundary (2048 k + 1023 | 1024, all 2^21 k), for both
    signs: x is built from a random v so that (x ^ M) - (v + M) is the wanted word; the low words of v and of the
    difference cycle through 0, 1, 2^32 - 1 and random values (a zero low difference gives equal low words)."""
    rng = np.random.default_rng(0x1D9)
    k = np.arange(1 << 21, dtype=U64) * U64(2048)
    dh = np.concatenate([(k + U64(b)) & U64(MASK32) for b in (1022, 1023, 1024, 1025)])
    n = dh.size

    def lows(phase):
        lo = rng.integers(0, 2**32, n, dtype=U64)
        sel = (np.arange(n) + phase) % 5
        lo[sel == 0] = 0
        lo[sel == 1] = 1
        lo[sel == 2] = MASK32
        return lo

    with np.errstate(over="ignore"):
        d = (dh << U64(32)) | lows(0)
        v = (rng.integers(0, 2**32, n, dtype=U64) << U64(32)) | lows(np.arange(n) // 5)
        for M in (U64(0), ONES):
            x = (d + (v + M)) ^ M  # (x ^ M) - (v + M) = d
            assert np.array_equal((x ^ M) - (v + M), d)
            assert np.array_equal(_state_add(x, v, M), _state_sub(x, v, M))
            assert np.array_equal(_state_sub(x, v, M), (_hi(d) + np.uint32(1024)) >> np.uint32(11))


def _sext7(t):
    t = np.asarray(t, dtype=np.int64) & 127
    return t - ((t & 64) << 1)


def _top_new(st):
    return -_sext7(-np.asarray(st, dtype=np.int64))


def test_top_digit_form_on_every_reachable_state():
    st = np.arange(0, 129, dtype=np.int64)
    assert np.array_equal(_top_new(st), st - ((st + 63) & ~np.int64(127)))
    assert _top_new(st).min() == -63 and _top_new(st).max() == 64


def test_digit_chain_with_new_top_form_equals_signed_decomposer(oracle_mod):
    """As test_fft.py's test_device_decomposition_steps_equal_signed_decomposer, with the top level as -sext7(-st):
    equal to the tfhe-rs SignedDecomposer rule for every 21-bit state and 2^21 itself (exhaustive, numpy), and to
    or_decompose on sampled and edge torus values."""
    V = np.arange((1 << 21) + 1, dtype=np.int64)

    def sequential(st):
        out = []
        for _ in range(3):
            res = st & 127
            st = st >> 7
            carry = ((((res - 1) | st) & res) >> 6) & 1
            st = st + carry
            out.append(res - (carry << 7))
        return out

    def steps(st):
        out = []
        for _ in range(2):
            b = (st >> 13) & 1
            W = st + 63 + b
            out.append((W & 127) - 63 - b)
            st = W >> 7
        assert st.min() >= 0 and st.max() <= 128  # the reachable top states
        out.append(_top_new(st))
        return out

    assert all(np.array_equal(a, b) for a, b in zip(sequential(V), steps(V)))
    rng = np.random.default_rng(8)
    xs = [int(x) for x in rng.integers(0, 2**64, 3000, dtype=np.uint64)]
    xs += [0, 2**64 - 1, 2**63, 2**42, 2**42 - 1, 2**64 - 2**42, 2**64 - 2**42 - 1]       # states 0, 2^21, 2^20, 1, 0
    xs += [(s << 43) + o for s in (63, 64, 65, (1 << 14) - 1, 1 << 14, (64 << 14) - 1, 64 << 14, (1 << 21) - 1)
           for o in (-(1 << 42) - 1, -(1 << 42), 0, (1 << 42) - 1, 1 << 42)]
    for x in xs:
        x %= 2**64
        st = np.array([(((x >> 32) + 1024) % 2**32) >> 11], dtype=np.int64)  # the device's decomp_state
        lv = [int(v[0]) for v in steps(st)]  # least significant first
        assert lv[::-1] == oracle_mod.decompose(x, 7, 3), hex(x)
