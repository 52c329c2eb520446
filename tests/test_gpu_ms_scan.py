"""The selection rule of the modulus-switch noise reduction (tfhe_amd/csrc/ms_reduce.hip) at constructed keys
and bounds: "first zero within the bound, else first strict minimiser, in index order", which the kernel
implements with ballots and a tile-wise early exit over 64 zeros per wave.

Every case is built from measures computed on the CPU by the oracle (or_ms_measure): rows of the real
1449-zero key are selected, reordered and duplicated into small keys, and the bound is placed strictly
between two computed measures, so the outcome each case is named for follows from the numbers.  build_cases()
also replays the rule over those measures to state the intended pick; tests/test_host.py asserts without a
GPU that or_ms_reduce alone gives that pick for every case.  Here the device's picks and ciphertexts must
equal or_ms_reduce's with the same explicit key (oracle.ms_key)."""
import functools

import numpy as np
import pytest

from conftest import KEY_SEED

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 129, 200)
POSITIONS = (0, 63, 64, 65, 127, 128)           # lane 0 / lane 63 of tiles 0 - 2; + count - 1 per key size
N_CT = 9


def _between(a, b):
    """A double strictly between two measures a < b."""
    m = a + (b - a) * 0.5
    assert a < m < b
    return m


def _replay(M_own, M_rows, bound):
    """The rule over given measures: own measure of the ciphertext, measures with each key row in index order."""
    best, pick = M_own, -1
    if best <= bound:
        return -1
    for z, m in enumerate(M_rows):
        if m < best:
            best, pick = m, z
            if best <= bound:
                break
    return pick


@functools.lru_cache(maxsize=None)
def build_cases():
    """-> (prm, list of cases); a case is dict(name, zeros [count][n+1], bound, cts [B][n+1], want [B]).
    CPU only: real keyswitch outputs and uniform rows as ciphertexts, the oracle's measures of each with each
    of the 1449 real zeros."""
    from oracle import oracle as O
    prm = O.params(1)
    ok = O.Keys(prm, KEY_SEED, with_bsk=False)
    dim = prm.n + 1
    rng = np.random.default_rng(0x5CA9)
    msgs = (np.arange(5, dtype=np.uint64) * 3 % 16) * np.uint64((1 << 63) // 16)
    cts = np.stack([O.keyswitch(prm, ok, c) for c in ok.encrypt(msgs, seed=0xC0FFEE71)] +
                   list(rng.integers(0, 2 ** 64 - 1, size=(N_CT - 5, dim), dtype=np.uint64, endpoint=True)))
    Z = ok.ms_zeros
    own = np.array([O.ms_measure(prm, ok, c) for c in cts])
    M = np.array([[O.ms_measure(prm, ok, c, z) for z in range(Z.shape[0])] for c in cts])
    zero_row = np.zeros(dim, dtype=np.uint64)
    cases = []

    def add(name, rows, bound, ct_idx, want):
        """rows: indices into Z, or -1 for an all-zero row"""
        rows = np.asarray(rows)
        zeros = np.where(rows[:, None] >= 0, Z[np.maximum(rows, 0)], zero_row[None, :])
        ct_idx = np.atleast_1d(ct_idx)
        # the intended picks must follow from the measures alone
        for q, w in zip(ct_idx, np.atleast_1d(want)):
            meas = [M[q, r] if r >= 0 else own[q] for r in rows]
            assert _replay(own[q], meas, bound) == w, (name, q)
        cases.append(dict(name=name, zeros=np.ascontiguousarray(zeros), bound=float(bound),
                          cts=np.ascontiguousarray(cts[ct_idx]), want=np.atleast_1d(want).astype(np.int64)))

    order = np.argsort(M, axis=1)                        # per ciphertext: rows by increasing measure
    for q in range(N_CT):
        assert len(set(M[q])) == M.shape[1]              # distinct measures: no accidental ties
        assert M[q, order[q, 1]] < own[q]                # the two best rows improve on the ciphertext alone

    def fill(q, count, seed, skip=2, above_own=False):
        """count rows for ciphertext q, none of its `skip` best, in a shuffled order"""
        pool = order[q, skip:]
        if above_own:
            pool = pool[M[q, pool] > own[q]]
        assert pool.size >= count
        return np.random.default_rng(seed).permutation(pool[:max(count, 256)])[:count]

    case_no = 0
    for count in COUNTS:
        for pos in sorted({p for p in POSITIONS + (count - 1,) if p < count}):
            q = case_no % N_CT
            case_no += 1
            r1, r2, r3 = order[q, :3]
            # the only zero within the bound at pos; everything else (r2 included) above it
            rows = fill(q, count, case_no, skip=1)
            rows[pos] = r1
            add(f"hit count={count} pos={pos}", rows, _between(M[q, r1], M[q, order[q, 1]]), q, pos)
            # no zero within the bound (r1 is not in the key; the bound lies between r1's and r2's measure):
            # full scan, the minimiser r2 at pos
            rows = fill(q, count, case_no + 1000)
            rows[pos] = r2
            add(f"min count={count} pos={pos}", rows, _between(M[q, r1], M[q, r2]), q, pos)

    for n, (i, j) in enumerate([(3, 40), (10, 70), (63, 64), (64, 127), (5, 199)]):
        q = n % N_CT
        r1, r2, r3 = order[q, :3]
        for tag, a, b in (("smaller first", r1, r2), ("smaller later", r2, r1)):
            rows = fill(q, 200, 2000 + n)
            rows[i], rows[j] = a, b
            add(f"two hits {tag} at {i},{j}", rows, _between(M[q, r2], M[q, r3]), q, i)
        rows = fill(q, 200, 2100 + n)
        rows[i] = rows[j] = r2                            # the minimising row twice, none within the bound
        add(f"duplicate minimiser at {i},{j}", rows, _between(M[q, r1], M[q, r2]), q, i)

    for q in (0, 6):
        r1, r2 = order[q, :2]
        lo = _between(M[q, r1], M[q, r2])                # below the ciphertext's own measure and every key row
        above = M[q][M[q] > own[q]].min()
        # already within the bound: untouched, although the key holds better rows
        rows = fill(q, 65, 3000 + q, skip=0)
        rows[0] = r1
        add(f"ciphertext within the bound ct={q}", rows, _between(own[q], above), q, -1)
        # all-zero rows: every measure equals the ciphertext's own, nothing is strictly better
        for count in (1, 64, 65):
            add(f"all-zero key count={count} ct={q}", [-1] * count, lo, q, -1)
        # every row worse than the ciphertext alone, all-zero rows (equal) in both tiles
        rows = fill(q, 130, 3100 + q, above_own=True)
        rows[[0, 63, 64, 129]] = -1
        add(f"no strict improvement ct={q}", rows, lo, q, -1)

    # batches of 1, 5, 9 on one 200-row key: ciphertexts that stop in tile 0, in tile 2, and never
    flat = np.sort(M.reshape(-1))
    kq = flat.size // 300
    T = _between(flat[kq], flat[kq + 1])
    assert (own > T).all()
    stop0, stop2, never = (0, 3, 6), (1, 4, 7), (2, 5, 8)
    within = M <= T
    clean = ~within.any(axis=0)                           # rows above the bound for every ciphertext
    rows = np.random.default_rng(4000).permutation(np.flatnonzero(clean))[:200]
    for qs, places in ((stop0, (0, 17, 63)), (stop2, (128, 150, 191))):
        for q, pos in zip(qs, places):
            cand = [r for r in np.flatnonzero(within[q]) if within[:, r].sum() == 1]
            assert cand, q                                # a row within the bound for ciphertext q alone
            rows[pos] = cand[0]
    want_all = np.array([_replay(own[q], M[q, rows], T) for q in range(N_CT)])
    assert all(0 <= want_all[q] < 64 for q in stop0) and all(128 <= want_all[q] < 192 for q in stop2)
    assert not within[np.ix_(never, rows)].any()
    for B in (1, 5, 9):
        idx = np.arange(1, 1 + B) % N_CT          # B = 1: a tile-2 stop; 5: tile 2, never, tile 0, tile 2, never
        add(f"mixed batch B={B}", rows, T, idx, want_all[idx])
    return prm, cases


def check_oracle_picks():
    """CPU-side: or_ms_reduce alone, with each case's explicit key, gives the intended picks."""
    from oracle import oracle as O
    prm, cases = build_cases()
    assert len(cases) > 60
    for c in cases:
        red, picks = O.ms_reduce(prm, None, c["cts"], ms=O.ms_key(c["zeros"], c["bound"]))
        assert np.array_equal(picks, c["want"]), c["name"]
        for i, p in enumerate(picks):
            with np.errstate(over="ignore"):
                assert np.array_equal(red[i], c["cts"][i] + c["zeros"][p] if p >= 0 else c["cts"][i]), c["name"]
    return prm, cases


def _kinds():
    return ("hit", "min", "two hits", "duplicate", "ciphertext within", "all-zero", "no strict", "mixed")


@pytest.mark.parametrize("kind", _kinds())
def test_ms_scan_vs_oracle(fhevm_engine, fhevm_keys, oracle_mod, kind):
    """Each case with its own load_ms_key(zeros, bound): picks and output ciphertexts equal or_ms_reduce's."""
    prm, cases = build_cases()
    mine = [c for c in cases if c["name"].startswith(kind)]
    assert mine
    try:
        for c in mine:
            ref, rpicks = oracle_mod.ms_reduce(prm, None, c["cts"], ms=oracle_mod.ms_key(c["zeros"], c["bound"]))
            assert np.array_equal(rpicks, c["want"]), c["name"]
            fhevm_engine.load_ms_key(c["zeros"], c["bound"])
            out, picks = fhevm_engine.ms_reduce(c["cts"])
            assert np.array_equal(picks, rpicks), f"{c['name']}: device {picks.tolist()} oracle {rpicks.tolist()}"
            assert np.array_equal(out, ref), c["name"]
    finally:
        fhevm_engine.load_ms_key(fhevm_keys[1].ms_zeros)     # the session engine is shared
