"""Many-LUT PBS on CPU: the LUT builder (tfhe_amd.lut_many) and the radix layer's opt-in use of it
(RadixCircuit(many_lut=True)) with a cleartext double of both bootstrap forms.  The double's many-LUT
bootstrap asserts the caller's guarantee (every input < SPACE / n_fn).  The MI355X run is
tests/test_gpu_many_lut.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import radix as R


# ---- lut_many ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1024, 2048])
@pytest.mark.parametrize("n_fn", [1, 2, 4])
def test_lut_many_is_lut_from_table_of_the_concatenation(N, n_fn):
    rng = np.random.default_rng(100 * n_fn + N)
    per = R.SPACE // n_fn
    tables = [[int(v) for v in rng.integers(0, R.SPACE, per)] for _ in range(n_fn)]
    lut, stride = tfhe_amd.lut_many(N, R.SPACE, tables, R.DELTA)
    assert stride == N // n_fn
    flat = [v for t in tables for v in t]
    assert np.array_equal(lut, tfhe_amd.lut_from_table(N, R.SPACE, flat, R.DELTA))


def test_lut_many_rejects_bad_shapes():
    t8 = list(range(8))
    with pytest.raises(ValueError):
        tfhe_amd.lut_many(2048, 16, [], R.DELTA)
    with pytest.raises(ValueError):                      # n_fn = 3: not a power of two
        tfhe_amd.lut_many(2048, 16, [t8[:5], t8[:5], t8[:6]], R.DELTA)
    with pytest.raises(ValueError):                      # n_fn = 8 does not divide msg_modulus = 4
        tfhe_amd.lut_many(2048, 4, [[0]] * 8, R.DELTA)
    with pytest.raises(ValueError):                      # tables of 16 entries where 8 are due
        tfhe_amd.lut_many(2048, 16, [list(range(16)), list(range(16))], R.DELTA)
    with pytest.raises(ValueError):                      # one table short
        tfhe_amd.lut_many(2048, 16, [t8, t8[:7]], R.DELTA)


# ---- radix layer ---------------------------------------------------------------------------------------
class CleartextCircuit(R.RadixCircuit):
    """Evaluates the tables on trivial blocks (mask width 2: only the body matters)."""

    def __init__(self, many_lut=None):
        eng = SimpleNamespace(params=SimpleNamespace(k=1, N=2, n=918, order=1))
        if many_lut is None:
            super().__init__(eng)            # the constructor as every existing caller uses it
        else:
            super().__init__(eng, many_lut=many_lut)
        self.many_calls = 0

    def _values(self, flat):
        assert not flat[:, :-1].any(), "trivial blocks only"
        assert np.all(flat[:, -1] % np.uint64(R.DELTA) == 0)
        return (flat[:, -1] // np.uint64(R.DELTA)).astype(np.int64)

    def _pbs(self, flat, tables, idx):
        v = self._values(flat)
        assert v.max(initial=0) < R.SPACE
        return self.trivial(np.array([tables[i][x] for i, x in zip(idx, v)], dtype=np.uint64))

    def _pbs_many(self, flat, table_groups, idx, n_fn):
        v = self._values(flat)
        assert v.max(initial=0) < R.SPACE // n_fn, f"many-LUT input {v.max()} outside 1/{n_fn} of the space"
        assert all(len(g) == n_fn and all(len(t) == R.SPACE // n_fn for t in g) for g in table_groups)
        self.many_calls += 1
        out = np.array([[table_groups[i][f][x] for f in range(n_fn)] for i, x in zip(idx, v)], dtype=np.uint64)
        return self.trivial(out.reshape(len(v), n_fn))


class ClearKey:
    def decrypt(self, cts, mm):
        return (np.asarray(cts)[..., -1] // np.uint64(R.DELTA)) % np.uint64(mm)


def propagate_rotations(B, nb):
    """Blind rotations of one g_propagate today: two tables on every block sum, the Kogge-Stone merges, the
    final carry application."""
    total, d = 2 * B * nb, 1
    while d < nb:
        total += B * (nb - d)
        d *= 2
    return total + (B * (nb - 1) if nb > 1 else 0)


def operands(w, B=5):
    rng = np.random.default_rng(w)
    top = (1 << w) - 1
    a = [top, 0, top, 1] + [int(x) for x in rng.integers(0, 1 << min(w, 62), B)]
    b = [1, 1, top, top] + [int(x) for x in rng.integers(0, 1 << min(w, 62), B)]
    return a, b


def run(op, w, many_lut, a, b=None):
    c = CleartextCircuit(many_lut)
    x = R.RadixUint.trivial(c, a, w)
    y = R.RadixUint.trivial(c, b, w) if b is not None else None
    r = c.run(R.fhevm_op(c, op, x, y))
    return c, [int(v) for v in r.decrypt(ClearKey())]


@pytest.mark.parametrize("w", [8, 64])
@pytest.mark.parametrize("op", ["add", "sub", "neg", "mul"])
def test_radix_many_lut(op, w):
    a, b = operands(w)
    B, nb, mod = len(a), w // 2, 1 << w
    expect = {"add": [(x + y) % mod for x, y in zip(a, b)], "sub": [(x - y) % mod for x, y in zip(a, b)],
              "neg": [(-x) % mod for x in a], "mul": [(x * y) % mod for x, y in zip(a, b)]}[op]
    rhs = None if op == "neg" else b
    c0, r0 = run(op, w, None, a, rhs)
    c1, r1 = run(op, w, True, a, rhs)
    c2, r2 = run(op, w, False, a, rhs)
    assert r0 == expect and r1 == expect and r2 == expect
    # the default is today's circuit: no many-LUT call, and for the single-propagate operators today's counts
    assert c0.many_calls == 0 and c2.many_calls == 0
    assert (c2.pbs_count, c2.launches) == (c0.pbs_count, c0.launches)
    if op != "mul":
        assert c0.pbs_count == propagate_rotations(B, nb)
    # many_lut merges the two first-level tables of the propagate: every block without carry-in (add, the
    # final add of mul), every block but the lowest with it (sub, neg)
    merged = B * nb if op in ("add", "mul") else B * (nb - 1)
    assert c1.many_calls >= 1
    assert c1.pbs_count == c0.pbs_count - merged
    assert c1.launches == c0.launches


def test_euint64_add_rotation_count():
    c0, _ = run("add", 64, None, [1], [2])
    c1, _ = run("add", 64, True, [1], [2])
    assert c0.pbs_count == 64 + 129 + 31 == 224
    assert c1.pbs_count == 192


def test_add_with_carry_in_keeps_block0_on_two_tables():
    w, B = 8, 3
    nb = w // 2
    c = CleartextCircuit(True)
    top = R.RadixUint.trivial(c, [(1 << w) - 1] * B, w).blocks
    out = c.run(R.g_propagate(c, R._add(top, top), True))                       # block sums 6, block 0: 6 + 1
    got = R.RadixUint(c, out).decrypt(ClearKey())
    assert [int(v) for v in got] == [(2 * ((1 << w) - 1) + 1) % (1 << w)] * B
    # block 0 is not merged, whatever its value
    assert c.pbs_count == propagate_rotations(B, nb) - B * (nb - 1)


def test_mixed_level_groups_by_n_fn():
    """One level with ordinary entries, 2-function and 4-function entries: one _pbs_many call per n_fn."""
    c = CleartextCircuit(True)
    v2 = c.trivial(np.arange(8, dtype=np.uint64))
    v4 = c.trivial(np.arange(4, dtype=np.uint64).reshape(2, 2))
    v1 = c.trivial(np.arange(16, dtype=np.uint64))
    t2 = (tuple(range(8)), tuple(15 - i for i in range(8)))
    t4 = tuple(tuple((i + 4 * f) % 16 for i in range(4)) for f in range(4))
    res = c.bootstrap([(v2, t2), (v1, R.T_MSG), (v4, t4), (v2, R.T_MSG_STATE)])
    ck = ClearKey()
    assert len(res) == 4 and len(res[0]) == 2 and len(res[2]) == 4 and len(res[3]) == 2
    assert [int(x) for x in ck.decrypt(res[0][1], 16)] == [15 - i for i in range(8)]
    assert [int(x) for x in ck.decrypt(res[1], 16)] == [i % 4 for i in range(16)]
    assert res[2][3].shape == (2, 2, c.dim)
    assert [int(x) for x in ck.decrypt(res[2][3], 16).reshape(-1)] == [12, 13, 14, 15]
    assert [int(x) for x in ck.decrypt(res[3][1], 16)] == list(R.T_STATE[:8])
    assert c.many_calls == 2 and c.launches == 1 and c.pbs_count == 8 + 16 + 4 + 8
