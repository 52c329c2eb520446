"""The resident radix executor (tfhe_amd/radix.py: LinBlocks, RadixCircuit(device=...)) on CPU: the lazy block
algebra against eager numpy, and device="cpu" circuits (the same executor over numpy buffers, assembled by
lincomb_ref) against the eager host mode with the cleartext double of tests/test_radix.py.  The MI355X runs are
tests/test_gpu_lincomb.py and tests/test_gpu_radix_resident.py."""
from types import SimpleNamespace

import numpy as np
import pytest

from tfhe_amd import radix as R
from test_radix import CleartextRadixCircuit, ClearKey, kat_op, supported, _w


class ResidentCleartextCircuit(CleartextRadixCircuit):
    """The cleartext double as a device="cpu" circuit.  The double answers with trivial blocks, which a resident
    circuit builds lazily: a bootstrap's output is a buffer, so they are materialised here."""

    def __init__(self, N=2048, many_lut=False):
        super().__init__(N)
        R.RadixCircuit.__init__(self, self.engine, many_lut=many_lut, device="cpu")
        self.max_seen = 0

    def _pbs(self, flat, tables, idx):
        return np.asarray(super()._pbs(flat, tables, idx))


def host_blocks(r):
    """A result (RadixUint or an encrypted bool block array) as the host array of its ciphertext words."""
    return r.to_host() if isinstance(r, R.RadixUint) else np.asarray(r)


# ---- 1. the algebra ---------------------------------------------------------------------------------------------
DIM = 5
COEFS = (0, 1, 4, 1 << 63, (1 << 64) - 1, 0x9E3779B97F4A7C15)


def _circuits():
    eng = SimpleNamespace(params=SimpleNamespace(k=1, N=DIM - 1, n=3, order=1))
    return R.RadixCircuit(eng, device="cpu"), R.RadixCircuit(eng)


def _unary_ops(rng, shape):
    """(name, f(c, x)) choices for an array of this shape; the same f runs on the lazy and on the eager array."""
    lead = shape[:-1]
    ops = [("scale", lambda c, x, k=COEFS[rng.integers(len(COEFS))]: R._scale(x, k)),
           ("not", lambda c, x: R._not(c, x)),
           ("add_const", lambda c, x, v=int(rng.integers(16)): R._add(x, R._const(c, x.shape[:-1], v))),
           ("copy", lambda c, x: x.copy()),
           ("self_add", lambda c, x: R._add(x, x, x))]
    for ax, n in enumerate(lead):
        s = int(rng.integers(-n, n + 1))
        ops.append((f"roll{ax}", lambda c, x, ax=ax, s=s: np.roll(x, s, axis=ax)))
        if n >= 2:
            lo, step = int(rng.integers(0, n - 1)), int(rng.integers(1, 3))
            key = (slice(None),) * ax + (slice(lo, None, step),)
            ops.append((f"slice{ax}", lambda c, x, key=key: x[key]))
            ops.append((f"neg_slice{ax}", lambda c, x, ax=ax: x[(slice(None),) * ax + (slice(None, -1),)]))
            ops.append((f"bcast{ax}", lambda c, x, ax=ax: np.broadcast_to(
                x[(slice(None),) * ax + (slice(0, 1),)], x.shape)))
    if len(lead) >= 2:
        j = int(rng.integers(lead[1]))
        ops.append(("pick", lambda c, x, j=j: x[:, j]))
        ops.append(("pick_none", lambda c, x, j=j: x[:, j][:, None]))
        ops.append(("pick_none_full", lambda c, x, j=j: x[:, None, j, :]))
        ops.append(("ellipsis", lambda c, x, j=j: x[j % lead[0], ...]))
    if len(lead) == 1:
        ops.append(("lift", lambda c, x: np.broadcast_to(x[:, None, :], (x.shape[0], 3, x.shape[1]))))
        ops.append(("reshape", lambda c, x: x.reshape(1, -1, x.shape[-1])))
    return ops


def _assign(c, x, y):
    """the carry-in idiom of g_propagate: s = s.copy(); s[:, 0] = ..."""
    s = x.copy()
    if x.ndim >= 3:
        s[:, 0] = R._add(y[:, 0], R._const(c, (y.shape[0],) + y.shape[2:-1], 1))
    else:
        s[0] = y[-1]
    return s


BINARY_OPS = [("add", lambda c, x, y: R._add(x, y)),
              ("pack", lambda c, x, y: R._pack(x, y)),
              ("sub", lambda c, x, y: R._sub(x, y)),
              ("cat0", lambda c, x, y: np.concatenate([x, y], axis=0)),
              ("cat_last_lead", lambda c, x, y: np.concatenate([x, y, x], axis=x.ndim - 2)),
              ("stack1", lambda c, x, y: np.stack([x, y], axis=1)),
              ("assign", _assign)]


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_linblocks_algebra_matches_eager_numpy(seed):
    rng = np.random.default_rng(seed)
    c_lazy, c_eager = _circuits()
    bufs = [rng.integers(0, 1 << 64, (4, 6, DIM), dtype=np.uint64), rng.integers(0, 1 << 64, (4, 6, DIM), dtype=np.uint64),
            rng.integers(0, 1 << 64, (6, DIM), dtype=np.uint64)]
    pool = [(c_lazy.wrap(b), b) for b in bufs]
    pool.append((c_lazy.wrap(bufs[0])[:, :, :], bufs[0]))  # the same words through a second buffer id
    trail = []
    for step in range(70):
        i = int(rng.integers(len(pool)))
        lazy, eager = pool[i]
        same = [p for p in pool if p[1].shape == eager.shape]
        if rng.integers(3) == 0 and eager.ndim <= 3:
            name, f = BINARY_OPS[rng.integers(len(BINARY_OPS))]
            l2, e2 = same[rng.integers(len(same))]
            new = (f(c_lazy, lazy, l2), f(c_eager, eager, e2))
        else:
            ops = _unary_ops(rng, eager.shape)
            name, f = ops[rng.integers(len(ops))]
            new = (f(c_lazy, lazy), f(c_eager, eager))
        trail.append(name)
        assert isinstance(new[0], R.LinBlocks), trail
        assert new[0].shape == new[1].shape, trail
        if 0 not in new[1].shape:
            pool.append(new)
    assert len(set(trail)) >= 12, "the walk exercised too few operations"
    for k, (lazy, eager) in enumerate(pool):
        got = lazy.materialize()
        assert got.dtype == np.uint64 and got.shape == eager.shape
        np.testing.assert_array_equal(got, eager, err_msg=f"pool entry {k} after {trail[:max(k - 3, 0)][-6:]}")
    # the sources were never written
    np.testing.assert_array_equal(pool[0][0].materialize(), bufs[0])


def test_linblocks_refuses_what_would_touch_words():
    c_lazy, _ = _circuits()
    x = c_lazy.wrap(np.arange(2 * 3 * DIM, dtype=np.uint64).reshape(2, 3, DIM))
    with pytest.raises(IndexError):
        x[:, :, 1:]
    with pytest.raises(IndexError):
        x[..., -1]
    with pytest.raises(ValueError):
        np.concatenate([x, x], axis=-1)
    with pytest.raises(ValueError):
        np.roll(x, 1, axis=2)
    with pytest.raises(TypeError):
        np.concatenate([x, np.zeros((2, 3, DIM), dtype=np.uint64)], axis=0)
    with pytest.raises(ValueError):
        c_lazy.wrap(np.zeros((2, DIM + 1), dtype=np.uint64))
    assert c_lazy.trivial([1, 2]).materialize().tolist() == [[0] * (DIM - 1) + [R.DELTA], [0] * (DIM - 1) + [2 * R.DELTA]]


def test_lincomb_ref_small_case():
    b0 = np.array([[1, 2, 3], [10, 20, 30]], dtype=np.uint64)
    b1 = np.array([[7, 7, 7]], dtype=np.uint64)
    out = R.lincomb_ref([b0, b1], [0, 2, 2, 5], [0, 1, 0, 0, 1], [1, 0, 0, 0, 0], [4, 1, 1, (1 << 64) - 1, 1 << 63],
                        [5, 9, 0], 3)
    m = 1 << 64
    want = [[47, 87, 127 + 5], [0, 0, 9], [(1 - 1 + 7 * (1 << 63)) % m, (2 - 2 + 7 * (1 << 63)) % m, (3 - 3 + 7 * (1 << 63)) % m]]
    assert out.tolist() == want
    assert R.lincomb_ref([], [0], [], [], [], None, 3).shape == (0, 3)


def test_resident_circuit_refuses_a_sharded_engine():
    pytest.importorskip("torch")
    eng = SimpleNamespace(params=SimpleNamespace(k=1, N=4, n=3, order=1), devices=[0, 1])
    with pytest.raises(ValueError):
        R.RadixCircuit(eng, device="cuda:0")


# ---- 2. the reference KATs ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kats():
    from conftest import load_kats
    return [k for k in load_kats() if supported(k)]


def test_radix_kats_resident_cpu_equal_eager(kats):
    assert len(kats) == 2394
    eager, lazy = CleartextRadixCircuit(N=2), ResidentCleartextCircuit(N=2)
    want = eager.run_many([kat_op(eager, k) for k in kats])
    got = lazy.run_many([kat_op(lazy, k) for k in kats])
    bad = [(k["source"], k["op"], k["args"]) for k, w, g in zip(kats, want, got)
           if not np.array_equal(host_blocks(w), host_blocks(g))]
    assert not bad, (len(bad), bad[:5])
    assert all(isinstance(g.blocks if isinstance(g, R.RadixUint) else g, R.LinBlocks) for g in got)
    ck = ClearKey()
    wrong = [(k["op"], k["args"]) for k, g in zip(kats, got)
             if (int(ck.decrypt(host_blocks(g), R.SPACE)[0]) != int(bool(k["expect"])) if k["result_type"] == "ebool"
                 else int(g.decrypt(ck)[0]) != k["expect"] or g.width != _w(k["result_type"]))]
    assert not wrong, wrong[:5]
    assert (lazy.pbs_count, lazy.launches) == (eager.pbs_count, eager.launches)
    assert lazy.max_seen <= 15 and eager.max_seen <= 15
    # the widest rows are g_sum_columns' groups of five clean blocks
    assert lazy.max_terms == 5


# ---- 3. random batches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [8, 32])
def test_radix_random_batch_resident_cpu(w):
    rng = np.random.default_rng(w)
    B = 24
    a = rng.integers(0, 1 << w, B, dtype=np.uint64)
    b = rng.integers(0, 1 << w, B, dtype=np.uint64)
    b[:4] = a[:4]
    a[4:6] = [0, (1 << w) - 1]
    s = rng.integers(0, 1 << w, B, dtype=np.uint64)
    s[:3] = [0, 1, w - 1]
    c = ResidentCleartextCircuit(N=4)
    ck = ClearKey()
    A, Bv, S = (R.RadixUint.trivial(c, v, w) for v in (a, b, s))
    m = (1 << w) - 1
    M = np.uint64(m)
    ops = ["add", "sub", "xor", "and", "or", "lt", "le", "gt", "ge", "eq", "ne", "min", "max", "neg", "not", "mul"]
    res = c.run_many([R.fhevm_op(c, op, A, None if op in ("neg", "not") else Bv) for op in ops])
    want = {"add": (a + b) & M, "sub": (a - b) & M, "xor": a ^ b, "and": a & b, "or": a | b, "lt": a < b, "le": a <= b,
            "gt": a > b, "ge": a >= b, "eq": a == b, "ne": a != b, "min": np.minimum(a, b), "max": np.maximum(a, b),
            "neg": (np.uint64(0) - a) & M, "not": ~a & M, "mul": (a * b) & M}
    for op, r in zip(ops, res):
        if op in ("lt", "le", "gt", "ge", "eq", "ne"):
            assert isinstance(r, R.LinBlocks)
            got = ck.decrypt(np.asarray(r), R.SPACE).astype(bool)
        else:
            assert isinstance(r.blocks, R.LinBlocks)
            got = r.decrypt(ck)
        np.testing.assert_array_equal(got, want[op], err_msg=op)

    def shifted(kind, x, k):
        k %= w
        return {"shl": (x << k) & m, "shr": x >> k, "rotl": ((x << k) | (x >> (w - k))) & m,
                "rotr": ((x >> k) | (x << (w - k))) & m}[kind]

    kinds = ("shl", "shr", "rotl", "rotr")
    res = c.run_many([R.fhevm_op(c, kind, A, k) for k in (0, 1, 5, 13, 31) for kind in kinds])
    for (k, kind), r in zip(((k, kind) for k in (0, 1, 5, 13, 31) for kind in kinds), res):
        np.testing.assert_array_equal(r.decrypt(ck), np.array([shifted(kind, int(x), k) for x in a], dtype=np.uint64),
                                      err_msg=f"{kind} {k}")
    res = c.run_many([R.fhevm_op(c, kind, A, S) for kind in kinds])
    for kind, r in zip(kinds, res):
        np.testing.assert_array_equal(r.decrypt(ck), np.array([shifted(kind, int(x), int(k)) for x, k in zip(a, s)],
                                                              dtype=np.uint64), err_msg=f"{kind} by an encrypted amount")
    divisors = [7, 32, 0, 550954323]
    res = c.run_many([R.fhevm_op(c, op, A, d) for d in divisors for op in ("div", "rem")])
    for t, d in enumerate(divisors):
        d %= 1 << w
        wq = np.full_like(a, m) if d == 0 else a // np.uint64(d)
        wr = a if d == 0 else a % np.uint64(d)
        np.testing.assert_array_equal(res[2 * t].decrypt(ck), wq, err_msg=f"div {d}")
        np.testing.assert_array_equal(res[2 * t + 1].decrypt(ck), wr, err_msg=f"rem {d}")
    assert c.max_seen <= 15
    assert c.max_terms <= 5


def test_rand_and_many_lut_resident_cpu():
    """g_rand* through the overridable _oprf, and a many-LUT level through _pbs_many, both over numpy buffers."""
    class C(ResidentCleartextCircuit):
        def _oprf(self, seeds, bit_kinds, idx):
            return np.asarray(self.trivial([(1 << bit_kinds[i]) - 1 for i in idx]))

        def _pbs_many(self, flat, table_groups, idx, n_fn):
            v = (flat[:, -1] // np.uint64(R.DELTA)).astype(np.int64)
            assert v.max(initial=0) < R.SPACE // n_fn
            return np.asarray(self.trivial([[table_groups[i][f][x] for f in range(n_fn)] for i, x in zip(idx, v)]))

    c = C(N=4, many_lut=True)
    ck = ClearKey()
    r = R.RadixUint.rand_bounded(c, [[1, 2], [3, 4]], 8, 32)
    assert isinstance(r.blocks, R.LinBlocks) and r.blocks.shape == (2, 4, c.dim)
    assert r.decrypt(ck).tolist() == [31, 31]
    assert R.RadixUint.rand(c, [5, 6], 8).decrypt(ck).tolist() == [255]
    assert int(ck.decrypt(np.asarray(c.run(R.fhevm_rand(c, "rand", [5, 6], 1))), R.SPACE)[0]) == 1
    a, b = np.array([200, 17, 255], dtype=np.uint64), np.array([100, 240, 1], dtype=np.uint64)
    A, Bv = R.RadixUint.trivial(c, a, 8), R.RadixUint.trivial(c, b, 8)
    add, sub = c.run_many([R.fhevm_op(c, "add", A, Bv), R.fhevm_op(c, "sub", A, Bv)])
    assert add.decrypt(ck).tolist() == [44, 1, 0] and sub.decrypt(ck).tolist() == [100, 33, 254]
