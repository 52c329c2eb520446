"""The lockstep level executor shared by the gate circuits (tfhe_amd/integer.py) and the radix circuits
(tfhe_amd/radix.py), on CPU: where a level is cut into engine calls, how a mixed level is grouped, how coroutines are
stepped, and the ``lut_index`` argument of the three host entry points of ``Engine`` that take one.  Everything goes
through the overridable seams (``_pbs`` / ``_pbs_many`` / ``_oprf``) or a recording engine, with the cleartext
doubles of tests/test_radix.py, tests/test_many_lut.py and tests/test_integer.py."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import integer as I
from tfhe_amd import radix as R
from test_integer import CleartextTorchEngine
from test_integer import ClearKey as BitKey
from test_many_lut import CleartextCircuit, ClearKey

MODES = [None, "cpu"]
T_INC = R._table(lambda v: v + 1)
T_DBL = R._table(lambda v: 2 * v)
G2A = (tuple(range(8)), tuple(7 - i for i in range(8)))
G2B = (tuple((3 * i) % 16 for i in range(8)), tuple((i + 5) % 16 for i in range(8)))
G4 = tuple(tuple((i + 4 * f) % 16 for i in range(4)) for f in range(4))


class Recorder(CleartextCircuit):
    """The cleartext double in host mode or as a device="cpu" circuit; every call of a seam is noted as
    (seam, rows, tables, idx) before the double answers.  A resident circuit takes buffers back, so the double's
    trivial blocks are materialised."""

    def __init__(self, device=None):
        super().__init__(True)
        if device is not None:
            R.RadixCircuit.__init__(self, self.engine, many_lut=True, device=device)
        self.trace, self.levels = [], []

    def bootstrap(self, reqs):
        self.levels.append(len(reqs))
        return super().bootstrap(reqs)

    def _pbs(self, flat, tables, idx):
        self.trace.append(("pbs", flat.shape[0], len(tables), idx.tolist()))
        return np.asarray(super()._pbs(flat, tables, idx))

    def _pbs_many(self, flat, table_groups, idx, n_fn):
        self.trace.append(("pbs_many", flat.shape[0], len(table_groups), idx.tolist(), n_fn))
        return np.asarray(super()._pbs_many(flat, table_groups, idx, n_fn))

    def _oprf(self, seeds, bit_kinds, idx):
        self.trace.append(("oprf", seeds.shape[0], len(bit_kinds), idx.tolist()))
        return np.asarray(self.trivial([int(s[0]) % (1 << bit_kinds[i]) for s, i in zip(seeds, idx)]))

    def blocks(self, vals):
        """Clear values as block arrays of this circuit that name a buffer (not lazy constants)."""
        v = np.asarray(vals, dtype=np.uint64)
        host = np.zeros(v.shape + (self.dim,), dtype=np.uint64)
        host[..., -1] = v * np.uint64(R.DELTA)
        return self._ingest(host)


def values(x):
    return ClearKey().decrypt(np.asarray(x), R.SPACE).astype(np.int64)


def rows_of(trace, seam):
    return [t[1] for t in trace if t[0] == seam]


def idx_of(trace, seam):
    return [i for t in trace if t[0] == seam for i in t[3]]


# ---- 1. chunk boundaries ------------------------------------------------------------------------------------------
CUTS = {3: [3], 4: [4], 5: [4, 1]}


@pytest.mark.parametrize("total", [3, 4, 5])
def test_radix_ordinary_level_is_cut_at_max_launch(monkeypatch, total):
    monkeypatch.setattr(R, "MAX_LAUNCH", 4)
    traces = []
    for mode in MODES:
        c = Recorder(mode)
        a, b = np.arange(2), (np.arange(total - 2) + 5).reshape(total - 2, 1)
        ra, rb = c.bootstrap([(c.blocks(a), T_INC), (c.blocks(b), T_DBL)])
        assert rows_of(c.trace, "pbs") == CUTS[total]
        assert all(t[2] == 2 for t in c.trace)
        assert idx_of(c.trace, "pbs") == [0, 0] + [1] * (total - 2)
        assert (c.pbs_count, c.launches) == (total, 1)
        assert ra.shape == (2, c.dim) and rb.shape == (total - 2, 1, c.dim)
        assert isinstance(ra, R.LinBlocks) == (mode is not None)
        assert values(ra).tolist() == (a + 1).tolist() and values(rb).tolist() == (2 * b).tolist()
        traces.append(c.trace)
    assert traces[0] == traces[1]


@pytest.mark.parametrize("total", [1, 2, 3])
def test_radix_many_lut_level_is_cut_at_max_launch_over_n_fn(monkeypatch, total):
    monkeypatch.setattr(R, "MAX_LAUNCH", 4)                      # two functions: two rows a call
    traces = []
    for mode in MODES:
        c = Recorder(mode)
        last = (np.array([[6]]), G2B)
        first = (np.arange(total - 1) + 1, G2A)
        ents = [first, last] if total > 1 else [(last[0], G2A)]
        res = c.bootstrap([(c.blocks(v), g) for v, g in ents])
        assert rows_of(c.trace, "pbs_many") == {1: [1], 2: [2], 3: [2, 1]}[total]
        assert all(t[0] == "pbs_many" and t[2] == len(ents) and t[4] == 2 for t in c.trace)
        assert idx_of(c.trace, "pbs_many") == [0] * (total - 1) + [len(ents) - 1]
        assert (c.pbs_count, c.launches) == (total, 1)
        for (v, g), r in zip(ents, res):
            assert isinstance(r, tuple) and len(r) == 2
            for f in range(2):
                assert r[f].shape == v.shape + (c.dim,)
                assert isinstance(r[f], R.LinBlocks) == (mode is not None)
                assert values(r[f]).tolist() == np.array(g[f])[v].tolist()
        traces.append(c.trace)
    assert traces[0] == traces[1]


@pytest.mark.parametrize("total", [3, 4, 5])
def test_radix_oprf_is_cut_at_max_launch(monkeypatch, total):
    monkeypatch.setattr(R, "MAX_LAUNCH", 4)
    traces = []
    seeds = np.array([[7 + 3 * r, 100 + r] for r in range(total)], dtype=np.uint64)
    bits = np.array([2, 1, 2, 2, 1][:total])
    for mode in MODES:
        c = Recorder(mode)
        out = c.oprf(seeds, bits)
        assert rows_of(c.trace, "oprf") == CUTS[total]
        assert all(t[2] == 2 for t in c.trace)                                  # the kinds: 1 and 2 bits
        assert idx_of(c.trace, "oprf") == (bits - 1).tolist()
        assert (c.pbs_count, c.launches) == (total, 1)
        assert out.shape == (total, c.dim) and isinstance(out, R.LinBlocks) == (mode is not None)
        assert values(out).tolist() == [int(s) % (1 << b) for s, b in zip(seeds[:, 0], bits)]
        traces.append(c.trace)
    assert traces[0] == traces[1]


class RecordingEngine(CleartextTorchEngine):
    """The gate double, noting the rows of every call; oprf: the bit is the low bit of the seed."""

    def __init__(self):
        super().__init__(n=6)
        self.calls = []

    def pbs(self, cts, lut):
        self.calls.append(len(cts))
        return super().pbs(cts, lut)

    def oprf(self, seeds, lut, post_adds):
        self.calls.append(len(seeds))
        out = np.zeros((len(seeds), self.params.n + 1), dtype=np.uint64)
        out[:, -1] = tfhe_amd.encode_bool(seeds[:, 0] & np.uint64(1))
        return out

    def oprf_device(self, d_seeds, d_lut, d_post):
        import torch
        assert d_post.tolist() == [0]
        return torch.from_numpy(self.oprf(d_seeds.numpy().view(np.uint64), d_lut, [0]).view(np.int64))


def bits_of(a):
    if not isinstance(a, np.ndarray):
        a = a.numpy().view(np.uint64)
    return BitKey().decrypt_bool(a)


@pytest.mark.parametrize("total", [3, 4, 5])
def test_gate_level_and_oprf_are_cut_at_max_launch(monkeypatch, total):
    pytest.importorskip("torch")
    monkeypatch.setattr(I, "MAX_LAUNCH", 4)
    a = np.array([True, False])
    b = (np.arange(total - 2) % 2 == 0).reshape(total - 2, 1)
    seeds = np.array([[r * r + 1, 9] for r in range(total)], dtype=np.uint64)
    got = []
    for dev in MODES:
        eng = RecordingEngine()
        c = I.Circuit(eng, device=dev)
        ra, rb = c.bootstrap([c.trivial(a), c.trivial(b)])
        assert eng.calls == CUTS[total] and (c.pbs_count, c.launches) == (total, 1)
        assert tuple(ra.shape) == (2, c.dim) and tuple(rb.shape) == (total - 2, 1, c.dim)
        assert isinstance(ra, np.ndarray) == (dev is None)
        assert bits_of(ra).tolist() == a.tolist() and bits_of(rb).tolist() == b.tolist()
        out = c.oprf(seeds)
        assert eng.calls == CUTS[total] * 2 and (c.pbs_count, c.launches) == (2 * total, 2)
        assert tuple(out.shape) == (total, c.dim) and isinstance(out, np.ndarray) == (dev is None)
        assert bits_of(out).tolist() == [bool(s & 1) for s in seeds[:, 0].tolist()]
        got.append(eng.calls)
    assert got[0] == got[1]


@pytest.mark.parametrize("dev", MODES)
def test_gate_circuit_counts_no_launch_for_an_empty_level(dev):
    pytest.importorskip("torch")
    eng = RecordingEngine()
    c = I.Circuit(eng, device=dev)
    assert c.bootstrap([]) == []
    (r,) = c.bootstrap([c.trivial(np.zeros((0, 3), dtype=bool))])
    assert tuple(r.shape) == (0, 3, c.dim)
    assert tuple(c.oprf(np.zeros((0, 2), dtype=np.uint64)).shape) == (0, c.dim)
    assert eng.calls == [] and (c.pbs_count, c.launches) == (0, 0)


# ---- 2. a mixed level ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_mixed_level_groups_and_answers_in_request_order(mode):
    c = Recorder(mode)
    ents = [(np.array([1, 2]), T_INC), (np.array([[0, 1, 3]]), G4), (np.array([[[5]], [[6]]]), T_DBL),
            (np.array([7, 0]), G2A), (np.array([[9, 3, 4]]), T_INC), (np.array([[[2]], [[5]]]), G2B)]
    res = c.bootstrap([(c.blocks(v), t) for v, t in ents])
    assert [t[0] for t in c.trace] == ["pbs", "pbs_many", "pbs_many"]
    assert c.trace[0] == ("pbs", 7, 2, [0, 0, 1, 1, 0, 0, 0])
    assert c.trace[1] == ("pbs_many", 4, 2, [0, 0, 1, 1], 2)
    assert c.trace[2] == ("pbs_many", 3, 1, [0, 0, 0], 4)
    assert (c.launches, c.pbs_count) == (1, 14)
    assert len(res) == len(ents)
    for (v, t), r in zip(ents, res):
        if isinstance(t[0], tuple):
            assert isinstance(r, tuple) and len(r) == len(t)
            for f, part in enumerate(r):
                assert part.shape == v.shape + (c.dim,)
                assert values(part).tolist() == np.array(t[f])[v].tolist()
        else:
            assert r.shape == v.shape + (c.dim,)
            assert values(r).tolist() == np.array(t)[v].tolist()
    with pytest.raises(ValueError):
        c.bootstrap([(c.blocks([1]), T_INC), (c.blocks([1]), (tuple(range(8)),) * 4)])


# ---- 3. lockstep --------------------------------------------------------------------------------------------------
def test_radix_run_many_steps_coroutines_in_lockstep():
    def op(c, tag, x, depth, width):
        for _ in range(depth):
            x = (yield [(x, T_INC)] * width)[0]
        return tag, x

    for mode in MODES:
        c = Recorder(mode)
        x = c.blocks([0, 4])
        res = c.run_many([op(c, "a", x, 0, 1), op(c, "b", x, 1, 1), op(c, "c", x, 3, 2)])
        assert [r[0] for r in res] == ["a", "b", "c"]
        assert [values(r[1]).tolist() for r in res] == [[0, 4], [1, 5], [3, 7]]
        assert c.levels == [3, 2, 2] and c.launches == 3 and c.pbs_count == 14
        assert c.run(op(c, "d", x, 0, 1))[0] == "d" and c.launches == 3


def test_gate_run_many_steps_coroutines_in_lockstep():
    class Counting(I.Circuit):
        levels = ()

        def bootstrap(self, lins):
            self.levels = self.levels + (len(lins),)
            return super().bootstrap(lins)

    def op(tag, x, depth, width):
        for _ in range(depth):
            x = I.NOT((yield [x] * width)[0])
        return tag, x

    c = Counting(RecordingEngine())
    x = c.trivial([True, False, False])
    res = c.run_many([op("a", x, 0, 1), op("b", x, 1, 1), op("c", x, 3, 2)])
    assert [r[0] for r in res] == ["a", "b", "c"]
    assert [bits_of(r[1]).tolist() for r in res] == [[True, False, False], [False, True, True], [False, True, True]]
    assert c.levels == (3, 2, 2) and c.launches == 3 and c.pbs_count == 21


# ---- 4. lut_index of the host entry points ------------------------------------------------------------------------
class FakeLib:
    """Stands in for the C library: notes the arguments of every call and reports success."""

    def __init__(self):
        self.calls = {}

    def __getattr__(self, name):
        def call(*args):
            self.calls[name] = args
            return 0
        return call


@pytest.fixture
def engine(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(tfhe_amd, "lib", lambda: fake)
    eng = tfhe_amd.Engine.__new__(tfhe_amd.Engine)
    eng.params = SimpleNamespace(N=8, io_dim=4, n=3, k=1)
    eng._h = None
    return eng, fake


def test_lut_index_of_the_wrong_length_is_refused(engine):
    eng, fake = engine
    cts, luts, seeds = np.zeros((3, 5), dtype=np.uint64), np.zeros((2, 8), dtype=np.uint64), np.zeros((3, 2), dtype=np.uint64)
    with pytest.raises(ValueError, match="^lut_index must have one entry per ciphertext$"):
        eng.pbs(cts, luts, [0, 1])
    with pytest.raises(ValueError, match="^lut_index must have one entry per ciphertext$"):
        eng.pbs_many(cts, luts, 2, 4, [0, 1, 0, 1])
    with pytest.raises(ValueError, match="^lut_index must have one entry per output row$"):
        eng.expand_cast(np.zeros(10, dtype=np.uint64), 2, luts, rep=2, lut_index=[0, 1, 0])
    with pytest.raises(ValueError, match="^lut_index must have one entry per seed$"):
        eng.oprf(seeds, luts, [0, 0], [0, 1])
    assert fake.calls == {}


def test_lut_index_reaches_the_library_as_uint32_or_null(engine):
    eng, fake = engine
    cts, luts, seeds = np.zeros((3, 5), dtype=np.uint64), np.zeros((2, 8), dtype=np.uint64), np.zeros((3, 2), dtype=np.uint64)
    words = np.zeros(10, dtype=np.uint64)
    sites = [("tfhe_hip_pbs", 5, 3, lambda li: eng.pbs(cts, luts, li)),
             ("tfhe_hip_expand_cast", 8, 4, lambda li: eng.expand_cast(words, 2, luts, rep=2, lut_index=li)),
             ("tfhe_hip_oprf", 6, 3, lambda li: eng.oprf(seeds, luts, [0, 0], li))]
    for name, pos, rows, call in sites:
        call(None)
        assert fake.calls[name][pos] is None, name
        index = [1, 0, 1, 1][:rows]
        call(np.array(index, dtype=np.int64)[::-1][::-1])          # neither uint32 nor required to be
        p = fake.calls[name][pos]
        assert isinstance(p, ctypes.POINTER(ctypes.c_uint32)) and [p[i] for i in range(rows)] == index, name
