"""Compact-list expansion on the device (tfhe_amd/csrc/expand.hip, tfhe_hip_expand_*), the parts that need no GPU:
the size rule of the list's words, the word order ctlist.list_words hands to the device, and the list checks of
the C ABI, which precede the null-ctx check and so show their verdict without a device."""
import ctypes
from functools import lru_cache

import numpy as np

import tfhe_amd
from tfhe_amd import ctlist
from test_ctlist import _fixtures

SEED = 0x7F4E0001


def words(lwe_dim, count):
    return tfhe_amd.lib().tfhe_hip_compact_list_words(lwe_dim, count)


def with_n(prm, n):
    d = type(prm).from_buffer_copy(prm)
    d.n = n
    return d


class SmallCase:
    """The full path at a small shape (tests/test_gpu_expand.py): P-GATE on the FFT64 transform with n = 64, order
    0, so a compact list of dimension 64 under the engine's own small key is a PBS input.  70 entries in two bins,
    two rows per entry (rep = 2), LUT r % 2 on row r.

    Encoding.  A P-GATE PBS output carries the keyswitch noise of that parameter set, a few 2^55 on the 2^64
    torus: too much for the packed space's 16 values (half-step 2^58), ample room in the engine's own gate space
    of 4 values at 2^61 (half-step 2^60).  encrypt_compact encodes v * 2^59, so the entries are v = 4 m, m < 4:
    m * 2^61.  test_small_case_decrypts_on_the_oracle checks on the CPU that the reference route returns every
    message under this encoding before the GPU test relies on it."""
    N_SMALL, COUNT, REP, DELTA = 64, 70, 2, 1 << 61

    def __init__(self):
        self.params = with_n(tfhe_amd.Params.preset(tfhe_amd.PRESET_GATE_FFT), self.N_SMALL)
        self.ck, self.sk = tfhe_amd.gen_keys(self.params, SEED)
        rng = np.random.default_rng(0xE59A)
        cpk = ctlist.gen_compact_public_key(self.ck.lwe_key, rng)
        self.msgs = rng.integers(0, 4, self.COUNT).astype(np.uint64)
        self.msgs[:4] = [0, 3, 1, 2]
        self.cl = ctlist.encrypt_compact(cpk, [4 * int(m) for m in self.msgs], [(ctlist.KIND_UNSIGNED, 2 * self.COUNT)], rng)
        N = self.params.N
        self.tables = ([0, 1, 2, 3], [1, 0, 3, 2])
        self.luts = np.stack([tfhe_amd.lut_from_table(N, 4, t, self.DELTA) for t in self.tables])
        self.rows = self.COUNT * self.REP
        self.idx = (np.arange(self.rows) % 2).astype(np.uint32)
        m2 = np.repeat(self.msgs, self.REP)
        self.expected = np.where(self.idx == 0, m2, np.array(self.tables[1], dtype=np.uint64)[m2])

    def reference_input(self):
        return np.repeat(ctlist.expand(self.cl), self.REP, axis=0)

    def decode(self, small_lwes):
        """(messages, worst |phase error|) of PBS outputs under the small key."""
        ph = self.ck.phase(small_lwes, key=self.ck.lwe_key)
        got = ((ph + np.uint64(self.DELTA // 2)) >> np.uint64(61)) & np.uint64(3)
        err = (ph - self.expected * np.uint64(self.DELTA)).view(np.int64)
        return got, int(np.abs(err).max())


@lru_cache(maxsize=None)
def small_case():
    return SmallCase()


# ---- the shapes of the GPU sweep (tests/test_gpu_expand.py) --------------------------------------------------------
def _counts(N):
    return (1, N - 1, N, N + 1, 2 * N + 3)


# (lwe_dim, counts, reps); the last one is the fhEVM dimension with a second, short bin
SWEEP = [(8, _counts(8), (1, 2, 3)), (32, _counts(32), (1, 2, 3)), (64, _counts(64), (1, 2, 3)),
         (4096, (3,), (1, 2, 3)), (2048, (1, 2048 + 3), (1, 2))]


def random_list(N, count, seed):
    """Random 64-bit masks and bodies with 0 and 2^64 - 1 planted in every mask (the wrapping negation of both)."""
    rng = np.random.default_rng(seed)
    bins = -(-count // N)
    masks = rng.integers(0, 2 ** 64, size=(bins, N), dtype=np.uint64)
    masks[:, 0], masks[:, 1] = 0, 2 ** 64 - 1
    masks[:, N - 2], masks[:, N - 1] = 0, 2 ** 64 - 1
    return ctlist.CompactList(N, count, masks, rng.integers(0, 2 ** 64, size=count, dtype=np.uint64))


def test_sweep_holds_both_sign_extremes():
    """The GPU sweep's table reaches a full bin (degree N - 1, nothing negated) in four shapes, and its reference
    has the two extremes where the sweep's assertions expect them."""
    assert sum(max(counts) >= N for N, counts, _ in SWEEP) >= 4
    cl = random_list(8, 8, 1)
    ex = ctlist.expand(cl)
    with np.errstate(over="ignore"):
        assert np.array_equal(ex[0, :7], np.uint64(0) - cl.masks[0, 1:]) and ex[0, 7] == cl.masks[0, 0]
    assert np.array_equal(ex[7, :8], cl.masks[0])


def test_compact_list_words():
    assert words(32, 1) == 33
    assert words(32, 32) == 64
    assert words(32, 33) == 97
    assert words(2048, 27) == 2075
    for dim in (0, 4, 48, 8192):
        assert words(dim, 3) == 0, dim
    for dim in (8, 32, 2048, 4096):
        assert words(dim, 0) == 0, dim
        assert words(dim, 1) == dim + 1


def test_list_words_of_the_reference_fixtures():
    fx = _fixtures()
    assert len(fx) == 4
    for name, data, _, _ in fx:
        cl = ctlist.load_compact_list(data)
        w = ctlist.list_words(cl)
        assert w.dtype == np.uint64 and w.ndim == 1 and w.flags.c_contiguous, name
        assert w.size == words(2048, cl.count), name
        assert np.array_equal(w, np.concatenate([cl.masks.ravel(), cl.bodies])), name


def test_list_words_of_a_two_bin_list():
    rng = np.random.default_rng(3)
    cl = ctlist.CompactList(8, 11, rng.integers(0, 2 ** 64, (2, 8), dtype=np.uint64),
                            rng.integers(0, 2 ** 64, 11, dtype=np.uint64))
    w = ctlist.list_words(cl)
    assert w.size == words(8, 11) == 27
    assert np.array_equal(w[:16].reshape(2, 8), cl.masks) and np.array_equal(w[16:], cl.bodies)


def test_small_case_decrypts_on_the_oracle(oracle_mod):
    """The condition under which the GPU test's decryption assertion means anything: the reference route (ctlist.expand,
    every row twice, the oracle's P-GATE FFT64 PBS at n = 64 with the key set of the same seed) returns every
    message, with the phase error under the half-step 2^60; and the expanded inputs decrypt before the PBS."""
    O = oracle_mod
    cs = small_case()
    assert cs.cl.lwe_dim == 64 and cs.cl.count == 70 and cs.cl.masks.shape == (2, 64)
    ex = ctlist.expand(cs.cl)
    ph = cs.ck.phase(ex, key=cs.ck.lwe_key)
    assert np.array_equal(((ph + np.uint64(1 << 60)) >> np.uint64(61)) & np.uint64(3), cs.msgs)
    oprm = with_n(O.params(2), 64)
    okeys = O.Keys(oprm, SEED)
    assert np.array_equal(okeys.lwe_key, cs.ck.lwe_key) and np.array_equal(okeys.bsk, cs.sk.bsk)
    out = O.pbs_batch_fft(oprm, okeys, cs.reference_input(), cs.luts, cs.idx)
    got, err = cs.decode(out)
    print("worst phase error 2^%.1f" % np.log2(max(err, 1)))
    assert np.array_equal(got, cs.expected)
    assert err < 1 << 60
    assert set(cs.expected[cs.idx == 1].tolist()) == {0, 1, 2, 3}  # the second LUT is exercised on every value


def test_list_checks_precede_the_ctx_check():
    """Every list check of tfhe_hip_expand_compact* runs before the null-ctx check; with a good list the null ctx
    is what is refused.  tfhe_hip_expand_cast* takes the dimension from the ctx, so there the ctx comes first."""
    L = tfhe_amd.lib()
    buf = np.zeros(256, dtype=np.uint64)
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    v = ctypes.c_void_p(buf.ctypes.data)

    def host(list_words, dim, count, rep, rows):
        return L.tfhe_hip_expand_compact(None, p, list_words, dim, count, rep, rows, p), L.tfhe_hip_last_error().decode()

    def dev(list_words, dim, count, rep, rows):
        return (L.tfhe_hip_expand_compact_async(None, v, list_words, dim, count, rep, rows, v, None),
                L.tfhe_hip_last_error().decode())

    for f in (host, dev):
        rc, msg = f(11, 8, 3, 2, 6)
        assert rc == -1 and "null ctx" in msg, msg
        rc, msg = f(0, 8, 0, 1, 0)      # the empty list is a valid list
        assert rc == -1 and "null ctx" in msg, msg
        rc, msg = f(12, 8, 3, 2, 6)
        assert rc == -1 and "list_words" in msg, msg
        rc, msg = f(8, 8, 0, 1, 0)      # count == 0 takes no words
        assert rc == -1 and "list_words" in msg, msg
        rc, msg = f(11, 8, 3, 0, 0)
        assert rc == -1 and "rep" in msg, msg
        rc, msg = f(11, 8, 3, 2, 7)
        assert rc == -1 and "rows" in msg, msg
        rc, msg = f(0, 8, 0, 1, 1)      # count == 0 gives no row
        assert rc == -1 and "rows" in msg, msg
        rc, msg = f((1 << 31) + 8, 8, 1 << 31, 1, 1)
        assert rc == -1 and "too many" in msg, msg
        # rows above 0x7FFFFFFF is a case of its own: count, list_words and rep pass, and rows <= count * rep
        rc, msg = f(1 << 31, 8, 1 << 30, 4, 1 << 31)
        assert rc == -1 and "rows" in msg and "too many rows" in msg, msg
        rc, msg = f(1 << 31, 8, 1 << 30, 4, (1 << 31) - 1)  # the largest row count passes on to the ctx check
        assert rc == -1 and "null ctx" in msg, msg
        for dim in (0, 4, 48):
            rc, msg = f(11, dim, 3, 2, 6)
            assert rc == -1 and "lwe_dim" in msg, (dim, msg)
        for dim in (8192, 1 << 20):
            rc, msg = f(dim + 3, dim, 3, 2, 6)
            assert rc == -5 and "4096" in msg, (dim, msg)
        rc, msg = f(4096 + 3, 4096, 3, 1, 3)  # the largest covered size passes on to the ctx check
        assert rc == -1 and "null ctx" in msg, msg
    rc = L.tfhe_hip_expand_cast(None, p, 12, 3, 2, 6, p, 1, None, p)
    assert rc == -1 and "expand_cast: null ctx" in L.tfhe_hip_last_error().decode()
    rc = L.tfhe_hip_expand_cast_async(None, v, 12, 3, 2, 6, v, 1, None, v, None)
    assert rc == -1 and "expand_cast: null ctx" in L.tfhe_hip_last_error().decode()
