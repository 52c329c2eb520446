"""Seeded server keys loaded on the MI355X (tfhe_amd/csrc/seeded_keys.hip, tfhe_hip_load_*_seeded,
Engine.load_compressed_keys): the expansion kernel against the host decompression word for word, the loaders against
the host route (decompress_server_key + load_keys) bit for bit, sequences of loads on one engine, two shards, and the
refusals.  Every input is a valid size or is refused on the host before a launch."""
import ctypes

import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import keyio
from oracle import oracle as O
from test_decompress import bootstrap_ref, with_n

pytestmark = pytest.mark.gpu

GUARD = 64                                     # TFHE_HIP_SEEDED_GUARD_WORDS
GUARD_WORD = np.uint64(0xA5A5A5A5A5A5A5A5)
MM = 16
DELTA = (1 << 63) // MM
TABLE = [(5 * m + 3) % MM for m in range(MM)]
MB_KERNEL = "blind_rotate_fft2k_mb_kernel"
SEED_A = 0x0123456789ABCDEF_FEDCBA9876543210
SEED_B = SEED_A ^ (0x80 << 120)                # differs from SEED_A in the top byte of `hi` only
P2, P3, P4 = tfhe_amd.PRESET_GATE_FFT, tfhe_amd.PRESET_FHEVM_FFT, tfhe_amd.PRESET_FHEVM_MB_FFT


def _s2(seed):
    return tfhe_amd._u64(keyio._seed2(seed))


def _rand(count, salt):
    return np.random.default_rng(0x5EED10AD + salt).integers(0, 1 << 64, count, dtype=np.uint64)


def _split(buf, want_len):
    assert buf.size == want_len + GUARD
    assert np.all(buf[want_len:] == GUARD_WORD), "the kernel wrote behind its output"
    return buf[:want_len]


@pytest.fixture(scope="module")
def engines():
    """(preset, n) -> an engine of that shape, shared by the kernel tests (they load no key)"""
    cache = {}

    def get(preset, n):
        if (preset, n) not in cache:
            cache[preset, n] = tfhe_amd.Engine(with_n(tfhe_amd.Params.preset(preset), n), 0)
        return cache[preset, n]

    yield get
    for e in cache.values():
        e.close()


# ------------------------------------------------------------------ the kernel against the host, word for word
def _list_pair(eng, dim, count, seed, salt):
    L = tfhe_amd.lib()
    bodies = _rand(count, salt)
    out = np.zeros(count * (dim + 1) + GUARD, dtype=np.uint64)
    tfhe_amd._check(L.tfhe_hip_seeded_expand_lwe_list(eng._h, dim, count, _s2(seed), tfhe_amd._u64(bodies),
                                                      tfhe_amd._u64(out)))
    ref = np.zeros(count * (dim + 1), dtype=np.uint64)
    tfhe_amd._check(L.tfhe_hip_decompress_lwe_list(dim, count, _s2(seed), tfhe_amd._u64(bodies), tfhe_amd._u64(ref)))
    return _split(out, ref.size), ref


# 2047 and 2049 are the kernel's chunk size (2048 mask words per workgroup) -+ 1; 4099 is three chunks
@pytest.mark.parametrize("dim", [1, 2, 3, 1021, 1022, 1023, 1024, 1025, 2047, 2048, 2049, 4099])
def test_lwe_list_rows(engines, dim):
    dev, ref = _list_pair(engines(P3, 16), dim, 3, SEED_A, dim)      # odd dims: the first-word parity alternates
    assert np.array_equal(dev, ref)


def test_seeds_that_differ_in_the_top_byte(engines):
    """the key schedule runs once per seed on the host: every byte of the seed must reach it"""
    a, ref_a = _list_pair(engines(P3, 16), 1023, 3, SEED_A, 7)
    b, ref_b = _list_pair(engines(P3, 16), 1023, 3, SEED_B, 7)
    assert np.array_equal(a, ref_a) and np.array_equal(b, ref_b)
    assert not np.array_equal(a.reshape(3, 1024)[:, :-1], b.reshape(3, 1024)[:, :-1])


@pytest.mark.parametrize("preset", [P2, P3])
@pytest.mark.parametrize("n", [1, 2, 15, 16])
def test_ksk_rows(engines, preset, n):
    L = tfhe_amd.lib()
    eng = engines(preset, n)
    p = eng.params
    bodies = _rand(p.k * p.N * p.ks_level, 100 + n)
    want = L.tfhe_hip_ksk_len(ctypes.byref(p))
    out = np.zeros(want + GUARD, dtype=np.uint64)
    tfhe_amd._check(L.tfhe_hip_seeded_expand_ksk(eng._h, _s2(SEED_A), tfhe_amd._u64(bodies), tfhe_amd._u64(out)))
    ref = np.zeros(want, dtype=np.uint64)
    tfhe_amd._check(L.tfhe_hip_decompress_ksk(ctypes.byref(p), _s2(SEED_A), tfhe_amd._u64(bodies), tfhe_amd._u64(ref)))
    dev = _split(out, want)
    assert np.array_equal(dev, ref)
    # level reversal: storage row s lands in engine row ks_level - 1 - s
    assert np.array_equal(dev.reshape(p.k * p.N, p.ks_level, n + 1)[:, ::-1, n], bodies.reshape(p.k * p.N, p.ks_level))


@pytest.mark.parametrize("preset", [P2, P3])
@pytest.mark.parametrize("n", [1, 3])
def test_classic_bsk_rows(engines, preset, n):
    L = tfhe_amd.lib()
    eng = engines(preset, n)
    p = eng.params
    bodies = _rand(n * p.pbs_level * (p.k + 1) * p.N, 200 + n)
    want = L.tfhe_hip_bsk_len(ctypes.byref(p))
    out = np.zeros(want + GUARD, dtype=np.uint64)
    tfhe_amd._check(L.tfhe_hip_seeded_expand_bsk(eng._h, 1, _s2(SEED_A), tfhe_amd._u64(bodies), tfhe_amd._u64(out)))
    ref = np.zeros(want, dtype=np.uint64)
    tfhe_amd._check(L.tfhe_hip_decompress_bsk(ctypes.byref(p), _s2(SEED_A), tfhe_amd._u64(bodies), tfhe_amd._u64(ref)))
    dev = _split(out, want)
    assert np.array_equal(dev, ref)
    b = bodies.reshape(n, p.pbs_level, p.k + 1, p.N)                 # source [i][l][c] -> destination [i][c L + l]
    d = dev.reshape(n, p.k + 1, p.pbs_level, (p.k + 1) * p.N)
    assert np.array_equal(d[..., p.k * p.N:], b.transpose(0, 2, 1, 3))


@pytest.mark.parametrize("g", [2, 3, 4])
@pytest.mark.parametrize("mult", [1, 2])
def test_multibit_bsk_rows(engines, g, mult):
    L = tfhe_amd.lib()
    n = g * mult
    eng = engines(P4, n)
    p = eng.params
    bodies = _rand(L.tfhe_hip_seeded_mb_bodies_len(ctypes.byref(p), g), 300 + 10 * g + mult)
    want = L.tfhe_hip_mb_bsk_len(ctypes.byref(p), g)
    out = np.zeros(want + GUARD, dtype=np.uint64)
    tfhe_amd._check(L.tfhe_hip_seeded_expand_bsk(eng._h, g, _s2(SEED_A), tfhe_amd._u64(bodies), tfhe_amd._u64(out)))
    ref = np.zeros(want, dtype=np.uint64)
    tfhe_amd._check(L.tfhe_hip_decompress_bsk_mb(ctypes.byref(p), g, _s2(SEED_A), tfhe_amd._u64(bodies),
                                                 tfhe_amd._u64(ref)))
    dev = _split(out, want)
    assert np.array_equal(dev, ref)
    b = bodies.reshape(n // g, 1 << g, 2, p.N)                       # sigma = 0 is skipped, in both groups
    assert np.array_equal(dev.reshape(n // g, (1 << g) - 1, 2, 2 * p.N)[..., p.N:], b[:, 1:])


# ------------------------------------------------------------------ the loaders against the host route
def _enc(dim, key, noise_log2, msgs, seed):
    m = np.asarray(msgs, dtype=np.uint64) * np.uint64(DELTA)
    out = np.zeros((m.size, dim + 1), dtype=np.uint64)
    assert tfhe_amd.lib().tfhe_hip_lwe_encrypt(dim, tfhe_amd._u64(key), noise_log2, seed, 0, tfhe_amd._u64(m), m.size,
                                               tfhe_amd._u64(out)) == 0
    return out


class Case:
    """one key set in seeded form, its host decompression, and one fixed batch of inputs"""

    def __init__(self, preset, n, ms_count=0, g=1, salt=0):
        self.preset, self.g = preset, g
        self.p = with_n(tfhe_amd.Params.preset(preset), n)
        p = self.p
        self.ck, _ = tfhe_amd.gen_keys(p, 0x5EED5EED + salt, with_server_key=False)
        self.csk = keyio.compress_server_key(self.ck, seed=0x5EED0003 + salt, ms_count=ms_count, grouping=g)
        self.csk = keyio.loads_compressed_server_key(keyio.dumps_compressed_server_key(self.csk))
        self.p2, self.sk = keyio.decompress_server_key(self.csk)
        self.msgs = np.arange(9, dtype=np.uint64) * 3 % MM
        if p.order == 1:
            self.cts = self.ck.encrypt(self.msgs, MM, seed=0xC0FFEE70)
            self.lut = tfhe_amd.lut_from_table(p.N, MM, TABLE, DELTA)[None]
        else:
            self.cts = self.ck.encrypt_bool(self.msgs % 2 == 1, seed=0xC0FFEE70)
            self.lut = tfhe_amd.lut_constant(p.N, tfhe_amd.MU)[None]
        self.small = _enc(p.n, self.ck.lwe_key, p.lwe_noise_log2, self.msgs, 0xC0FFEE71)
        if ms_count and n < 100:
            # At a reduced n the key's default bound 2^58 lies above every row's own measure and nothing is scanned
            # (tests/offpreset_cases.py MsCase).  The key carries half the smallest measure that the oracle finds for
            # this batch with any zero instead: no row is within it, every row scans the whole key.
            prm, keys = self.oracle_keys()
            rows = [O.keyswitch(prm, keys, c) for c in self.cts]
            mk = O.ms_key(self.sk.ms_zeros)
            self.csk.ms["bound"] = 0.5 * min(O.ms_measure(prm, None, c, z, ms=mk) for c in rows for z in range(ms_count))
        self.big = _enc(p.k * p.N, self.ck.glwe_key, p.glwe_noise_log2, self.msgs[:5], 0xC0FFEE72)

    def oracle_keys(self):
        """the oracle's view of the decompressed keys (preset 4 is preset 3's shape at another n)"""
        prm = with_n(O.params(P3 if self.preset == P4 else self.preset), self.p.n)
        keys = O.Keys.__new__(O.Keys)
        keys.prm, keys.seed, keys.lwe_key, keys.glwe_key = prm, 0, self.ck.lwe_key, self.ck.glwe_key
        keys.bsk, keys.ksk, keys._bsk_ntt, keys.ms_zeros = self.sk.bsk, self.sk.ksk, None, self.sk.ms_zeros
        return prm, keys

    def host_engine(self, device=0, zeros=True):
        """the route that needs no device expansion: decompress_server_key + load_keys (+ load_ms_key)"""
        return self.host_load(tfhe_amd.Engine(self.p2, device), zeros)

    def host_load(self, eng, zeros=True):
        eng.load_keys(tfhe_amd.ServerKey(self.p2, self.sk.bsk, self.sk.ksk, None, grouping=self.sk.grouping))
        if zeros and self.sk.ms_zeros is not None:
            eng.load_ms_key(self.sk.ms_zeros, **self.csk.ms)
        return eng

    def outputs(self, eng):
        return eng.pbs(self.cts, self.lut), eng.keyswitch(self.big)

    def same(self, eng, ref) -> bool:
        return all(np.array_equal(a, b) for a, b in zip(self.outputs(eng), ref))

    def decrypts(self, out) -> bool:
        if self.p.order == 1:
            return np.array_equal(self.ck.decrypt(out, MM), np.array([TABLE[m] for m in self.msgs]))
        return np.array_equal(self.ck.decrypt_bool(out), self.msgs % 2 == 1)


def _oracle_rows(case, rows=3):
    """the CPU oracle's PBS of the first rows; with an explicit bound in the key: keyswitch -> or_ms_reduce with that
    bound (or_pbs_batch knows the default bound only) -> rotation and extraction, and the reduction must be live"""
    prm, keys = case.oracle_keys()
    if case.sk.ms_zeros is None or case.csk.ms["bound"] == tfhe_amd.MS_FHEVM["bound"]:
        return O.pbs_batch_fft(prm, keys, case.cts[:rows], case.lut)
    small = np.stack([O.keyswitch(prm, keys, c) for c in case.cts[:rows]])
    small, picks = O.ms_reduce(prm, None, small, ms=O.ms_key(case.sk.ms_zeros, **case.csk.ms))
    assert (picks >= 0).any()
    return np.stack([bootstrap_ref(O, prm, keys, c, case.lut[0])[1] for c in small])


def _loaders_agree(case, oracle_mod):
    with tfhe_amd.Engine(case.p2, 0) as dev, case.host_engine() as host:
        dev.load_compressed_keys(case.csk)
        assert dev.grouping == host.grouping == case.g
        out, ks = case.outputs(dev)
        ref, ks_ref = case.outputs(host)
        assert np.array_equal(out, ref) and np.array_equal(ks, ks_ref)
        assert case.decrypts(out)
        if case.g == 1:
            assert np.array_equal(out[:3], _oracle_rows(case))
    # the BSK-only form: a rotation-only engine from the seeded bootstrapping key
    if case.g == 1:
        with tfhe_amd.Engine(case.p2, 0) as dev, tfhe_amd.Engine(case.p2, 0) as host:
            dev.load_compressed_bsk(case.csk.bsk_seed, case.csk.bsk_bodies)
            host.load_bsk(case.sk.bsk)
            assert np.array_equal(dev.bootstrap(case.small, case.lut), host.bootstrap(case.small, case.lut))
            with pytest.raises(tfhe_amd.TfheError):
                dev.pbs(case.cts, case.lut)                            # rotation-only: no keyswitching key
    else:
        with tfhe_amd.Engine(case.p2, 0) as dev, case.host_engine() as host:
            L = tfhe_amd.lib()
            bb = np.ascontiguousarray(case.csk.bsk_bodies).ravel()
            tfhe_amd._check(L.tfhe_hip_load_keys_mb_seeded(dev._h, case.g, _s2(case.csk.bsk_seed), tfhe_amd._u64(bb),
                                                           bb.size, None, None, 0))
            assert np.array_equal(dev.bootstrap(case.small, case.lut), host.bootstrap(case.small, case.lut))
            with pytest.raises(tfhe_amd.TfheError):
                dev.pbs(case.cts, case.lut)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(*key):
        if key not in cache:
            preset, n, ms_count, g = key
            cache[key] = Case(preset, n, ms_count, g, salt=len(cache))
        return cache[key]

    return get


def test_loader_fhevm_with_zeros(cases, oracle_mod):
    case = cases(P3, 16, 24, 1)
    assert case.sk.ms_zeros.shape == (24, 17)
    _loaders_agree(case, oracle_mod)
    # the noise reduction is live: without the zeros the same batch comes out different
    with case.host_engine(zeros=False) as bare, case.host_engine() as host:
        assert not np.array_equal(bare.pbs(case.cts, case.lut), host.pbs(case.cts, case.lut))


def test_loader_gate(cases, oracle_mod):
    _loaders_agree(cases(P2, 16, 0, 1), oracle_mod)


@pytest.mark.parametrize("g", [2, 3, 4])
def test_loader_multibit(cases, oracle_mod, g):
    _loaders_agree(cases(P4, 12, 0, g), oracle_mod)


def test_loader_full_fhevm_key(oracle_mod):
    """the real PRESET_FHEVM_FFT key set: n = 918, 1449 zeros (tests/test_gpu_seeded.py does the host route)"""
    case = Case(P3, 918, tfhe_amd.MS_FHEVM["count"], 1, salt=99)
    assert case.sk.ms_zeros.shape == (1449, 919)
    with tfhe_amd.Engine(case.p2, 0) as dev, case.host_engine() as host:
        dev.load_compressed_keys(case.csk)
        out = dev.pbs(case.cts, case.lut)
        assert np.array_equal(out, host.pbs(case.cts, case.lut))
        assert np.array_equal(dev.keyswitch(case.big), host.keyswitch(case.big))
        assert case.decrypts(out)
        assert np.array_equal(out[:3], _oracle_rows(case))


# ------------------------------------------------------------------ sequences on one engine
def test_multibit_classic_multibit_on_one_engine(cases):
    """the key buffers grow and are reused; the classic back end is restored in between"""
    mb2, cl, mb3 = cases(P4, 12, 0, 2), cases(P4, 12, 24, 1), cases(P4, 12, 0, 3)
    refs = {}
    for c in (mb2, cl, mb3):
        with c.host_engine() as host:
            refs[c] = c.outputs(host)
    with tfhe_amd.Engine(cl.p2, 0) as eng:
        eng.load_compressed_keys(mb2.csk)
        assert eng.grouping == 2 and eng.br_kernel(9) == MB_KERNEL and mb2.same(eng, refs[mb2])
        eng.load_compressed_keys(cl.csk)
        assert eng.grouping == 1 and eng.br_kernel(9) != MB_KERNEL and cl.same(eng, refs[cl])
        eng.load_compressed_keys(mb3.csk)
        assert eng.grouping == 3 and eng.br_kernel(9) == MB_KERNEL and mb3.same(eng, refs[mb3])


def test_seeded_over_host_loaded_and_back(cases):
    a, b = cases(P3, 16, 24, 1), cases(P3, 16, 0, 1)
    with a.host_engine() as host_a, b.host_engine() as host_b:
        ref_a, ref_b = a.outputs(host_a), b.outputs(host_b)
    with tfhe_amd.Engine(a.p2, 0) as eng:
        a.host_load(eng)
        assert a.same(eng, ref_a)
        eng.load_compressed_keys(b.csk)          # b carries no zeros: a's are switched off by hand, as on the host route
        eng.load_ms_key(None)
        assert b.same(eng, ref_b)
        a.host_load(eng)
        assert a.same(eng, ref_a)
        eng.load_compressed_keys(a.csk)
        assert a.same(eng, ref_a)


def test_zeros_and_multibit_keys(cases):
    """the zeros are refused on a multi-bit engine and dropped by a multi-bit load"""
    L = tfhe_amd.lib()
    cl, mb = cases(P4, 12, 24, 1), cases(P4, 12, 0, 2)
    with cl.host_engine(zeros=False) as bare:
        ref_bare = cl.outputs(bare)
    with cl.host_engine() as host:
        ref_zeros = cl.outputs(host)
    assert not np.array_equal(ref_bare[0], ref_zeros[0])
    msb = np.ascontiguousarray(cl.csk.ms_bodies)
    with tfhe_amd.Engine(cl.p2, 0) as eng:
        eng.load_compressed_keys(cl.csk)
        assert cl.same(eng, ref_zeros)
        eng.load_compressed_keys(mb.csk)
        ms = cl.csk.ms
        assert L.tfhe_hip_load_ms_key_seeded(eng._h, _s2(cl.csk.ms_seed), tfhe_amd._u64(msb), msb.size, ms["bound"],
                                             ms["r_sigma"], ms["input_variance"]) == -5
        with mb.host_engine() as host:
            assert mb.same(eng, mb.outputs(host))
        bb, kb = np.ascontiguousarray(cl.csk.bsk_bodies).ravel(), np.ascontiguousarray(cl.csk.ksk_bodies).ravel()
        tfhe_amd._check(L.tfhe_hip_load_keys_seeded(eng._h, _s2(cl.csk.bsk_seed), tfhe_amd._u64(bb), bb.size,
                                                    _s2(cl.csk.ksk_seed), tfhe_amd._u64(kb), kb.size))
        assert cl.same(eng, ref_bare)              # the multi-bit load dropped the zeros
        tfhe_amd._check(L.tfhe_hip_load_ms_key_seeded(eng._h, _s2(cl.csk.ms_seed), tfhe_amd._u64(msb), msb.size,
                                                      ms["bound"], ms["r_sigma"], ms["input_variance"]))
        assert cl.same(eng, ref_zeros)


@pytest.mark.parametrize("key", [(P3, 16, 24, 1), (P4, 12, 0, 3)])
def test_two_shards_on_one_device(cases, key):
    """Engine(params, [0, 0]): the bodies are broadcast and each shard expands its own copy"""
    case = cases(*key)
    with case.host_engine() as one:
        ref = case.outputs(one)
    with tfhe_amd.Engine(case.p2, [0, 0]) as two:
        two.load_compressed_keys(case.csk)
        assert two.key_bcast_mode == "copy"
        assert case.same(two, ref)


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_resident_key_usable(cases):
    L = tfhe_amd.lib()
    case, mb = cases(P4, 12, 24, 1), cases(P4, 12, 0, 2)
    u = tfhe_amd._u64
    bb, kb = np.ascontiguousarray(case.csk.bsk_bodies).ravel(), np.ascontiguousarray(case.csk.ksk_bodies).ravel()
    mbb = np.ascontiguousarray(mb.csk.bsk_bodies).ravel()
    msb = np.ascontiguousarray(case.csk.ms_bodies)
    sb, sk_ = _s2(case.csk.bsk_seed), _s2(case.csk.ksk_seed)
    with case.host_engine() as host:
        ref = case.outputs(host)
    out = np.zeros(bb.size * 2 + GUARD, dtype=np.uint64)
    with tfhe_amd.Engine(case.p2, 0) as eng, tfhe_amd.Engine(with_n(case.p2, 10), 0) as eng10, \
            tfhe_amd.Engine(tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM), 0) as ntt, \
            tfhe_amd.Engine(with_n(tfhe_amd.Params.preset(P2), 12), 0) as gate:
        eng.load_compressed_keys(case.csk)
        h = eng._h
        EINVAL, EUNSUPPORTED = -1, -5
        refused = [
            (L.tfhe_hip_load_keys_seeded(h, sb, u(bb), bb.size - 1, sk_, u(kb), kb.size), EINVAL),
            (L.tfhe_hip_load_keys_seeded(h, sb, u(bb), bb.size, sk_, u(kb), kb.size + 1), EINVAL),
            (L.tfhe_hip_load_keys_seeded(h, None, u(bb), bb.size, sk_, u(kb), kb.size), EINVAL),
            (L.tfhe_hip_load_keys_seeded(h, sb, None, bb.size, sk_, u(kb), kb.size), EINVAL),
            (L.tfhe_hip_load_keys_seeded(h, sb, u(bb), bb.size, None, u(kb), kb.size), EINVAL),
            (L.tfhe_hip_load_keys_seeded(h, sb, u(bb), bb.size, sk_, None, kb.size), EINVAL),
            (L.tfhe_hip_load_keys_seeded(None, sb, u(bb), bb.size, sk_, u(kb), kb.size), EINVAL),
            (L.tfhe_hip_load_bsk_seeded(h, sb, u(bb), bb.size + 1), EINVAL),
            (L.tfhe_hip_load_bsk_seeded(h, sb, None, bb.size), EINVAL),
            (L.tfhe_hip_load_keys_mb_seeded(h, 2, sb, u(mbb), mbb.size - 1, sk_, u(kb), kb.size), EINVAL),
            (L.tfhe_hip_load_keys_mb_seeded(h, 2, sb, u(mbb), mbb.size, sk_, u(kb), kb.size - 1), EINVAL),
            (L.tfhe_hip_load_keys_mb_seeded(h, 3, sb, u(mbb), mbb.size, sk_, u(kb), kb.size), EINVAL),   # g = 2 bodies
            (L.tfhe_hip_load_keys_mb_seeded(h, 5, sb, u(mbb), mbb.size, sk_, u(kb), kb.size), EINVAL),
            (L.tfhe_hip_load_keys_mb_seeded(h, 1, sb, u(bb), bb.size, sk_, u(kb), kb.size), EINVAL),
            (L.tfhe_hip_load_keys_mb_seeded(h, 2, None, u(mbb), mbb.size, sk_, u(kb), kb.size), EINVAL),
            (L.tfhe_hip_load_keys_mb_seeded(eng10._h, 3, sb, u(mbb), mbb.size, sk_, u(kb), kb.size), EINVAL),  # 10 % 3
            (L.tfhe_hip_load_keys_mb_seeded(eng10._h, 4, sb, u(mbb), mbb.size, sk_, u(kb), kb.size), EINVAL),  # 10 % 4
            (L.tfhe_hip_load_keys_mb_seeded(gate._h, 2, sb, u(mbb), mbb.size, sk_, u(kb), kb.size), EUNSUPPORTED),
            (L.tfhe_hip_load_keys_seeded(ntt._h, sb, u(bb), bb.size, sk_, u(kb), kb.size), EUNSUPPORTED),
            (L.tfhe_hip_load_ms_key_seeded(h, None, u(msb), msb.size, 1.0, 1.0, 1.0), EINVAL),
            (L.tfhe_hip_load_ms_key_seeded(h, sb, None, msb.size, 1.0, 1.0, 1.0), EINVAL),
            (L.tfhe_hip_load_ms_key_seeded(h, sb, u(msb), msb.size, -1.0, 1.0, 1.0), EINVAL),
            (L.tfhe_hip_load_ms_key_seeded(gate._h, sb, u(msb), msb.size, 1.0, 1.0, 1.0), EUNSUPPORTED),  # order 0
            (L.tfhe_hip_seeded_expand_bsk(h, 5, sb, u(mbb), u(out)), EINVAL),
            (L.tfhe_hip_seeded_expand_bsk(h, 0, sb, u(bb), u(out)), EINVAL),
            (L.tfhe_hip_seeded_expand_bsk(h, 1, sb, u(bb), None), EINVAL),
            (L.tfhe_hip_seeded_expand_ksk(h, sb, None, u(out)), EINVAL),
            (L.tfhe_hip_seeded_expand_lwe_list(h, 0, 3, sb, u(msb), u(out)), EINVAL),
        ]
        for i, (got, want) in enumerate(refused):
            assert got == want, (i, got, want)
        assert eng.grouping == 1 and case.same(eng, ref)
