"""Seeded noise-squashing and ct128 packing keys loaded on the MI355X (tfhe_amd/csrc/seeded_keys128.hip,
tfhe_hip_sns_load_key_seeded, tfhe_hip_sns_pks_load_key_seeded, Squasher / SquashedPacker.load_compressed_key): the
expansion kernel against the host decompression word for word with the guard words behind it intact, the loaders
against the host route (decompress + the existing loader) bit for bit, sequences of loads on one context, the
refusals, and the way from container bytes to decrypted messages with no secret on the server side.  Every input is a
valid size or is refused on the host before a launch."""
import ctypes

import numpy as np
import pytest

import sns_pks_ref as R
import sns_seeded_cases as C
import tfhe_amd
from tfhe_amd import keyio
from tfhe_amd import sns as S
from tfhe_amd import sns_compression as SC
from test_decompress import with_n

pytestmark = pytest.mark.gpu

GUARD_WORD = np.uint64(0xA5A5A5A5A5A5A5A5)
EINVAL = -1                                     # TFHE_HIP_EINVAL
CHUNK_ENV = "TFHE_HIP_SNS_SEEDED_CHUNK"         # GGSWs per chunk of the squashing-key loader, read at every load


def _rand_words(count, salt):
    return np.random.default_rng(0x5EED128 + salt).integers(0, 1 << 64, count, dtype=np.uint64)


def _intact(guard):
    assert guard.size == S.SEEDED_GUARD_WORDS and np.all(guard == GUARD_WORD), "the kernel wrote behind its output"


@pytest.fixture(scope="module")
def squashers():
    """n -> a Squasher of the preset at that n, shared by the tests of this module"""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = S.Squasher(C.squash_params(n), 0)
        return cache[n]

    yield get
    for s in cache.values():
        s.close()


# ------------------------------------------------------------------ the kernel against the host, word for word
def _squash_pair(sq, n, seed, salt):
    sp = C.squash_params(n)
    ckey = S.CompressedSquashedKey(sp, seed, _rand_words(n * sp.level * (sp.k + 1) * 2 * sp.N, salt))
    dev, guard = sq.seeded_expand(ckey)
    _intact(guard)
    return dev, ckey.decompress().bsk


# chunk None: the whole key in one launch (75 GGSWs per chunk); 1 and 2: launches whose first row is not row 0; n = 76
# with the default chunk: a launch of 75 GGSWs and one of the last GGSW alone
@pytest.mark.parametrize("n,chunk", [(1, None), (2, None), (3, None), (3, "1"), (3, "2"), (76, None)])
def test_squashing_rows(squashers, monkeypatch, n, chunk):
    if chunk is None:
        monkeypatch.delenv(CHUNK_ENV, raising=False)
    else:
        monkeypatch.setenv(CHUNK_ENV, chunk)
    dev, ref = _squash_pair(squashers(n), n, C.MASK_SEED, n)
    assert np.array_equal(dev, ref)


def test_seeds_that_differ_in_the_top_byte(squashers, monkeypatch):
    """the key schedule runs once per seed on the host: every byte of the seed must reach it"""
    monkeypatch.delenv(CHUNK_ENV, raising=False)
    a, ref_a = _squash_pair(squashers(1), 1, C.MASK_SEED, 50)
    b, ref_b = _squash_pair(squashers(1), 1, C.MASK_SEED_TOP, 50)
    assert np.array_equal(a, ref_a) and np.array_equal(b, ref_b)
    sp = C.squash_params(1)
    ma, mb = (x.reshape(-1, sp.k + 1, 2, sp.N)[:, :sp.k] for x in (a, b))
    assert not np.array_equal(ma, mb)
    assert np.array_equal(a.reshape(-1, sp.k + 1, 2, sp.N)[:, sp.k], b.reshape(-1, sp.k + 1, 2, sp.N)[:, sp.k])


# (in_dim, out_k, out_N, level): the smallest ring at one level; three levels (the reversal); the preset's output
# shape; N = 2048 (one full pass of the kernel); N = 4096 (two passes)
PACK_SHAPES = [(16, 1, 32, 1), (16, 1, 64, 3), (32, 6, 1024, 1), (16, 2, 2048, 1), (16, 1, 4096, 1)]


@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_packing_rows(shape):
    in_dim, out_k, out_N, level = shape
    pp = C.packing_params(*shape)
    ckey = SC.CompressedSquashedCompressionKey(pp, C.MASK_SEED, _rand_words(in_dim * level * 2 * out_N, out_N + level))
    packer = SC.SquashedPacker(pp, 0)
    try:
        dev, guard = packer.seeded_expand(ckey)
    finally:
        packer.close()
    _intact(guard)
    assert np.array_equal(dev, ckey.decompress().pksk)
    # level reversal: storage row s lands in engine row level - 1 - s
    bodies = dev.reshape(in_dim, level, out_k + 1, 2, out_N)[:, ::-1, out_k].transpose(0, 1, 3, 2)
    assert np.array_equal(bodies, ckey.bodies)


# ------------------------------------------------------------------ the loaders against the host route, bit for bit
N_LOAD, B_LOAD = 7, 33                          # 33 ciphertexts cross the MAC's group of 32


@pytest.fixture(scope="module")
def load_inputs():
    msgs = np.arange(B_LOAD, dtype=np.uint64) % 16
    x = C.small_inputs(N_LOAD, msgs)
    x.setflags(write=False)
    return msgs, x


def _run(sq, x):
    return sq.blind_rotate(x), sq.squash(x)


@pytest.mark.parametrize("chunk", [None, "3"])           # "3": chunks of 3, 3 and 1 GGSWs through the staging buffer
def test_squasher_load_sequence(squashers, load_inputs, monkeypatch, chunk):
    """unseeded A -> seeded B -> unseeded B -> seeded A on one context: accumulators and outputs of each seeded load
    equal those of the host route for the same key, and differ between the keys"""
    if chunk is None:
        monkeypatch.delenv(CHUNK_ENV, raising=False)
    else:
        monkeypatch.setenv(CHUNK_ENV, chunk)
    msgs, x = load_inputs
    sp, key, ck_a, dk_a = C.squash_keys(N_LOAD)
    _, _, ck_b, dk_b = C.squash_keys(N_LOAD, C.MASK_SEED_TOP)
    sq = squashers(N_LOAD)
    acc_a, out_a = _run(sq.load_key(dk_a), x)
    acc_sb, out_sb = _run(sq.load_compressed_key(ck_b), x)
    acc_b, out_b = _run(sq.load_key(dk_b), x)
    acc_sa, out_sa = _run(sq.load_compressed_key(ck_a), x)
    assert np.array_equal(acc_sb, acc_b) and np.array_equal(out_sb, out_b)
    assert np.array_equal(acc_sa, acc_a) and np.array_equal(out_sa, out_a)
    assert not np.array_equal(out_a, out_b)
    assert np.array_equal(key.decrypt(out_sa), msgs) and np.array_equal(key.decrypt(out_sb), msgs)
    st = sq.seeded_load_stats()
    assert all(v >= 0 for v in st.values()) and st["expand_ms"] > 0


def test_packer_load_sequence():
    """pack at count = lwe_per_glwe + 1 (a full group and a group of one), unseeded -> seeded -> unseeded"""
    pp, key, ckey, dk = C.packing_keys(32, 1, 64, 3)
    _, _, ckey2, dk2 = C.packing_keys(32, 1, 64, 3, in_key_seed=8)
    count = pp.lwe_per_glwe + 1
    msgs = np.arange(count, dtype=np.uint64) % 16
    x = R.encrypt(pp, key.in_key, msgs)
    packer = SC.SquashedPacker(pp, 0)
    try:
        ref2 = packer.load_key(dk2).pack(x)
        got = packer.load_compressed_key(ckey).pack(x)
        ref = packer.load_key(dk).pack(x)
        got2 = packer.load_compressed_key(ckey2).pack(x)
        assert packer.seeded_load_stats()["expand_ms"] > 0
    finally:
        packer.close()
    assert got.shape == (2, pp.out_k + 1, 2, pp.out_N)
    assert np.array_equal(got, ref) and np.array_equal(got2, ref2) and not np.array_equal(ref, ref2)
    assert np.array_equal(got, SC.pack_host(pp, dk.pksk, x))
    assert np.array_equal(SC.decrypt_list(key, SC._compress_groups(pp, got, count)), msgs)


# n = 76 is the smallest n whose 27 n = 2052 polynomials exceed both the unseeded loader's chunk of 2048 polynomials and
# the seeded loader's 75 GGSWs: every smaller n is one chunk on both routes
N_EDGE = 76


@pytest.fixture(scope="module")
def edge_keys():
    """two keys of random body words at N_EDGE (no real keys: the routes are compared with each other) and their
    host decompressions, built once and left read-only"""
    sp = C.squash_params(N_EDGE)
    out = []
    for seed in (C.MASK_SEED, C.MASK_SEED_TOP):
        ck = S.CompressedSquashedKey(sp, seed, _rand_words(N_EDGE * sp.level * (sp.k + 1) * 2 * sp.N, N_EDGE))
        dk = ck.decompress()
        ck.bodies.setflags(write=False)
        dk.bsk.setflags(write=False)
        out += [ck, dk]
    return out


# None: chunks of 75 GGSWs and 1; "7": ten chunks of 7 and a tail of 6.  The unseeded loads: 2048 polynomials and 4
@pytest.mark.parametrize("chunk", [None, "7"])
def test_chunk_edges_of_both_sources(squashers, edge_keys, monkeypatch, chunk):
    """unseeded A -> seeded B -> unseeded B -> seeded A at n = 76, where both loaders run a second chunk: the
    accumulator and the output of one ciphertext after each seeded load equal those of the host route, bit for bit"""
    if chunk is None:
        monkeypatch.delenv(CHUNK_ENV, raising=False)
    else:
        monkeypatch.setenv(CHUNK_ENV, chunk)
    ck_a, dk_a, ck_b, dk_b = edge_keys
    x = _rand_words(N_EDGE + 1, 7600).reshape(1, N_EDGE + 1)
    sq = squashers(N_EDGE)
    acc_a, out_a = _run(sq.load_key(dk_a), x)
    acc_sb, out_sb = _run(sq.load_compressed_key(ck_b), x)
    acc_b, out_b = _run(sq.load_key(dk_b), x)
    acc_sa, out_sa = _run(sq.load_compressed_key(ck_a), x)
    assert np.array_equal(acc_sb, acc_b) and np.array_equal(out_sb, out_b)
    assert np.array_equal(acc_sa, acc_a) and np.array_equal(out_sa, out_a)
    assert not np.array_equal(acc_a, acc_b) and not np.array_equal(out_a, out_b)


# ------------------------------------------------------------------ refusals
def _refuses(load, ctx, words):
    """null context, null words and the lengths len - 1, len + 1 and 0: EINVAL each"""
    assert load(None, tfhe_amd._u64(words), words.size) == EINVAL
    assert load(ctx, None, words.size) == EINVAL
    for wrong in (words.size - 1, words.size + 1, 0):
        assert load(ctx, tfhe_amd._u64(words), wrong) == EINVAL


def test_refused_unseeded_loads_leave_the_resident_key(squashers, load_inputs):
    _, x = load_inputs
    sp, key, ckey, dk = C.squash_keys(N_LOAD)
    sq = squashers(N_LOAD)
    before = sq.load_key(dk).squash(x)
    _refuses(S._lib().tfhe_hip_sns_load_key, sq._h, np.ascontiguousarray(dk.bsk).ravel())
    assert np.array_equal(sq.squash(x), before)

    pp, pkey, pck, pdk = C.packing_keys(32, 1, 64, 3)
    lw = R.encrypt(pp, pkey.in_key, np.arange(5, dtype=np.uint64))
    packer = SC.SquashedPacker(pp, 0)
    try:
        pbefore = packer.load_key(pdk).pack(lw)
        _refuses(SC._lib().tfhe_hip_sns_pks_load_key, packer._h, np.ascontiguousarray(pdk.pksk).ravel())
        assert np.array_equal(packer.pack(lw), pbefore)
    finally:
        packer.close()


def test_refused_loads_leave_the_resident_key(squashers, load_inputs, monkeypatch):
    monkeypatch.delenv(CHUNK_ENV, raising=False)
    _, x = load_inputs
    sp, key, ckey, dk = C.squash_keys(N_LOAD)
    sq = squashers(N_LOAD)
    before = sq.load_key(dk).squash(x)
    L = S._lib()
    b = np.ascontiguousarray(ckey.bodies).ravel()
    seed = tfhe_amd._u64(S.seed_words(ckey.seed))
    assert L.tfhe_hip_sns_load_key_seeded(sq._h, seed, None, b.size) == EINVAL
    assert L.tfhe_hip_sns_load_key_seeded(sq._h, None, tfhe_amd._u64(b), b.size) == EINVAL
    assert L.tfhe_hip_sns_load_key_seeded(None, seed, tfhe_amd._u64(b), b.size) == EINVAL
    for wrong in (b.size - 2, b.size + 2, 0, b.size // 3):
        assert L.tfhe_hip_sns_load_key_seeded(sq._h, seed, tfhe_amd._u64(b), wrong) == EINVAL
    assert np.array_equal(sq.squash(x), before)

    pp, pkey, pck, pdk = C.packing_keys(32, 1, 64, 3)
    lw = R.encrypt(pp, pkey.in_key, np.arange(5, dtype=np.uint64))
    packer = SC.SquashedPacker(pp, 0)
    try:
        pbefore = packer.load_key(pdk).pack(lw)
        P = SC._lib()
        pb = np.ascontiguousarray(pck.bodies).ravel()
        assert P.tfhe_hip_sns_pks_load_key_seeded(packer._h, seed, None, pb.size) == EINVAL
        assert P.tfhe_hip_sns_pks_load_key_seeded(packer._h, None, tfhe_amd._u64(pb), pb.size) == EINVAL
        assert P.tfhe_hip_sns_pks_load_key_seeded(None, seed, tfhe_amd._u64(pb), pb.size) == EINVAL
        for wrong in (pb.size - 2, pb.size + 2, 0):
            assert P.tfhe_hip_sns_pks_load_key_seeded(packer._h, seed, tfhe_amd._u64(pb), wrong) == EINVAL
        assert np.array_equal(packer.pack(lw), pbefore)
    finally:
        packer.close()


# ------------------------------------------------------------------ container bytes -> decrypted messages
def test_container_to_decrypted_messages(monkeypatch):
    """The client issues the container; the server holds its bytes only: loads_compressed_server_key ->
    load_compressed_key on both contexts -> squash, pack, compress; the client decrypts the list.  n = 7, packing key
    in_dim 4096 -> k = 1, N = 128, 4 per GLWE; 6 ciphertexts: one full group and a group of two."""
    monkeypatch.delenv(CHUNK_ENV, raising=False)
    ck, _ = tfhe_amd.gen_keys(with_n(tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_FFT), N_LOAD), 0x5EED0E2E,
                              with_server_key=False)
    sq_key = S.SquashedKey(C.squash_params(N_LOAD), C.RNG_SEED, ck.lwe_key, with_bsk=False)
    comp_key = SC.SquashedCompressionKey(C.packing_params(4096, 1, 128, 1, lwe_per_glwe=4), C.RNG_SEED,
                                         sq_key.glwe_key, with_key=False)
    blob = keyio.dumps_compressed_server_key(
        keyio.compress_server_key(ck, seed=0x5EED0E2F, squashing=sq_key, squashed_compression=comp_key))
    msgs = np.array([3, 0, 15, 8, 7, 12], dtype=np.uint64)
    small = C.small_inputs(N_LOAD, msgs, key=ck.lwe_key)

    csk = keyio.loads_compressed_server_key(blob)                       # the server side: bytes only
    squasher = S.Squasher(csk.squashing.params, 0)
    packer = SC.SquashedPacker(csk.squashed_compression.params, 0)
    try:
        squashed = squasher.load_compressed_key(csk.squashing).squash(small)
        comp = packer.load_compressed_key(csk.squashed_compression).compress_squashed_into_list(squashed)
    finally:
        squasher.close()
        packer.close()
    assert [c.bodies for c in comp] == [4, 2]
    assert np.array_equal(sq_key.decrypt(squashed), msgs)
    assert np.array_equal(SC.decrypt_list(comp_key, comp), msgs)
