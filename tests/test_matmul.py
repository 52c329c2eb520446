"""Encrypted matrix x clear matrix without a GPU (tfhe_amd/matmul.py, the host functions of tfhe_hip_matmul_*):
the closed form of the dot product against the literal polynomial product plus extraction, the host encrypt / expand /
dot / decode functions against the numpy restatement (tests/matmul_ref.py), argument checks, and the whole chain at
N = 256 with the oracle's packing keyswitch as the packing stage.  Every comparison of ciphertext words is an integer
equality."""
import ctypes

import numpy as np
import pytest

import matmul_ref as REF
import tfhe_amd
from tfhe_amd import compression as C
from tfhe_amd import matmul as MM

U64 = 2 ** 64 - 1
STORAGE_LOGS = (39, 33, 64)   # 33: values straddle words; 64: no switch


def full_range_glwes(rng, shape):
    return rng.integers(0, U64, size=shape, dtype=np.uint64, endpoint=True)


# ---- the restatement itself ----------------------------------------------------------------------------------
def test_closed_form_equals_literal_form():
    """N = 64, two K-blocks with a ragged second one, full-range masks and bodies, int32 weights with INT32_MIN, -1, 0
    and INT32_MAX planted: the vectorised closed form equals the schoolbook product plus extraction at N - 1."""
    N, R, K, Cc = 64, 2, 67, 3
    rng = np.random.default_rng(1)
    g = full_range_glwes(rng, (R, 2, 2, N))
    W = REF.plant_weights(rng.integers(-2 ** 31, 2 ** 31, size=(K, Cc), dtype=np.int64))
    closed = REF.dot_closed(g, W, N)
    for r in range(R):
        for c in range(Cc):
            lit = REF.dot_literal([[g[r, kb, 0], g[r, kb, 1]] for kb in range(2)], W[:, c], N)
            assert [int(x) for x in closed[r, c]] == lit, (r, c)


def test_literal_extraction_matches_compression_extract_lwe():
    """The restated tfhe-rs extraction rule equals compression.extract_lwe (written independently) at every degree
    class: 0, 1, the middle, N - 1."""
    N = 64
    pp = C.PksParams(N, 1, N, 14, 2, N, 26, -48)
    g = full_range_glwes(np.random.default_rng(2), (2, N))
    for n in (0, 1, 31, N - 1):
        assert REF.extract_lwe([[int(x) for x in g[0]], [int(x) for x in g[1]]], n) == \
            [int(x) for x in C.extract_lwe(pp, g, n)]


# ---- host functions against the restatement ------------------------------------------------------------------
def test_preset():
    mp = MM.MatmulParams.preset()
    assert (mp.N, mp.bits_reserved, mp.in_storage_log, mp.noise_log2) == (2048, 27, 39, -48)
    assert mp.body_words == 2048 * 39 // 64


@pytest.fixture(scope="module")
def encrypt_case():
    """Two GLWEs of N = 64 under one key, encrypted at every storage width with the same seeds and noise streams."""
    N, b = 64, 20
    rk = tfhe_amd.rng_key(77)
    key = np.zeros(N, dtype=np.uint64)
    assert MM._lib().tfhe_hip_matmul_keygen_k(ctypes.byref(MM.MatmulParams(N, b, 64, -48)), ctypes.byref(rk),
                                            tfhe_amd._u64(key)) == 0
    rng = np.random.default_rng(3)
    seeds = full_range_glwes(rng, (2, 2))
    values = rng.integers(-2 ** (b - 1), 2 ** (b - 1), size=(2, N), dtype=np.int64)
    values[0, :4] = (-2 ** (b - 1), 2 ** (b - 1) - 1, -1, 0)
    packed = {w: MM.encrypt_glwes(MM.MatmulParams(N, b, w, -48), key, rk, 5, seeds, values) for w in STORAGE_LOGS}
    return N, b, rk, key, seeds, values, packed


def test_key_is_binary_and_seeded(encrypt_case):
    N, b, rk, key, *_ = encrypt_case
    assert set(np.unique(key)) == {0, 1}
    other = np.zeros(N, dtype=np.uint64)
    MM._lib().tfhe_hip_matmul_keygen_k(ctypes.byref(MM.MatmulParams(N, b, 64, -48)), ctypes.byref(tfhe_amd.rng_key(78)),
                                       tfhe_amd._u64(other))
    assert not np.array_equal(key, other)


def test_encrypt_full_width_is_mask_key_noise_message(encrypt_case):
    """in_storage_log = 64 stores the body unswitched: body - A*S - v*delta is the noise, exactly: its first word is
    the first Gaussian of ChaCha stream stream0 + g (read back through tfhe_hip_seeded_lwe_list_k with a zero key),
    all words are small and the two GLWEs' noises differ."""
    N, b, rk, key, seeds, values, packed = encrypt_case
    mp = MM.MatmulParams(N, b, 64, -48)
    glwes = MM.expand_host(mp, seeds, packed[64])
    L = tfhe_amd.lib()
    noises = []
    for g in range(2):
        mask = np.zeros(N, dtype=np.uint64)
        L.tfhe_hip_csprng_words(tfhe_amd._u64(np.ascontiguousarray(seeds[g])), 0, N, tfhe_amd._u64(mask))
        assert np.array_equal(glwes[g, 0], mask)
        phase = C.glwe_phase(1, N, key, glwes[g].reshape(-1))
        e = [(int(phase[t]) - REF.encode(values[g, t], b)) & U64 for t in range(N)]
        e = [x - (1 << 64) if x >> 63 else x for x in e]
        assert max(abs(x) for x in e) < 2 ** (64 - 48 + 3) and any(e)      # 8 sigma
        first = np.zeros(1, dtype=np.uint64)
        zero_key = np.zeros(1, dtype=np.uint64)
        sd = np.ascontiguousarray(seeds[g])
        assert L.tfhe_hip_seeded_lwe_list_k(1, 1, tfhe_amd._u64(zero_key), -48, ctypes.byref(rk), ctypes.c_uint64(5 + g),
                                            tfhe_amd._u64(sd), None, tfhe_amd._u64(first)) == 0
        assert e[0] & U64 == int(first[0])
        noises.append(e)
    assert noises[0] != noises[1]


@pytest.mark.parametrize("w", [39, 33])
def test_encrypt_switches_and_packs_as_the_restatement(encrypt_case, w):
    """The same seeds and streams give the same full-width body at every storage width; the stored words equal the
    restated switch and LSB-first packing of it, each GLWE on its own word boundary."""
    N, b, rk, key, seeds, values, packed = encrypt_case
    mp = MM.MatmulParams(N, b, w, -48)
    assert mp.body_words == -(-N * w // 64) and packed[w].shape == (2, mp.body_words)
    for g in range(2):
        body = packed[64][g]
        want = REF.pack_bits([REF.storage_switch(x, w) for x in body], w)
        assert np.array_equal(packed[w][g], want)


@pytest.mark.parametrize("w", STORAGE_LOGS)
def test_expand_host_equals_restatement(w):
    N, G = 64, 3
    mp = MM.MatmulParams(N, 20, w, -48)
    rng = np.random.default_rng(4 + w)
    seeds = full_range_glwes(rng, (G, 2))
    packed = full_range_glwes(rng, (G, mp.body_words))     # any bits, the spare ones of the last word included
    got = MM.expand_host(mp, seeds, packed)
    for g in range(G):
        mask = np.zeros(N, dtype=np.uint64)
        tfhe_amd.lib().tfhe_hip_csprng_words(tfhe_amd._u64(np.ascontiguousarray(seeds[g])), 0, N, tfhe_amd._u64(mask))
        assert np.array_equal(got[g, 0], mask)
        assert np.array_equal(got[g, 1], REF.expand_body(packed[g], N, w))


def test_dot_host_equals_restatement():
    """Two K-blocks with a ragged second, a column stride above C: bit-exact, and the LWEs past C keep their words."""
    N, R, K, Cc, stride = 64, 2, 67, 5, 7
    mp = MM.MatmulParams(N, 20, 39, -48)
    rng = np.random.default_rng(5)
    g = full_range_glwes(rng, (R, 2, 2, N))
    W = REF.plant_weights(rng.integers(-2 ** 31, 2 ** 31, size=(K, Cc), dtype=np.int64))
    out = np.full((R, stride, N + 1), 0x5E5E5E5E5E5E5E5E, dtype=np.uint64)
    MM.dot_host(mp, W, g, col_stride=stride, out=out)
    assert np.array_equal(out[:, :Cc], REF.dot_closed(g, W, N))
    assert (out[:, Cc:] == 0x5E5E5E5E5E5E5E5E).all()


@pytest.mark.parametrize("b", [1, 2, 20, 27, 63])
def test_decode_sign_boundary_and_rounding(b):
    """2^(b-1) - 1 is the largest positive value and 2^(b-1) the most negative one; half a delta rounds up."""
    mp = MM.MatmulParams(64, b, 39, -48)
    delta = 1 << (64 - b)
    vals = [(1 << (b - 1)) - 1, 1 << (b - 1), 0, (1 << b) - 1]
    phases = [(v * delta) & U64 for v in vals]
    phases += [(p + delta // 2 - 1) & U64 for p in phases[:1]] + [(phases[0] + (delta + 1) // 2) & U64]
    if delta > 1:
        phases.append((phases[1] - delta // 2 - 1) & U64)      # just below the tie under 2^(b-1): rounds to 2^(b-1) - 1
    got = MM.decode(mp, np.array(phases, dtype=np.uint64))
    assert [int(x) for x in got] == [REF.decode(p, b) for p in phases]
    assert int(got[0]) == (1 << (b - 1)) - 1 and int(got[1]) == -(1 << (b - 1)) and int(got[3]) == -1


# ---- argument checks -------------------------------------------------------------------------------------------
BAD_PARAMS = [(32, 20, 39, -48), (8192, 20, 39, -48), (96, 20, 39, -48), (64, 0, 39, -48), (64, 64, 39, -48),
              (64, 20, 0, -48), (64, 20, 65, -48), (64, 20, 39, 0), (64, 20, 39, -64)]


@pytest.mark.parametrize("fields", BAD_PARAMS)
def test_bad_parameters_are_refused(fields):
    """EINVAL from every entry point, create included (the parameter check comes before any device work)."""
    mp = MM.MatmulParams(*fields)
    L = MM._lib()
    assert L.tfhe_hip_matmul_body_words(ctypes.byref(mp)) == 0
    with pytest.raises(ValueError):
        mp.body_words
    h = ctypes.c_void_p()
    assert L.tfhe_hip_matmul_create(ctypes.byref(mp), 0, ctypes.byref(h)) == -1 and not h.value
    buf = np.zeros(2 * 8192 + 2, dtype=np.uint64)
    out = np.zeros(8, dtype=np.int64)
    assert L.tfhe_hip_matmul_decode(ctypes.byref(mp), tfhe_amd._u64(buf), 1, out.ctypes.data_as(MM._I64P)) == -1
    assert L.tfhe_hip_matmul_keygen_k(ctypes.byref(mp), ctypes.byref(tfhe_amd.rng_key(1)), tfhe_amd._u64(buf)) == -1
    with pytest.raises(ValueError):
        MM.MatMul(mp, None, "cpu")


def test_valid_edges_are_accepted():
    for fields in [(64, 1, 1, -1), (4096, 63, 64, -63)]:
        assert MM.MatmulParams(*fields).body_words == -(-fields[0] * fields[2] // 64)


def test_empty_and_out_of_range_matrices_are_refused():
    mp = MM.MatmulParams(64, 20, 39, -48)
    cpu = MM.MatMul(mp, None, "cpu")
    for bad in (np.zeros((0, 3), dtype=np.int64), np.zeros((3, 0), dtype=np.int64), np.zeros(3, dtype=np.int64),
                np.array([[2 ** 31]]), np.array([[-2 ** 31 - 1]]), np.array([[0.5]])):
        with pytest.raises(ValueError):
            cpu.clear_matrix(bad)
        with pytest.raises(ValueError):
            MM.dot_host(mp, bad, np.zeros((1, 1, 2, 64), dtype=np.uint64))
    assert cpu.clear_matrix(np.array([[2 ** 31 - 1, -2 ** 31]])).w.dtype == np.int32
    # the C ABI itself: K = 0, C = 0, col_stride < C
    L = MM._lib()
    w = np.zeros(4, dtype=np.int32)
    g = np.zeros(2 * 64, dtype=np.uint64)
    out = np.zeros(4 * 65, dtype=np.uint64)
    for K, Cc, stride in ((0, 2, 2), (2, 0, 2), (1, 2, 1)):
        assert L.tfhe_hip_matmul_dot_host(ctypes.byref(mp), w.ctypes.data_as(MM._I32P), K, Cc, tfhe_amd._u64(g), 1, stride,
                                          tfhe_amd._u64(out)) == -1
    with pytest.raises(ValueError):
        MM.encrypt_matrix(REF.chain_case().pkey, np.zeros((0, 4), dtype=np.int64))
    with pytest.raises(ValueError):
        MM.PrivateKey(mp, C.PksParams(128, 1, 128, 14, 2, 128, 26, -48), 1)     # pks in_dim != N


def test_abi_symbols_are_exported():
    names = [s for s in tfhe_amd.ABI_SYMBOLS if s.startswith("tfhe_hip_matmul_")]
    assert len(names) == 15
    for s in names:
        assert hasattr(tfhe_amd.lib(), s)


# ---- the whole chain on the CPU ----------------------------------------------------------------------------------
def test_cpu_chain_shapes():
    case = REF.chain_case()
    assert case.enc.seeds.shape == (2 * 2, 2) and case.enc.packed.shape == (4, 256 * 39 // 64)
    assert [[cg.bodies for cg in row] for row in case.cpu_result] == [[256, 5], [256, 5]]
    assert case.mp.bits_reserved == case.width + 1 and case.mp.N == REF.CHAIN_N


def test_cpu_chain_decrypts_to_the_product():
    """The reference's criterion (ml/extensions/tests/test_matmul.py:64-186, conftest.py:7-8) on the CPU chain: the 12
    most significant bits agree on all but at most 1 % of the entries.  This also pins that the committed seeds stay
    inside the cap the GPU test relies on."""
    case = REF.chain_case()
    got = MM.decrypt_matrix(case.cpu_result, case.pkey, REF.CHAIN_C)
    assert got.shape == case.expected.shape
    bad = REF.msb_mismatches(got, case.expected, case.width)
    print(f"bit width {case.width}, {bad} of {got.size} entries differ on the 12 MSBs, max |error| "
          f"{np.abs(got - case.expected).max()}")
    assert bad <= got.size // 100


def test_cpu_chain_dot_stage_equals_restatement():
    """The LWEs between dot and packing, from the chain's own ciphertexts: host expand + host dot == restatement."""
    case = REF.chain_case()
    mp = case.mp
    glwes = MM.expand_host(mp, case.enc.seeds, case.enc.packed).reshape(2, 2, 2, mp.N)
    assert np.array_equal(MM.dot_host(mp, case.W, glwes), REF.dot_closed(glwes, case.W, mp.N))


def test_second_matrix_gives_other_words():
    case = REF.chain_case()
    assert not np.array_equal(case.cpu_result[0][0].packed, case.cpu_result2[0][0].packed)
