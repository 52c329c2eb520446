"""Seeded multi-bit bootstrapping keys on the CPU (include/tfhe_hip.h, tfhe_amd/csrc/seeded.cpp, tfhe_amd/keyio.py).

At PRESET_FHEVM_MB_FFT with n reduced to g and 2g, g in {2, 3, 4}: every row of a host-decompressed key decrypts under
the GLWE key to indicator x (the plaintext tfhe-rs puts in that row); the sigma = 0 GGSW that only the container holds
encrypts the all-zero indicator; tfhe_hip_decompress_bsk_mb equals its definition word for word; the container round
trips for grouping 1 .. 4 and rejects truncation and a wrong grouping factor; the two host calls refuse what
tfhe_hip_load_keys_mb refuses.  The byte layout of a real tfhe-rs multi-bit CompressedServerKey is PARITY UNPINNED."""
import ctypes
import struct

import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import keyio
from test_decompress import with_n

N, K, L_PBS, BASE_LOG = 2048, 1, 1, 23
GS = (2, 3, 4)
TOL_LOG2 = 45            # the bound of tests/test_seeded.py _rows_decrypt
# That bound lies above this gadget's plaintext g_0 = 2^41, so alone it cannot tell a live row from a dead one.  The
# rows' own noise is Gaussian with sigma = 2^(64 - 47) = 2^17; 2^22 is 32 sigma, far beyond the largest of the few
# million samples drawn here and far below 2^41.
NOISE_LOG2 = 22
BSK_SEED = 0x0123456789ABCDEF_0F1E2D3C4B5A6978
TAIL = 32 + 24 + 4 + 4 + 4 + 8   # container bytes behind the bootstrapping key: moduli, ciphertext modulus, order, Options, Tag


def mb_params(n: int):
    return with_n(tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_MB_FFT), n)


def glwe_key() -> np.ndarray:
    """a binary GLWE key of 48 ones: the phase check below costs one rotation per one"""
    s = np.zeros(N, dtype=np.uint64)
    s[np.random.default_rng(0x61E).choice(N, 48, replace=False)] = 1
    s[[0, N - 1]] = 1
    return s


def lwe_keys(g: int, n: int):
    """secret keys under which every sigma in 0 .. 2^g - 1 is the live indicator of some group of some key"""
    groups = n // g
    for j in range(-(-(1 << g) // groups)):
        sig = [(j * groups + q) % (1 << g) for q in range(groups)]
        yield np.array([(sig[q] >> i) & 1 for q in range(groups) for i in range(g)], dtype=np.uint64), sig


def words(seed: int, first: int, count: int) -> np.ndarray:
    out = np.zeros(count, dtype=np.uint64)
    tfhe_amd._check(tfhe_amd.lib().tfhe_hip_csprng_words(tfhe_amd._u64(keyio._seed2(seed)), first, count,
                                                          tfhe_amd._u64(out)))
    return out


def mb_bodies(p, g: int, lwe: np.ndarray, S: np.ndarray, seed: int = BSK_SEED, rk_seed: int = 0x5EEDB0D1) -> np.ndarray:
    L = tfhe_amd.lib()
    b = np.zeros(L.tfhe_hip_seeded_mb_bodies_len(ctypes.byref(p), g), dtype=np.uint64)
    rk = tfhe_amd.rng_key(rk_seed)
    tfhe_amd._check(L.tfhe_hip_seeded_mb_server_keygen_k(ctypes.byref(p), g, ctypes.byref(rk),
                                                         tfhe_amd._u64(keyio._seed2(seed)), tfhe_amd._u64(lwe),
                                                         tfhe_amd._u64(S), tfhe_amd._u64(b)))
    return b.reshape(p.n // g, 1 << g, L_PBS, K + 1, N)


def decompress_mb(p, g: int, bodies: np.ndarray, seed: int = BSK_SEED) -> np.ndarray:
    L = tfhe_amd.lib()
    out = np.zeros(L.tfhe_hip_mb_bsk_len(ctypes.byref(p), g), dtype=np.uint64)
    tfhe_amd._check(L.tfhe_hip_decompress_bsk_mb(ctypes.byref(p), g, tfhe_amd._u64(keyio._seed2(seed)),
                                                 tfhe_amd._u64(np.ascontiguousarray(bodies)), tfhe_amd._u64(out)))
    return out.reshape(p.n // g, (1 << g) - 1, L_PBS, K + 1, (K + 1) * N)


def row_error(row: np.ndarray, S: np.ndarray, live: bool, l: int, c: int) -> int:
    """max |phase - indicator x plaintext| of one GGSW row (mask | body) in tfhe-rs's form"""
    with np.errstate(over="ignore"):
        phase = row[K * N:] - keyio.negacyclic_mul_binary(row[:K * N], S)
        gl = np.uint64(1 << (64 - BASE_LOG * (l + 1)))
        want = np.zeros(N, dtype=np.uint64)
        if live:
            if c < K:
                want -= gl * S
            else:
                want[0] = gl
        return int(np.abs((phase - want).view(np.int64)).max())


@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("mult", [1, 2])
def test_rows_decrypt_and_match_the_definition(g, mult):
    n = g * mult
    p, S = mb_params(n), glwe_key()
    seen = set()
    for lwe, sig in lwe_keys(g, n):
        bodies = mb_bodies(p, g, lwe, S)
        key = decompress_mb(p, g, bodies)
        for q in range(n // g):
            seen.add(sig[q])
            for sigma in range(1 << g):
                for l in range(L_PBS):
                    for c in range(K + 1):
                        rho = ((q * (1 << g) + sigma) * L_PBS + l) * (K + 1) + c
                        mask = words(BSK_SEED, rho * K * N, K * N)
                        row = np.concatenate([mask, bodies[q, sigma, l, c]])
                        if sigma:   # the numpy restatement: stream rows by rho, keep sigma >= 1, [q][sigma - 1][l][c]
                            assert np.array_equal(key[q, sigma - 1, l, c], row), (q, sigma, l, c)
                        # sigma = 0 lives in the container only: it encrypts the all-zero indicator
                        err = row_error(row, S, sig[q] == sigma, l, c)
                        assert err < 2 ** TOL_LOG2 and err < 2 ** NOISE_LOG2, (q, sigma, l, c, err)
    assert seen == set(range(1 << g))


def test_the_live_plaintext_is_not_noise():
    """the check above can tell a live row from a dead one: the plaintext is far above the noise bound"""
    p, S = mb_params(2), glwe_key()
    lwe = np.array([1, 0], dtype=np.uint64)                       # sigma = 1 is live
    key = decompress_mb(p, 2, mb_bodies(p, 2, lwe, S))
    for c in range(K + 1):
        assert row_error(key[0, 0, 0, c], S, True, 0, c) < 2 ** NOISE_LOG2 <= row_error(key[0, 0, 0, c], S, False, 0, c)
        assert row_error(key[0, 1, 0, c], S, False, 0, c) < 2 ** NOISE_LOG2 <= row_error(key[0, 1, 0, c], S, True, 0, c)


@pytest.fixture(scope="module")
def key_sets():
    """grouping -> (ClientKey, CompressedServerKey) at n = 12"""
    out = {}
    for g in (1, 2, 3, 4):
        ck, _ = tfhe_amd.gen_keys(mb_params(12), 0x5EED0B00 + g, with_server_key=False)
        out[g] = ck, keyio.compress_server_key(ck, seed=0x5EED0B10 + g, grouping=g)
    return out


@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_container_roundtrip(key_sets, g):
    ck, csk = key_sets[g]
    assert csk.grouping == g
    assert csk.bsk_bodies.shape == ((12, 1, 2, N) if g == 1 else (12 // g, 1 << g, 1, 2, N))
    blob = keyio.dumps_compressed_server_key(csk)
    back = keyio.loads_compressed_server_key(blob)
    assert back.grouping == g and back.params == csk.params
    assert (back.bsk_seed, back.ksk_seed) == (csk.bsk_seed, csk.ksk_seed)
    assert np.array_equal(back.bsk_bodies, csk.bsk_bodies) and back.bsk_bodies.shape == csk.bsk_bodies.shape
    assert np.array_equal(back.ksk_bodies, csk.ksk_bodies)
    assert keyio.dumps_compressed_server_key(back) == blob
    cuts = [len(blob) // 4, len(blob) // 2]
    if g > 1:
        cuts.append(len(blob) - TAIL - 4)                               # inside the grouping factor
    for cut in cuts:
        with pytest.raises(keyio.KeyFormatError):
            keyio.loads_compressed_server_key(blob[:cut])
    p2, sk = keyio.decompress_server_key(back)
    assert (p2.n, p2.N, sk.grouping) == (12, N, g)
    if g > 1:
        assert sk.ms_zeros is None and sk.bsk.size == tfhe_amd.lib().tfhe_hip_mb_bsk_len(ctypes.byref(p2), g)
        want = decompress_mb(p2, g, csk.bsk_bodies, csk.bsk_seed)
        assert np.array_equal(sk.bsk, want.reshape(-1))


def test_classic_container_bytes_unchanged(key_sets):
    """a classic key dumps with bootstrapping-key variant 0 and no grouping factor: the bytes of the earlier layout"""
    _, csk = key_sets[1]
    blob = keyio.dumps_compressed_server_key(csk)
    head = 8 + 3 + 4 + 8 + 3 + 8 + len(keyio.COMPRESSED_SERVER_KEY_TYPE) + 16
    ksk_end = head + 8 + 8 * csk.ksk_bodies.size + 24 + 4 + 16 + 24
    assert struct.unpack_from("<II", blob, ksk_end) == (0, 0)           # bootstrapping key tag, variant Classic
    bsk_end = ksk_end + 12 + 8 + 8 * csk.bsk_bodies.size + 32 + 4 + 16 + 24
    assert blob[bsk_end] == 0                                           # Option<MS key> = None follows at once
    assert len(blob) == bsk_end + 1 + TAIL


@pytest.mark.parametrize("g", [2, 3, 4])
def test_container_rejects_a_wrong_grouping_factor(key_sets, g):
    _, csk = key_sets[g]
    blob = bytearray(keyio.dumps_compressed_server_key(csk))
    at = len(blob) - TAIL - 8                                          # grouping_factor follows the BSK's modulus
    assert struct.unpack_from("<IQ", blob, at - 4) == (64, g)
    for wrong in (1, 5, 2 if g != 2 else 3):
        struct.pack_into("<Q", blob, at, wrong)
        with pytest.raises(keyio.KeyFormatError):
            keyio.loads_compressed_server_key(bytes(blob))
    with pytest.raises(keyio.KeyFormatError):
        bad = keyio.CompressedServerKey(csk.params, csk.bsk_seed, csk.bsk_bodies, csk.ksk_seed, csk.ksk_bodies,
                                        grouping=2 if g != 2 else 3)
        keyio.decompress_server_key(bad)


def test_host_calls_refuse_what_load_keys_mb_refuses():
    L = tfhe_amd.lib()
    S, seed = glwe_key(), tfhe_amd._u64(keyio._seed2(BSK_SEED))
    rk = tfhe_amd.rng_key(1)
    buf = np.zeros(16 * 2 * 2 * N, dtype=np.uint64)

    def both(p, g, lwe):
        a = L.tfhe_hip_seeded_mb_server_keygen_k(ctypes.byref(p), g, ctypes.byref(rk), seed, tfhe_amd._u64(lwe),
                                                 tfhe_amd._u64(S), tfhe_amd._u64(buf))
        b = L.tfhe_hip_decompress_bsk_mb(ctypes.byref(p), g, seed, tfhe_amd._u64(buf), tfhe_amd._u64(buf.copy()))
        assert a == b
        return a

    lwe = np.zeros(12, dtype=np.uint64)
    for g in (0, 1, 5):
        assert both(mb_params(12), g, lwe) == -1                          # EINVAL: g outside {2, 3, 4}
        assert L.tfhe_hip_seeded_mb_bodies_len(ctypes.byref(mb_params(12)), g) == 0
    assert both(mb_params(7), 2, lwe) == -1 and both(mb_params(8), 3, lwe) == -1     # n % g != 0
    gate = with_n(tfhe_amd.Params.preset(tfhe_amd.PRESET_GATE_FFT), 4)
    ntt = with_n(tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM), 4)
    assert both(gate, 2, lwe) == -5 and both(ntt, 2, lwe) == -5          # EUNSUPPORTED: N = 1024, the NTT transform
    assert L.tfhe_hip_seeded_mb_server_keygen_k(ctypes.byref(mb_params(4)), 2, ctypes.byref(rk), None,
                                                tfhe_amd._u64(lwe), tfhe_amd._u64(S), tfhe_amd._u64(buf)) == -1
    assert L.tfhe_hip_decompress_bsk_mb(ctypes.byref(mb_params(4)), 2, seed, None, tfhe_amd._u64(buf)) == -1
    lwe[1] = 2
    # a key word that is not binary is refused by the keygen
    assert L.tfhe_hip_seeded_mb_server_keygen_k(ctypes.byref(mb_params(4)), 2, ctypes.byref(rk), seed,
                                                tfhe_amd._u64(lwe), tfhe_amd._u64(S), tfhe_amd._u64(buf)) == -1
    assert L.tfhe_hip_seeded_mb_bodies_len(ctypes.byref(mb_params(12)), 3) == 4 * 8 * 2 * N
