"""Multi-bit PBS keys and their exact reference on the CPU (include/tfhe_hip.h, tests/multibit_ref.py): key sizes,
refusals that need no device, key streams against the classic keygen, the stored indicators, the reference's blind
rotation at toy n, and the sum-then-switch convention.  The device side is tests/test_gpu_multibit.py."""
import ctypes

import numpy as np
import pytest

from conftest import KEY_SEED
import multibit_ref as mb

import tfhe_amd

N = 2048
GS = (2, 3, 4)
DELTA = (1 << 63) // 16
TABLE = [(3 * v + 1) % 16 for v in range(16)]


def toy_params(n: int = 12):
    p = tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_MB_FFT)
    p.n = n
    return p


@pytest.fixture(scope="module")
def toy_keys():
    """g -> (ClientKey, multi-bit ServerKey) at n = 12, one secret key set for all three"""
    return {g: tfhe_amd.gen_keys(toy_params(), KEY_SEED, grouping=g) for g in GS}


def _phase(oracle_mod, ck, glwe):
    return oracle_mod.glwe_phase_native(1, N, ck.glwe_key, np.ascontiguousarray(glwe, dtype=np.uint64))


def test_preset_and_bsk_len():
    p = tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_MB_FFT)
    q = tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_FFT)
    assert p.n == 924 and p.n % 12 == 0
    assert {f: v for f, v in p.as_dict().items() if f != "n"} == {f: v for f, v in q.as_dict().items() if f != "n"}
    L = tfhe_amd.lib()
    for g in GS:
        assert L.tfhe_hip_mb_bsk_len(ctypes.byref(p), g) == (924 // g) * ((1 << g) - 1) * 4 * N
    assert L.tfhe_hip_mb_bsk_len(ctypes.byref(toy_params(12)), 4) == 3 * 15 * 4 * N
    for g in (0, 1, 5, 8):
        assert L.tfhe_hip_mb_bsk_len(ctypes.byref(p), g) == 0
    assert L.tfhe_hip_mb_bsk_len(ctypes.byref(q), 4) == 0          # 918 % 4 != 0
    assert L.tfhe_hip_mb_bsk_len(ctypes.byref(q), 2) == 459 * 3 * 4 * N
    assert L.tfhe_hip_mb_bsk_len(None, 2) == 0
    assert L.tfhe_hip_grouping(None) == 1


def test_refusals_without_a_device():
    ck, _ = tfhe_amd.gen_keys(toy_params(), KEY_SEED, with_server_key=False)
    for g in (0, 1, 5):
        with pytest.raises(tfhe_amd.TfheError) as e:
            tfhe_amd.server_keygen(ck, KEY_SEED, grouping=g) if g != 1 else tfhe_amd._mb_server_key(
                ck.params, tfhe_amd.rng_key(KEY_SEED), ck.lwe_key, ck.glwe_key, 1)
        assert e.value.code == -1 and "grouping factor" in str(e.value)
    ck10, _ = tfhe_amd.gen_keys(toy_params(10), KEY_SEED, with_server_key=False)
    for g in (3, 4):
        with pytest.raises(tfhe_amd.TfheError) as e:
            tfhe_amd.server_keygen(ck10, KEY_SEED, grouping=g)
        assert e.value.code == -1 and "not divisible" in str(e.value)
    # out of scope: the NTT transform, N = 1024
    for preset in (tfhe_amd.PRESET_FHEVM, tfhe_amd.PRESET_GATE_FFT):
        p = tfhe_amd.Params.preset(preset)
        p.n = 12
        ckx, _ = tfhe_amd.gen_keys(p, KEY_SEED, with_server_key=False)
        with pytest.raises(tfhe_amd.TfheError) as e:
            tfhe_amd.server_keygen(ckx, KEY_SEED, grouping=2)
        assert e.value.code == -5
    L = tfhe_amd.lib()
    one = np.zeros(1, dtype=np.uint64)
    assert L.tfhe_hip_load_keys_mb(None, 2, tfhe_amd._u64(one), 1, None, 0) == -1
    assert b"load_keys_mb" in L.tfhe_hip_last_error()


def test_secret_keys_and_ksk_equal_the_classic_keygen(toy_keys):
    ck0, sk0 = tfhe_amd.gen_keys(toy_params(), KEY_SEED)
    for g in GS:
        ck, sk = toy_keys[g]
        assert sk.grouping == g and sk.ms_zeros is None
        assert np.array_equal(ck.lwe_key, ck0.lwe_key) and np.array_equal(ck.glwe_key, ck0.glwe_key)
        assert np.array_equal(sk.ksk, sk0.ksk)
        assert sk.bsk.size == (12 // g) * ((1 << g) - 1) * 4 * N
        # server_keygen for given secret keys, and the seeded C entry point, give the same words
        sk2 = tfhe_amd.server_keygen(ck, KEY_SEED, grouping=g)
        assert np.array_equal(sk2.bsk, sk.bsk) and np.array_equal(sk2.ksk, sk.ksk)
        b3 = np.zeros_like(sk.bsk)
        rc = tfhe_amd.lib().tfhe_hip_mb_server_keygen(ctypes.byref(ck.params), g, KEY_SEED, tfhe_amd._u64(ck.lwe_key),
                                                      tfhe_amd._u64(ck.glwe_key), tfhe_amd._u64(b3), None)
        assert rc == 0 and np.array_equal(b3, sk.bsk)
    # no GGSW repeats a classic row or another grouping's: the streams are the key's own
    firsts = [toy_keys[g][1].bsk[:N] for g in GS] + [sk0.bsk[:N]]
    assert all(not np.array_equal(firsts[0], f) for f in firsts[3:])


@pytest.mark.parametrize("g", GS)
def test_every_ggsw_decrypts_to_its_indicator(oracle_mod, toy_keys, g):
    ck, sk = toy_keys[g]
    key = mb.key_view(sk.bsk, g, 12)
    gad = 1 << 41
    S = ck.glwe_key.astype(np.int64)
    seen = 0
    for q in range(12 // g):
        bits = sum(int(ck.lwe_key[g * q + i]) << i for i in range(g))
        for s in range(1, 1 << g):
            ind = int(s == bits)
            seen += ind
            body = _phase(oracle_mod, ck, key[q, s - 1, 1].reshape(-1)).view(np.int64)
            want = np.zeros(N, dtype=np.int64)
            want[0] = ind * gad
            assert np.abs(body - want).max() < 1 << 30, (q, s)      # noise 2^17 sd against the gadget 2^41
            mask = _phase(oracle_mod, ck, key[q, s - 1, 0].reshape(-1)).view(np.int64)
            assert np.abs(mask + ind * gad * S).max() < 1 << 30, (q, s)
    assert seen == sum(1 for q in range(12 // g) if ck.lwe_key[g * q:g * q + g].any())


def _toy_cts(ck, msgs, seed):
    """small-key encryptions (the blind rotation's input at a KS -> PBS set)"""
    m = np.asarray(msgs, dtype=np.uint64) * np.uint64(DELTA)
    out = np.zeros((m.size, ck.params.n + 1), dtype=np.uint64)
    rc = tfhe_amd.lib().tfhe_hip_lwe_encrypt(ck.params.n, tfhe_amd._u64(ck.lwe_key), ck.params.lwe_noise_log2, seed, 0,
                                             tfhe_amd._u64(m), m.size, tfhe_amd._u64(out))
    assert rc == 0
    return out


@pytest.mark.parametrize("g", GS)
def test_reference_rotation_decrypts_the_lut_for_all_messages(oracle_mod, toy_keys, g):
    ck, sk = toy_keys[g]
    lut = tfhe_amd.lut_from_table(N, 16, TABLE, DELTA)
    cts = _toy_cts(ck, np.arange(16), seed=0xB170 + g)
    for m, ct in enumerate(cts):
        trace, s1 = mb.blind_rotate_trace(oracle_mod, sk.bsk, g, ct, lut)
        assert trace.shape == (12 // g + 1, 2 * N) and s1.shape == (12 // g, 2)
        ph = int(_phase(oracle_mod, ck, trace[-1])[0])
        assert ((ph + DELTA // 2) // DELTA) % 16 == TABLE[m], (g, m)


def test_sum_then_switch_on_a_crafted_pair():
    """a_0, a_1 each just below a rounding tie: each rounds down, their sum rounds past the next step."""
    step = 1 << 52                                 # 2^64 / 4096
    a0 = 5 * step + step // 2 - 1
    a1 = 9 * step + step // 2 - 1
    t = mb.subset_switch(np.array([a0, a1], dtype=np.uint64))
    assert list(t) == [5, 9, 15]                  # sigma = 1, 2, 3
    assert int(mb.ms(np.uint64(a0)) + mb.ms(np.uint64(a1))) == 14 != int(t[2])
    # wrap of the sum mod 2^64 and of the switched value mod 2N
    t = mb.subset_switch(np.array([(1 << 64) - 1, (1 << 63)], dtype=np.uint64))
    assert list(t) == [0, 2048, 2048]
    t = mb.subset_switch(np.array([4095 * step, step, 2 * step], dtype=np.uint64))
    assert list(t) == [4095, 1, 0, 2, 1, 3, 2]


@pytest.mark.parametrize("tv", [0, 2048, 4095])
def test_group_step_rotates_by_the_live_subset(oracle_mod, toy_keys, tv):
    """One exact group step on a trivial accumulator is X^{t_sigma*} acc for sigma* = the group's key bits, at the
    edge values of t: 0 (identity), 2048 (negation), 4095 (X^-1)."""
    g = 2
    ck, sk = toy_keys[g]
    key = mb.key_view(sk.bsk, g, 12)
    q = next(q for q in range(6) if ck.lwe_key[2 * q:2 * q + 2].any())
    bits = int(ck.lwe_key[2 * q]) + 2 * int(ck.lwe_key[2 * q + 1])
    t = np.array([7, 11, 13])
    t[bits - 1] = tv
    acc = np.zeros((2, N), dtype=np.uint64)
    acc[1] = (np.arange(N, dtype=np.uint64) % np.uint64(16)) * np.uint64(DELTA)
    out, s1 = mb.group_step(oracle_mod, key[q], t, acc)
    want = mb.rotate(acc[1], tv)
    got = _phase(oracle_mod, ck, out.reshape(-1))
    assert np.abs((got - want).view(np.int64)).max() < DELTA // 2 ** 6
    assert np.all(s1 > 0)
    ident, s0 = mb.group_step(oracle_mod, key[q], np.zeros(3, dtype=np.int64), acc)
    assert np.array_equal(ident, acc) and np.all(s0 == 0)


def test_exponent_table_is_the_transform_of_x(oracle_mod):
    """e[p] against the definition: the oracle's fft1k forward transform of X^1 is zeta^{e[p]} at every point."""
    x1 = np.zeros(N)
    x1[1] = 1.0
    z = oracle_mod.fft_fwd(x1)[0]
    e = mb.exponents()
    w = np.array([oracle_mod.fft_twiddle(int(v), 4096) for v in e])
    assert np.abs(z - (w[:, 0] + 1j * w[:, 1])).max() < 64 * 2.0 ** -53
    assert oracle_mod.fft_twiddle(0, 4096) == (1.0, 0.0)
