"""The multi-bit blind rotation on the device (tfhe_amd/csrc/pbs_fft2k_mb.hip) against the exact reference
(tests/multibit_ref.py), at toy n unless a test names the preset.

Teacher forcing as tests/test_gpu_exact.py does per element, here per group: a ciphertext whose masks are zeroed from
group m on runs m live group steps and then exact identities (every t_sigma = 0), so the device's accumulator for m + 1
is its group step m applied to its accumulator for m, and the exact step of the latter is the arbiter.

Recorded on one MI355X (DESIGN §4o has the table): max error / bound 2^-15.5 (g = 2), 2^-16.3 (g = 3), 2^-17.2
(g = 4) at toy n and 2^-17.3 over the 462 steps of two full rotations at preset 4, rms error 0.6 .. 1.3 x u S1 / sqrt(N);
output phase noise of 1024 PBS at preset 4, g = 4: rms 2^50.82 against the classic kernel's 2^49.56 at the same n
(ratio 2.40), decision half-interval 144.6 sigma (classic 346.2).
"""
import math

import numpy as np
import pytest

from conftest import KEY_SEED
import multibit_ref as mb
from test_multibit import DELTA, N, TABLE, toy_params, _toy_cts

import tfhe_amd
from tfhe_amd import radix as R

pytestmark = pytest.mark.gpu

KERNEL = "blind_rotate_fft2k_mb_kernel"
STEP = 1 << 52            # 2^64 / 2N: one step of the modulus switch
HALF = 1 << 51            # its rounding boundary


class Env:
    def __init__(self, g, n):
        self.g, self.n = g, n
        self.ck, self.sk = tfhe_amd.gen_keys(toy_params(n), KEY_SEED, grouping=g)
        self.eng = tfhe_amd.Engine(self.ck.params, 0)
        self.eng.load_keys(self.sk)
        self.lut = tfhe_amd.lut_from_table(N, 16, TABLE, DELTA)


@pytest.fixture(scope="module")
def envs():
    cache = {}

    def get(g, n=12):
        if (g, n) not in cache:
            cache[g, n] = Env(g, n)
        return cache[g, n]

    yield get
    for e in cache.values():
        e.eng.close()


def _truncated(cts: np.ndarray, m: int, g: int) -> np.ndarray:
    """copies with the masks of groups >= m set to 0 (body kept)"""
    out = cts.copy()
    out[:, g * m:-1] = 0
    return out


def _crafted(env, count=5):
    """count ciphertexts with crafted masks: ct 0 subset sums exactly on the rounding tie, the same group twice in a
    row; ct 1 t_sigma = 0 inside a live group (a zero mask, and a pair summing to 0) and t_sigma = 2048; ct 2 sums
    one below the tie and t_sigma > 2048; ct 3 an all-zero group before a live one; ct 4 random."""
    g, n = env.g, env.n
    rng = np.random.default_rng(0xB17 + 16 * g + n)
    cts = _toy_cts(env.ck, rng.integers(0, 16, count), seed=0xB1A0 + g)
    u = np.uint64
    t = rng.integers(1, 4096, g).astype(np.uint64)
    cts[0, :g] = t * u(STEP)
    cts[0, 0] = (u(2) * t[0] + u(1)) * u(HALF)
    cts[1, 0] = 0
    cts[1, 1] = u(1 << 63)
    if g > 2:
        cts[1, 2] = u(1 << 63)                      # a_1 + a_2 = 0 mod 2^64
    cts[2, :g] = t * u(STEP)
    cts[2, 0] = (u(2) * t[0] + u(1)) * u(HALF) - u(1)
    cts[2, 1] = u(3000 * STEP)
    if n >= 2 * g:
        cts[0, g:2 * g] = cts[0, :g]
        cts[3, g:2 * g] = 0
    return cts


def _teacher_forced(env, oracle_mod, cts):
    """one launch of exactly len(cts) ciphertexts per truncation point; every group step against the exact one"""
    g, n = env.g, env.n
    groups = n // g
    dev = np.stack([env.eng.blind_rotate(_truncated(cts, m, g), env.lut) for m in range(groups + 1)])
    key = mb.key_view(env.sk.bsk, g, n)
    exact, s1 = [], []
    for m in range(groups):
        for b in range(len(cts)):
            e, s = mb.group_step(oracle_mod, key[m], mb.subset_switch(cts[b, g * m:g * m + g]), dev[m, b])
            exact.append(e.reshape(-1))
            s1.append(s)
    for b in range(len(cts)):
        assert np.array_equal(dev[0, b], mb.initial_acc(cts[b], env.lut).reshape(-1))
    return dev, mb.check_steps(g, dev[1:].reshape(-1, 2 * N), np.array(exact), np.array(s1)), np.array(s1)


@pytest.mark.parametrize("B", [1, 2, 3, 5])
@pytest.mark.parametrize("g", [2, 3, 4])
def test_every_group_step_within_the_bound(envs, oracle_mod, g, B):
    env = envs(g)
    assert env.eng.grouping == g and env.eng.br_kernel(B) == KERNEL
    cts = _crafted(env)[:B]
    dev, st, s1 = _teacher_forced(env, oracle_mod, cts)
    assert st["steps"] == (12 // g) * B - (1 if B >= 4 else 0)
    if B >= 4:
        assert np.all(s1.reshape(12 // g, B, 2)[1, 3] == 0)           # the all-zero group was an exact identity
    t0 = mb.subset_switch(cts[0, :g])
    assert t0[0] == (int(cts[0, 0]) + HALF) // STEP % 4096            # the tie rounds up
    if B >= 3:
        t1, t2 = mb.subset_switch(cts[1, :g]), mb.subset_switch(cts[2, :g])
        assert t1[0] == 0 and t1[1] == 2048 and (t1 != 0).any() and (t2 > 2048).any()
        assert t2[0] == (t0[0] - 1) % 4096


@pytest.mark.parametrize("g", [2, 3, 4])
def test_one_group(envs, oracle_mod, g):
    """n = g: a single group step is the whole rotation"""
    env = envs(g, g)
    dev, st, _ = _teacher_forced(env, oracle_mod, _crafted(env, 3))
    assert dev.shape[0] == 2 and st["steps"] == 3


@pytest.mark.parametrize("g", [2, 3, 4])
def test_batch_independence_determinism_and_output_modes(envs, oracle_mod, g):
    env = envs(g)
    eng, ck = env.eng, env.ck
    tables = [TABLE, [(5 * v + 2) % 16 for v in range(16)], [(15 - v) % 16 for v in range(16)]]
    luts = np.stack([tfhe_amd.lut_from_table(N, 16, t, DELTA) for t in tables])
    msgs = np.array([3, 0, 15, 8, 6])
    idx = np.array([2, 0, 1, 1, 2], dtype=np.uint32)
    cts = _toy_cts(ck, msgs, seed=0xB1B0 + g)
    acc = eng.blind_rotate(cts, luts, idx)
    assert np.array_equal(eng.blind_rotate(cts, luts, idx), acc)                      # two runs
    for b in range(5):
        alone = eng.blind_rotate(cts[b:b + 1], luts, idx[b:b + 1])
        assert np.array_equal(alone[0], acc[b]), b
    perm = np.array([4, 2, 0, 3, 1])
    assert np.array_equal(eng.blind_rotate(cts[perm], luts, idx[perm]), acc[perm])    # any position
    big = eng.bootstrap(cts, luts, idx)                                               # the other output mode
    assert np.array_equal(eng.sample_extract(acc), big)
    got = ck.decrypt(big, 16)
    assert list(got) == [tables[int(i)][int(m)] for m, i in zip(msgs, idx)]


# ---- upper layers on multi-bit keys, toy n ------------------------------------------------------------------------
def test_pbs_many_two_functions(envs):
    env = envs(4)
    t0, t1 = [(3 * v + 1) % 8 for v in range(8)], [(7 - v) % 8 for v in range(8)]
    lut, stride = tfhe_amd.lut_many(N, 16, [t0, t1], DELTA)
    msgs = np.arange(8)
    out = env.eng.pbs_many(env.ck.encrypt(msgs, 16, seed=0xB1C0), lut[None], 2, stride).reshape(8, 2, -1)
    assert list(env.ck.decrypt(out[:, 0], 16)) == t0 and list(env.ck.decrypt(out[:, 1], 16)) == t1


def test_bootstrap_with_a_null_ksk(envs):
    env = envs(3)
    sk = tfhe_amd.ServerKey(env.ck.params, env.sk.bsk, None, None, grouping=3)
    msgs = np.array([1, 7, 12])
    cts = _toy_cts(env.ck, msgs, seed=0xB1D0)
    with tfhe_amd.Engine(env.ck.params, 0) as eng:
        eng.load_keys(sk)
        assert eng.grouping == 3
        big = eng.bootstrap(cts, env.lut)
        assert np.array_equal(big, env.eng.bootstrap(cts, env.lut))
        assert list(env.ck.decrypt(big, 16)) == [TABLE[m] for m in msgs]
        with pytest.raises(tfhe_amd.TfheError) as e:
            eng.pbs(env.ck.encrypt(msgs, 16, seed=1), env.lut)
        assert e.value.code == -4                                                     # rotation-only: ENOKEYS


def test_device_resident_radix_add_and_lt(envs):
    env = envs(4)
    c = R.RadixCircuit(env.eng, device="cuda:0")
    a = np.array([200, 17, 255], dtype=np.uint64)
    b = np.array([100, 17, 1], dtype=np.uint64)
    A = R.RadixUint.encrypt(c, env.ck, a, 8, seed=0xB1E0, stream0=0)
    Bv = R.RadixUint.encrypt(c, env.ck, b, 8, seed=0xB1E0, stream0=12)
    add, lt = c.run_many([R.fhevm_op(c, "add", A, Bv), R.fhevm_op(c, "lt", A, Bv)])
    np.testing.assert_array_equal(add.decrypt(env.ck), (a + b) & np.uint64(255))
    np.testing.assert_array_equal(env.ck.decrypt(np.asarray(lt), R.SPACE).astype(bool), a < b)


def test_two_shards(envs):
    env = envs(2)
    msgs = np.arange(7) * 2
    cts = env.ck.encrypt(msgs, 16, seed=0xB1F0)
    with tfhe_amd.Engine(env.ck.params, [0, 0]) as eng:
        eng.load_keys(env.sk)
        assert eng.grouping == 2 and eng.br_kernel(4) == KERNEL
        out = eng.pbs(cts, env.lut)
    assert np.array_equal(out, env.eng.pbs(cts, env.lut))
    assert list(env.ck.decrypt(out, 16)) == [TABLE[m] for m in msgs]


def test_classic_keys_after_multibit_keys(envs, oracle_mod):
    env = envs(4)
    prm = oracle_mod.params(3)
    prm.n = 12
    okeys = oracle_mod.Keys(prm, KEY_SEED)
    ck, sk = tfhe_amd.gen_keys(toy_params(), KEY_SEED)
    assert np.array_equal(sk.bsk, okeys.bsk)
    cts = ck.encrypt(np.arange(6), 16, seed=0xB200)
    with tfhe_amd.Engine(ck.params, 0) as eng:
        eng.load_keys(env.sk)
        assert eng.br_kernel(6) == KERNEL
        mbout = eng.pbs(cts, env.lut)
        eng.load_keys(sk)
        assert eng.grouping == 1 and eng.br_kernel(6) == "blind_rotate_fft2k_kernel"
        out = eng.pbs(cts, env.lut)
        assert np.array_equal(out, oracle_mod.pbs_batch_fft(prm, okeys, cts, env.lut[None]))
        eng.load_keys(env.sk)                                                         # and back
        assert eng.grouping == 4 and np.array_equal(eng.pbs(cts, env.lut), mbout)
    assert list(ck.decrypt(mbout, 16)) == [TABLE[m] for m in range(6)]


# ---- contract -----------------------------------------------------------------------------------------------------
def test_refusals(envs):
    env = envs(4)
    L = tfhe_amd.lib()
    zeros = tfhe_amd.ms_zeros_keygen(env.ck.params, KEY_SEED, env.ck.lwe_key, 4)
    with pytest.raises(tfhe_amd.TfheError) as e:
        env.eng.load_ms_key(zeros)
    assert e.value.code == -5 and "multi-bit" in str(e.value)
    with pytest.raises(tfhe_amd.TfheError) as e:
        env.eng.ms_reduce(_toy_cts(env.ck, [1], seed=3))
    assert e.value.code == -5 and "multi-bit" in str(e.value)
    ksk = env.sk.ksk
    with tfhe_amd.Engine(env.ck.params, 0) as eng:
        short = env.sk.bsk[:-N]
        rc = L.tfhe_hip_load_keys_mb(eng._h, 4, tfhe_amd._u64(short), short.size, tfhe_amd._u64(ksk), ksk.size)
        assert rc == -1 and b"sizes" in L.tfhe_hip_last_error()
        rc = L.tfhe_hip_load_keys_mb(eng._h, 3, tfhe_amd._u64(env.sk.bsk), env.sk.bsk.size, tfhe_amd._u64(ksk), ksk.size)
        assert rc == -1 and b"sizes" in L.tfhe_hip_last_error()                       # a g = 4 key loaded as g = 3
        rc = L.tfhe_hip_load_keys_mb(eng._h, 5, tfhe_amd._u64(env.sk.bsk), env.sk.bsk.size, tfhe_amd._u64(ksk), ksk.size)
        assert rc == -1 and b"grouping factor" in L.tfhe_hip_last_error()
        assert eng.grouping == 1
        with pytest.raises(tfhe_amd.TfheError) as e:
            eng.blind_rotate(_toy_cts(env.ck, [1], seed=3), env.lut)
        assert e.value.code == -4                                                     # nothing was loaded
    with tfhe_amd.Engine(toy_params(10), 0) as eng:
        rc = L.tfhe_hip_load_keys_mb(eng._h, 4, tfhe_amd._u64(env.sk.bsk), env.sk.bsk.size, None, 0)
        assert rc == -1 and b"not divisible" in L.tfhe_hip_last_error()
    for preset in (tfhe_amd.PRESET_FHEVM, tfhe_amd.PRESET_GATE_FFT):                  # an NTT ctx, an N = 1024 ctx
        p = tfhe_amd.Params.preset(preset)
        p.n = 12
        with tfhe_amd.Engine(p, 0) as eng:
            rc = L.tfhe_hip_load_keys_mb(eng._h, 4, tfhe_amd._u64(env.sk.bsk), env.sk.bsk.size, None, 0)
            assert rc == -5 and b"multi-bit" in L.tfhe_hip_last_error()


# ---- preset 4, g = 4 ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def preset4():
    p = tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_MB_FFT)
    ck, sk = tfhe_amd.gen_keys(p, KEY_SEED, grouping=4)
    eng = tfhe_amd.Engine(p, 0)
    eng.load_keys(sk)
    yield ck, sk, eng, tfhe_amd.lut_from_table(N, 16, TABLE, DELTA)
    eng.close()


def test_preset4_64_pbs_decrypt(preset4):
    ck, sk, eng, lut = preset4
    msgs = np.arange(64) % 16
    out = eng.pbs(ck.encrypt(msgs, 16, seed=0xB210), lut)
    assert eng.br_kernel(64) == KERNEL
    assert list(ck.decrypt(out, 16)) == [TABLE[m] for m in msgs]


def test_preset4_full_rotation_teacher_forced(preset4, oracle_mod):
    ck, sk, eng, lut = preset4
    n, g = 924, 4
    groups = n // g
    cts = _toy_cts(ck, [5, 10], seed=0xB220)
    batch = np.concatenate([np.stack([_truncated(c[None], m, g)[0] for m in range(groups + 1)]) for c in cts])
    dev = eng.blind_rotate(batch, lut).reshape(2, groups + 1, 2 * N)
    assert np.array_equal(eng.blind_rotate(cts, lut), dev[:, -1])
    key = mb.key_view(sk.bsk, g, n)
    exact, s1 = [], []
    for b in range(2):
        for m in range(groups):
            e, s = mb.group_step(oracle_mod, key[m], mb.subset_switch(cts[b, g * m:g * m + g]), dev[b, m])
            exact.append(e.reshape(-1))
            s1.append(s)
    st = mb.check_steps(g, dev[:, 1:].reshape(-1, 2 * N), np.array(exact), np.array(s1))
    assert st["steps"] == 2 * groups
    # the exact reference's own full rotation, not teacher-forced, decrypts the same message
    trace, _ = mb.blind_rotate_trace(oracle_mod, sk.bsk, g, cts[0], lut)
    ph = oracle_mod.glwe_phase_native(1, N, ck.glwe_key, trace[-1])
    assert ((int(ph[0]) + DELTA // 2) // DELTA) % 16 == TABLE[5]


def test_preset4_noise_against_the_classic_kernel(preset4):
    """Output phase error of 1024 PBS, multi-bit g = 4 against classic keys of the same secret keys at n = 924 (no
    modulus-switch noise reduction on either side).  Recorded, not asserted: the ratio and the decision
    half-interval in sigma; asserted: nothing mis-decodes."""
    ck, sk, eng, lut = preset4
    msgs = np.arange(1024) % 16
    cts = ck.encrypt(msgs, 16, seed=0xB230)
    want = np.array([TABLE[m] for m in msgs], dtype=np.uint64)

    def phase_err(e):
        out = e.pbs(cts, lut)
        assert np.array_equal(ck.decrypt(out, 16), want)
        return (ck.phase(out) - want * np.uint64(DELTA)).view(np.int64).astype(np.float64)

    err_mb = phase_err(eng)
    skc = tfhe_amd.server_keygen(ck, KEY_SEED)
    skc.ms_zeros = None
    with tfhe_amd.Engine(ck.params, 0) as ec:
        ec.load_keys(skc)
        assert ec.br_kernel(1024) == "blind_rotate_fft2k_kernel"
        err_c = phase_err(ec)
    rms_mb, rms_c = math.sqrt((err_mb ** 2).mean()), math.sqrt((err_c ** 2).mean())
    print(f"preset 4, g = 4: output phase noise rms 2^{math.log2(rms_mb):.2f} (classic 2^{math.log2(rms_c):.2f}, "
          f"ratio {rms_mb / rms_c:.3f}), decision half-interval {DELTA / 2 / rms_mb:.1f} sigma "
          f"(classic {DELTA / 2 / rms_c:.1f}), max |err| 2^{math.log2(np.abs(err_mb).max()):.2f}")
