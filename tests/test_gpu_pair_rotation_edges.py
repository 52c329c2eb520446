"""Rotation and digit edge cases of the FFT64 blind rotation (pbs_fft.hip rotate_states, decomp_top), bit-exact
against oracle/fft_oracle.c on the component-pair batch kernel and on the latency kernel.

The mask words are a << 53, so the modulus switch returns a exactly, and a cycles through every slot shift
A = (a >> 6) & 15, the lane shifts r = a & 63 in {0, 1, 63} (no lane, one lane, all but one lane wrap in slot 15) and
both signs (a >= 1024).  The LUT holds full-width words, so the low words of the 64-bit differences and their borrows
are live from the first CMUX.  One row has every mask word 0: no rotation, all-zero digits in every level (the
signed-zero path of the top-level digit).  B = 3 leaves a padding pair in the batch kernel's last workgroup.
"""
import numpy as np
import pytest

from conftest import KEY_SEED

import tfhe_amd

pytestmark = pytest.mark.gpu
N, n = 1024, 630
GOLDILOCKS = (1 << 64) - (1 << 32) + 1


def _rotations():
    a = [0, 1, 63, 64, 65, 960, 1023, 1024, 1025, 1087, 2047]
    for A in range(16):
        for s in (0, 1024):
            a += [s + 64 * A + r for r in (0, 1, 63)]
    return np.array(a, dtype=np.uint64)


@pytest.fixture(scope="module")
def case(oracle_mod):
    """Engine, inputs and the oracle's accumulators (computed once, shared by both kernels' tests)."""
    params = tfhe_amd.Params.preset(tfhe_amd.PRESET_GATE_FFT)
    assert (params.n, params.N) == (n, N)
    _, sk = tfhe_amd.gen_keys(params, KEY_SEED)
    prm = oracle_mod.params(2)
    okeys = oracle_mod.Keys(prm, KEY_SEED)
    rng = np.random.default_rng(0x207A)
    rot = _rotations()
    assert {int(v) >> 6 & 15 for v in rot} == set(range(16)) and {int(v) & 63 for v in rot} == {0, 1, 63}
    assert all(64 * A + 63 in rot for A in range(16)) and rot.min() == 0 and rot.max() == 2047
    cts = np.zeros((3, n + 1), dtype=np.uint64)
    cts[0, :n] = np.resize(rot, n) << np.uint64(53)
    cts[1, :n] = np.resize(np.roll(rot[::-1], 7), n) << np.uint64(53)
    cts[:, n] = rng.integers(0, 2**64, 3, dtype=np.uint64)  # row 2: every mask word 0
    lut = rng.integers(0, GOLDILOCKS, N, dtype=np.uint64)
    ref = np.stack([oracle_mod.blind_rotate_fft(prm, okeys, cts[i], lut) for i in range(3)])
    ref.setflags(write=False)
    eng = tfhe_amd.Engine(params, 0)
    eng.load_keys(sk)
    yield eng, cts, lut, ref
    eng.close()


@pytest.mark.parametrize("latency_batch, kernel", [(0, "pair"), (1 << 20, "latency")])
def test_rotation_edges_bitexact(case, latency_batch, kernel):
    eng, cts, lut, ref = case
    try:
        eng.set_latency_batch(latency_batch)
        acc = eng.blind_rotate(cts, lut)
    finally:
        eng.set_latency_batch(256)  # the P-GATE FFT64 default
    for i in range(3):
        assert np.array_equal(acc[i], ref[i]), f"{kernel} kernel: accumulator {i} differs from the oracle"
