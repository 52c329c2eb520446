"""The transposes of the P-GATE pair kernel fed from the DFT8's last stage (fft512.h: dft8_xpose_p): each of
a transpose's eight stores is issued as soon as its slot's output is final -- slots 0, 4, 2, 6, then 1, 5, 3, 7 -- with
the rest of the DFT8 between them.  Placement only, so both accumulator components and the extracted LWE stay bit-equal
to oracle/fft_oracle.c.  What can go wrong is a store sent to the wrong slot (4 for 2, 5 for 3), one emitted before its
value is final, a twiddle multiply lost (slot 0 has one in the forward's first transpose and none in its second), or a
read moved in front of the stores.  The cases, on the rotation-only engine of test_gpu_pair_seam.py:
  (n, B) = (1, 1), (2, 3), (3, 2), random masks: one CMUX; a padding pair with three workgroups; all four waves live
  n = 1, B = 2, impulse accumulators: the LUT zeroed outside coefficient j, the rows rotating by r = 1 and, with the
           sign bit, r = 63.  The digit polynomials have one or two non-zero coefficients, so every DFT8 input has a
           single live slot and every output slot carries another twiddle: no swap or skipped multiply can cancel
  n = 2, a row whose masks all rotate by 0: every digit is zero, the top level's -0.0
and two LUTs chosen by lut_index through Engine.pbs with the preset's full keys at B = 2."""
import functools

import numpy as np
import pytest

from conftest import KEY_SEED

import tfhe_amd
import test_decompress as T
from test_gpu_decompress import rotation_inputs
from test_gpu_pair_seam import ms2048

pytestmark = pytest.mark.gpu
PRESET = 2  # P-GATE FFT64
PAIR = "blind_rotate_fft_pair_kernel"
CASES = [(1, 1), (2, 3), (3, 2)]
IMPULSES = [0, 1, 63, 64, 511, 512, 960, 1023]
AMOUNT_R1, AMOUNT_R63_NEG = 1, 1024 + 63


@functools.lru_cache(maxsize=None)
def context(n):
    """(oracle module, oracle parameters at n, rotation-only keys, the seam test's LUT): built once per n."""
    O = T.oracle()
    prm = O.params(PRESET)
    dprm = T.with_n(prm, n)
    glwe_key = O.Keys(prm, T.SEED, with_bsk=False, with_ksk=False).glwe_key
    lwe_key = np.random.default_rng(n).integers(0, 2, n).astype(np.uint64)
    keys = T.rotation_keys(O, dprm, T.DK_SEED, lwe_key, glwe_key)
    lut = O.lut_from_table(prm.N, 16, [(7 * m + 2) % 16 for m in range(16)], 1 << 59)
    return O, dprm, keys, lut


def check(n, cts, lut):
    """Both components of blind_rotate and the bootstrap's LWE, word for word against the oracle."""
    O, dprm, keys, _ = context(n)
    B, N = cts.shape[0], dprm.N
    ref = [T.bootstrap_ref(O, dprm, keys, cts[q], lut) for q in range(B)]
    ref_acc, ref_out = np.stack([r[0] for r in ref]).reshape(B, -1), np.stack([r[1] for r in ref])
    with tfhe_amd.Engine(T.with_n(tfhe_amd.Params.preset(PRESET), n), 0) as eng:
        eng.load_bsk(keys.bsk)
        eng.set_latency_batch(0)
        assert eng.br_kernel(B) == PAIR
        acc = eng.blind_rotate(cts, lut)
        assert acc.shape == ref_acc.shape
        for comp in (0, 1):
            got, want = acc[:, comp * N:(comp + 1) * N], ref_acc[:, comp * N:(comp + 1) * N]
            assert np.array_equal(got, want), \
                f"blind_rotate component {comp}: rows {np.nonzero((got != want).any(1))[0]}, " \
                f"{int((got != want).sum())} words differ"
        out = eng.bootstrap(cts, lut)
        assert np.array_equal(out, ref_out), f"bootstrap: rows {np.nonzero((out != ref_out).any(1))[0]}"
    return ref_acc


@pytest.mark.parametrize("n,B", CASES, ids=lambda v: str(v))
def test_pair_dft8_stores_random_masks(n, B):
    lut = context(n)[3]
    cts = rotation_inputs(lut.size, n, B, 311 + n)
    cts[:, :n] = np.random.default_rng(3110 + n).integers(0, 2 ** 64, (B, n), dtype=np.uint64)
    check(n, cts, lut)


@pytest.mark.parametrize("j", IMPULSES)
def test_pair_dft8_stores_impulse(j):
    n, B = 1, 2
    lut = context(n)[3].copy()
    assert lut[j] != 0
    keep = lut[j]
    lut[:] = 0
    lut[j] = keep
    cts = rotation_inputs(lut.size, n, B, 313)
    cts[0, 0] = np.uint64(AMOUNT_R1) << np.uint64(53)
    cts[1, 0] = np.uint64(AMOUNT_R63_NEG) << np.uint64(53)
    assert ms2048(cts[:, 0]).tolist() == [AMOUNT_R1, AMOUNT_R63_NEG]
    ref_acc = check(n, cts, lut)
    assert ref_acc.any(axis=1).all()  # the impulse went through the CMUX of either row


def test_pair_dft8_stores_all_zero_digits():
    """Row 0 rotates by 0 at every CMUX: X^0 acc - acc = 0, so every transform of that ciphertext runs on zeros (the top
    digits are -0.0) and its accumulator must come back as it went in; row 1 keeps random masks."""
    n, B = 2, 2
    lut = context(n)[3]
    cts = rotation_inputs(lut.size, n, B, 317)
    cts[0, :n] = 0
    cts[1, :n] = np.random.default_rng(3170).integers(0, 2 ** 64, n, dtype=np.uint64)
    assert not ms2048(cts[0, :n]).any() and ms2048(cts[1, :n]).all()
    check(n, cts, lut)


def test_pair_dft8_stores_two_luts_full_keys(oracle_mod, gate_fft_keys):
    """Preset n, full keys, B = 2 (one workgroup, all four waves live) through Engine.pbs: two LUTs by lut_index and two
    messages, so both components of both ciphertexts differ."""
    O = oracle_mod
    prm = O.params(PRESET)
    okeys = O.Keys(prm, KEY_SEED)
    ck, sk = gate_fft_keys
    msgs = np.array([6, 1], dtype=np.uint64) * np.uint64((1 << 63) // 8)
    cts = ck.encrypt_torus(msgs, seed=0xC0FFEE11)
    luts = np.stack([O.lut_from_table(prm.N, 8, [(m * 3 + 1) % 8 for m in range(8)], (1 << 63) // 8),
                     O.lut_from_table(prm.N, 8, [(m * 5 + 2) % 8 for m in range(8)], (1 << 63) // 8)])
    idx = np.array([1, 0], dtype=np.uint32)
    ref = O.pbs_batch_fft(prm, okeys, cts, luts, idx)
    assert not np.array_equal(ref[0], ref[1])
    with tfhe_amd.Engine(ck.params, 0) as eng:
        eng.load_keys(sk)
        eng.set_latency_batch(0)
        assert eng.br_kernel(2) == PAIR
        out = eng.pbs(cts, luts, idx)
    assert np.array_equal(out, ref), f"pbs: rows {np.nonzero((out != ref).any(1))[0]}"
