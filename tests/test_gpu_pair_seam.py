"""The seams of the P-GATE pair kernel's CMUX loop (pbs_fft.hip): the rotation image of CMUX i + 1 is stored
under the accumulator update of CMUX i (a prologue stores CMUX 0's; the last CMUX stores one that nobody reads, with the
amount of the body word), and the partial-sum exchange between the two component waves of a ciphertext (the forms of
tools/ab_patches/r10_own_publish.patch, which keep the sums by role and publish them under the last level step's MAC,
were checked with this file too).  All of it is placement, so both accumulator components and the extracted LWE stay
bit-equal to oracle/fft_oracle.c.  A swapped key row or a mis-routed publish shows in one component of
eng.blind_rotate; a stale or early image shows at the trip counts and amounts below:
  (n, B) = (1, 1): the prologue's image is the only one read; the seam store after the only CMUX takes the body word,
           which is given r = 63 and the sign bit
           (2, 2), (3, 5): a padding pair, an odd batch, three workgroups
           (4, 3)
           (16, 2): row 0 rotates by 0, 63, 64, 1023, 1024, 1087, 2047, 1, 1, 960, 1984, 0, 0, 65, 1025, 2046 -- r = 0
           and 63, A = 0 and 15, both signs, equal amounts twice in a row, a = 0 (an all-zero difference); row 1 keeps
           ordinary masks, so the two ciphertexts of the workgroup differ at every CMUX
on the rotation-only engine of test_gpu_pair_keystream.py, and two LUTs chosen by lut_index with different messages
through Engine.pbs with the preset's full keys at B = 2."""
import numpy as np
import pytest

from conftest import KEY_SEED

import tfhe_amd
import test_decompress as T
from test_gpu_decompress import rotation_inputs

pytestmark = pytest.mark.gpu
PRESET = 2  # P-GATE FFT64
PAIR = "blind_rotate_fft_pair_kernel"
CASES = [(1, 1), (2, 2), (3, 5), (4, 3), (16, 2)]
AMOUNTS16 = [0, 63, 64, 1023, 1024, 1087, 2047, 1, 1, 960, 1984, 0, 0, 65, 1025, 2046]
BODY_R63_NEG = 1024 + 64 * 5 + 63  # the body word's amount at (1, 1): sign bit, r = 63


def ms2048(x):
    return ((((np.asarray(x, dtype=np.uint64) >> np.uint64(52)) + np.uint64(1)) >> np.uint64(1)) & np.uint64(2047))


@pytest.mark.parametrize("n,B", CASES, ids=lambda v: str(v))
def test_pair_seam_trip_counts_and_amounts(oracle_mod, n, B):
    O = oracle_mod
    prm = O.params(PRESET)
    dprm = T.with_n(prm, n)
    glwe_key = O.Keys(prm, T.SEED, with_bsk=False, with_ksk=False).glwe_key
    lwe_key = np.random.default_rng(n).integers(0, 2, n).astype(np.uint64)
    keys = T.rotation_keys(O, dprm, T.DK_SEED, lwe_key, glwe_key)
    cts = rotation_inputs(prm.N, n, B, 277 + n)
    if (n, B) == (1, 1):
        cts[0, n] = np.uint64(BODY_R63_NEG) << np.uint64(53)
        assert int(ms2048(cts[0, n])) == BODY_R63_NEG
    if n == 16:
        cts[0, :n] = np.array(AMOUNTS16, dtype=np.uint64) << np.uint64(53)
        assert ms2048(cts[0, :n]).tolist() == AMOUNTS16
        cts[1, :n] = np.random.default_rng(1610).integers(0, 2 ** 64, n, dtype=np.uint64)
        assert (ms2048(cts[1, :n]) != ms2048(cts[0, :n])).all()
    lut = O.lut_from_table(prm.N, 16, [(7 * m + 2) % 16 for m in range(16)], 1 << 59)
    ref = [T.bootstrap_ref(O, dprm, keys, cts[q], lut) for q in range(B)]
    ref_acc, ref_out = np.stack([r[0] for r in ref]).reshape(B, -1), np.stack([r[1] for r in ref])
    params = T.with_n(tfhe_amd.Params.preset(PRESET), n)
    with tfhe_amd.Engine(params, 0) as eng:
        eng.load_bsk(keys.bsk)
        eng.set_latency_batch(0)
        assert eng.br_kernel(B) == PAIR
        acc = eng.blind_rotate(cts, lut)
        N = prm.N
        for comp in (0, 1):
            got, want = acc[:, comp * N:(comp + 1) * N], ref_acc[:, comp * N:(comp + 1) * N]
            assert np.array_equal(got, want), \
                f"blind_rotate component {comp}: rows {np.nonzero((got != want).any(1))[0]}"
        assert acc.shape == ref_acc.shape
        out = eng.bootstrap(cts, lut)
        assert np.array_equal(out, ref_out), f"bootstrap: rows {np.nonzero((out != ref_out).any(1))[0]}"


def test_pair_seam_two_luts_full_keys(oracle_mod):
    """Preset n, full keys, B = 2 (one workgroup, all four waves live): two different LUTs by lut_index and two
    different messages, so component 0 and component 1 of the two ciphertexts all differ."""
    O = oracle_mod
    prm = O.params(PRESET)
    okeys = O.Keys(prm, KEY_SEED)
    ck, sk = tfhe_amd.gen_keys(tfhe_amd.Params.preset(tfhe_amd.PRESET_GATE_FFT), KEY_SEED)
    msgs = np.array([2, 5], dtype=np.uint64) * np.uint64((1 << 63) // 8)
    cts = ck.encrypt_torus(msgs, seed=0xC0FFEE10)
    luts = np.stack([O.lut_from_table(prm.N, 8, [(m * 3 + 2) % 8 for m in range(8)], (1 << 63) // 8),
                     O.lut_from_table(prm.N, 8, [(m * 5 + 1) % 8 for m in range(8)], (1 << 63) // 8)])
    idx = np.array([1, 0], dtype=np.uint32)
    ref = O.pbs_batch_fft(prm, okeys, cts, luts, idx)
    assert not np.array_equal(ref[0], ref[1])
    with tfhe_amd.Engine(ck.params, 0) as eng:
        eng.load_keys(sk)
        eng.set_latency_batch(0)
        assert eng.br_kernel(2) == PAIR
        out = eng.pbs(cts, luts, idx)
    assert np.array_equal(out, ref), f"pbs: rows {np.nonzero((out != ref).any(1))[0]}"
