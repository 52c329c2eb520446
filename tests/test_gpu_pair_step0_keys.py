"""The P-GATE pair kernel's level step 0 takes its key words from L2 into registers (pbs_fft.hip, load_step0_keys): wave
(p, c) reads rows (c, 0, j = 0, 1) of BSK_i itself, mac_first turns each key word into the partial sum that takes its
registers, and the LDS chunk of level step 1 is issued while step 0 still runs, with no workgroup barrier in front of
it.  All of it is placement: every accumulator and every output stays bit-equal to oracle/fft_oracle.c.  A wrong row,
component or j, or a key word landing in the other output's registers, changes every coefficient.  The cases:
  (n, B) = (1, 1): the only CMUX: the step-0 rows are the first and the step-2 rows the last of the key, the early
           chunk has no exchange before it; a lone ciphertext beside a padding pair
           (2, 3): the CMUX seam is crossed once, with the early chunk behind a real exchange; an odd batch
           (5, 7): four workgroups, the last half padding; the rows of CMUX n - 1 end at the buffer's num_records
           (4, 1030): 515 workgroups: on a 256-CU part both slots of every CU are taken and a second dispatch round
           starts, so both priority halves and the staggered half-round take part
on a rotation-only engine with the keys and the edge-word inputs of test_gpu_pair_keystream.py, and a two-entry LUT
chosen by lut_index through Engine.pbs with the preset's full keys at B = 3 (the row offsets up to i = 629)."""
import numpy as np
import pytest

from conftest import KEY_SEED

import tfhe_amd
import test_decompress as T
from test_gpu_decompress import rotation_inputs
from test_gpu_pair_keystream import PAIR, PRESET

pytestmark = pytest.mark.gpu
CASES = [(1, 1), (2, 3), (5, 7), (4, 1030)]


@pytest.mark.parametrize("n,B", CASES, ids=lambda v: str(v))
def test_pair_kernel_step0_keys_off_preset_n(oracle_mod, n, B):
    O = oracle_mod
    prm = O.params(PRESET)
    dprm = T.with_n(prm, n)
    glwe_key = O.Keys(prm, T.SEED, with_bsk=False, with_ksk=False).glwe_key
    lwe_key = np.random.default_rng(40 + n).integers(0, 2, n).astype(np.uint64)
    keys = T.rotation_keys(O, dprm, T.DK_SEED, lwe_key, glwe_key)
    cts = rotation_inputs(prm.N, n, B, 1200 + n)
    lut = O.lut_from_table(prm.N, 16, [(7 * m + 2) % 16 for m in range(16)], 1 << 59)
    ref = [T.bootstrap_ref(O, dprm, keys, cts[q], lut) for q in range(B)]
    ref_acc, ref_out = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    params = T.with_n(tfhe_amd.Params.preset(PRESET), n)
    with tfhe_amd.Engine(params, 0) as eng:
        eng.load_bsk(keys.bsk)
        eng.set_latency_batch(0)
        assert eng.br_kernel(B) == PAIR
        acc = eng.blind_rotate(cts, lut)
        assert np.array_equal(acc, ref_acc), f"blind_rotate: rows {np.nonzero((acc != ref_acc).any(1))[0]}"
        out = eng.bootstrap(cts, lut)
        assert np.array_equal(out, ref_out), f"bootstrap: rows {np.nonzero((out != ref_out).any(1))[0]}"


def test_pair_kernel_step0_keys_full_keys(oracle_mod):
    """Preset n, full keys, B = 3 (two workgroups, one padding pair), two LUTs by lut_index through Engine.pbs."""
    O = oracle_mod
    prm = O.params(PRESET)
    okeys = O.Keys(prm, KEY_SEED)
    ck, sk = tfhe_amd.gen_keys(tfhe_amd.Params.preset(tfhe_amd.PRESET_GATE_FFT), KEY_SEED)
    msgs = np.random.default_rng(1291).integers(0, 8, 3).astype(np.uint64) * np.uint64((1 << 63) // 8)
    cts = ck.encrypt_torus(msgs, seed=0xC0FFEE12)
    luts = np.stack([O.lut_from_table(prm.N, 8, [(m * 3 + 2) % 8 for m in range(8)], (1 << 63) // 8),
                     O.lut_constant(prm.N, 3 << 60)])
    idx = np.array([0, 1, 0], dtype=np.uint32)
    ref = O.pbs_batch_fft(prm, okeys, cts, luts, idx)
    with tfhe_amd.Engine(ck.params, 0) as eng:
        eng.load_keys(sk)
        eng.set_latency_batch(0)
        assert eng.br_kernel(3) == PAIR
        out = eng.pbs(cts, luts, idx)
    assert np.array_equal(out, ref), f"pbs: rows {np.nonzero((out != ref).any(1))[0]}"
