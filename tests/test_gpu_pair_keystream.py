"""The P-GATE pair kernel's two input streams (pbs_fft.hip): the LWE mask word, loaded one CMUX ahead of the CMUX that
rotates by it, and the bootstrapping-key chunk, whose 1 KB LDS-DMA pieces ride on immediate offsets.  Both are placement
only, so every accumulator and every output stays bit-equal to oracle/fft_oracle.c.  What these cases add is the trip
counts and batches at which a word taken one CMUX early or late, or a key KiB landing in the wrong place, would show:
  (n, B) = (1, 1): the only prefetch reads the body word; a lone ciphertext beside a padding pair
           (2, 3): six level steps; an odd batch; two workgroups
           (3, 5): three workgroups, the last one half padding
           (65, 4): the rotation's slot part and sign both change along the way
on a rotation-only engine with the keys and the edge-word inputs of test_gpu_decompress.py, and a two-entry LUT chosen
by lut_index through Engine.pbs with the preset's full keys at B = 3."""
import numpy as np
import pytest

from conftest import KEY_SEED

import tfhe_amd
import test_decompress as T
from test_gpu_decompress import rotation_inputs

pytestmark = pytest.mark.gpu
PRESET = 2  # P-GATE FFT64
PAIR = "blind_rotate_fft_pair_kernel"
CASES = [(1, 1), (2, 3), (3, 5), (65, 4)]


@pytest.mark.parametrize("n,B", CASES, ids=lambda v: str(v))
def test_pair_kernel_off_preset_n(oracle_mod, n, B):
    O = oracle_mod
    prm = O.params(PRESET)
    dprm = T.with_n(prm, n)
    glwe_key = O.Keys(prm, T.SEED, with_bsk=False, with_ksk=False).glwe_key
    lwe_key = np.random.default_rng(n).integers(0, 2, n).astype(np.uint64)
    keys = T.rotation_keys(O, dprm, T.DK_SEED, lwe_key, glwe_key)
    cts = rotation_inputs(prm.N, n, B, 177 + n)
    if n == 65:
        # the masks of one row walk through every slot part and both signs of a = 1024 s + 64 A + r
        cts[0, :n] = (np.arange(n, dtype=np.uint64) * np.uint64(2048 // 64 + 1) % np.uint64(2048)) << np.uint64(53)
    lut = O.lut_from_table(prm.N, 16, [(5 * m + 3) % 16 for m in range(16)], 1 << 59)
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


def test_pair_kernel_lut_index_full_keys(oracle_mod):
    """Preset n, full keys, B = 3 (two workgroups, one padding pair), two LUTs by lut_index through Engine.pbs."""
    O = oracle_mod
    prm = O.params(PRESET)
    okeys = O.Keys(prm, KEY_SEED)
    ck, sk = tfhe_amd.gen_keys(tfhe_amd.Params.preset(tfhe_amd.PRESET_GATE_FFT), KEY_SEED)
    msgs = np.random.default_rng(91).integers(0, 8, 3).astype(np.uint64) * np.uint64((1 << 63) // 8)
    cts = ck.encrypt_torus(msgs, seed=0xC0FFEE91)
    luts = np.stack([O.lut_from_table(prm.N, 8, [(m * 5 + 1) % 8 for m in range(8)], (1 << 63) // 8),
                     O.lut_constant(prm.N, 1 << 61)])
    idx = np.array([1, 0, 1], dtype=np.uint32)
    ref = O.pbs_batch_fft(prm, okeys, cts, luts, idx)
    with tfhe_amd.Engine(ck.params, 0) as eng:
        eng.load_keys(sk)
        eng.set_latency_batch(0)
        assert eng.br_kernel(3) == PAIR
        out = eng.pbs(cts, luts, idx)
    assert np.array_equal(out, ref), f"pbs: rows {np.nonzero((out != ref).any(1))[0]}"
