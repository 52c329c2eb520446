"""The P-GATE pair kernel after its LDS traffic was re-placed by hand (pbs_fft.hip: pipelined MAC key reads, transpose
stores interleaved with their twiddle multiplies, no wait between a wave's transpose stores and reads, grouped
exchange reads).  Placement only, so every result stays bit-equal to oracle/fft_oracle.c; what these
tests add to test_gpu_fft.py is the shapes where a missing or misplaced wait would show:
  * forced tiny batches on the pair kernel: one workgroup with a padding partner (B = 1), one full workgroup (2), both (3);
  * a contended batch of 4 x (CU count) + 2 ciphertexts: two co-resident workgroups on every CU (LDS contention between
    them) plus one workgroup in a second round, oracle-compared across the dispatch-half boundaries;
  * the same contended batch three times: identical outputs (a race would differ from run to run).
"""
import numpy as np
import pytest

from conftest import KEY_SEED

import tfhe_amd

pytestmark = pytest.mark.gpu
N = 1024


@pytest.fixture(scope="module")
def fft_keys():
    return tfhe_amd.gen_keys(tfhe_amd.Params.preset(tfhe_amd.PRESET_GATE_FFT), KEY_SEED)


@pytest.fixture(scope="module")
def fft_engine(fft_keys):
    ck, sk = fft_keys
    eng = tfhe_amd.Engine(ck.params, 0)
    eng.load_keys(sk)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def fft_params(oracle_mod):
    return oracle_mod.params(2)


@pytest.fixture(scope="module")
def fft_okeys(oracle_mod, fft_params):
    return oracle_mod.Keys(fft_params, KEY_SEED)


@pytest.fixture(scope="module")
def small_case(fft_keys, oracle_mod, fft_params, fft_okeys):
    """Three ciphertexts, two LUTs chosen by lut_index, and the oracle's accumulators and PBS outputs for them
    (computed once; the B = 1, 2, 3 cases take prefixes: the oracle works ciphertext by ciphertext)."""
    ck, _ = fft_keys
    rng = np.random.default_rng(71)
    msgs = rng.integers(0, 8, 3).astype(np.uint64) * np.uint64((1 << 63) // 8)
    cts = ck.encrypt_torus(msgs, seed=0xC0FFEE71)
    luts = np.stack([oracle_mod.lut_from_table(N, 8, [(m * 3 + 2) % 8 for m in range(8)], (1 << 63) // 8),
                     oracle_mod.lut_constant(N, 1 << 61)])
    idx = np.array([1, 0, 1], dtype=np.uint32)
    acc = np.stack([oracle_mod.blind_rotate_fft(fft_params, fft_okeys, cts[i], luts[idx[i]]) for i in range(3)])
    out = oracle_mod.pbs_batch_fft(fft_params, fft_okeys, cts, luts, idx)
    for a in (cts, luts, idx, acc, out):
        a.setflags(write=False)
    return cts, luts, idx, acc, out


@pytest.mark.parametrize("B", [1, 2, 3])
def test_pair_kernel_small_forced_batches_bitexact(fft_engine, small_case, B):
    cts, luts, idx, acc_ref, out_ref = small_case
    try:
        fft_engine.set_latency_batch(0)  # every batch on the pair kernel
        acc = fft_engine.blind_rotate(cts[:B], luts, idx[:B])
        out = fft_engine.pbs(cts[:B], luts, idx[:B])
    finally:
        fft_engine.set_latency_batch(256)  # the P-GATE FFT64 default
    assert np.array_equal(acc, acc_ref[:B]), "pair-kernel accumulators differ from the oracle"
    assert np.array_equal(out, out_ref[:B]), "pair-kernel PBS outputs differ from the oracle"


@pytest.fixture(scope="module")
def contended(fft_engine, fft_keys):
    """B = 4 x CUs + 2 (1026 on MI355X): workgroups 0 .. 2 CUs - 1 fill every CU twice, workgroup 2 CUs runs after."""
    ck, _ = fft_keys
    cus = fft_engine.cus_per_device
    B = 4 * cus + 2
    bits = np.random.default_rng(72).integers(0, 2, B).astype(bool)
    cts = ck.encrypt_bool(bits, seed=0xC0FFEE72)
    out = fft_engine.pbs(cts, fft_engine.gate_lut())
    for a in (bits, cts, out):
        a.setflags(write=False)
    return cus, bits, cts, out


def test_contended_batch_decrypts_and_sampled_bitexact(contended, fft_keys, oracle_mod, fft_params, fft_okeys):
    ck, _ = fft_keys
    cus, bits, cts, out = contended
    B = len(bits)
    assert B > 256, "the batch must be above the latency range to run on the pair kernel"
    assert np.array_equal(ck.decrypt_bool(out), bits)
    # two ciphertexts per workgroup: the first workgroups, the dispatch-half boundary (workgroups CUs - 1 | CUs, where
    # the wave priority and the start stagger switch), the end of the first round and the last workgroup
    sample = np.r_[0:8, 2 * cus - 4:2 * cus + 4, B - 8:B]
    assert len(sample) <= 24
    ref = oracle_mod.pbs_batch_fft(fft_params, fft_okeys, cts[sample], oracle_mod.lut_constant(N, 1 << 61)[None])
    assert np.array_equal(out[sample], ref)


def test_contended_batch_run_to_run_identical(contended, fft_engine):
    _, _, cts, out = contended
    lut = fft_engine.gate_lut()
    for run in (2, 3):
        assert np.array_equal(fft_engine.pbs(cts, lut), out), f"run {run} differs from run 1"
