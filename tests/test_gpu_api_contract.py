"""Host API contract of libtfhe_hip.so on the MI355X that no other suite pins: which timing slots one PBS call
fills (plain and many-LUT run the same stage sequence), the plain PBS through its host-buffer and device-buffer
entries, the single-shard stage entries (blind rotate, sample extraction, noise reduction, NTT) that share one
staged-call frame, and the rows of the back-end table (kernel names, latency crossovers).  Every comparison of
ciphertexts is bit-exact."""
import numpy as np
import pytest

import tfhe_amd

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001
ENGINES = {"engine": "product_keys", "fhevm_engine": "fhevm_keys", "gate_fft_engine": "gate_fft_keys",
           "fhevm_fft_engine": "fhevm_fft_keys"}


def two_luts(eng, n_fn=1):
    """Two LUTs of n_fn functions each over 16 messages, and the stride between the functions."""
    per = 16 // n_fn
    tabs = [[[(5 * f + 3 * m + t) % 16 for m in range(per)] for f in range(n_fn)] for t in (1, 2)]
    luts = [tfhe_amd.lut_many(eng.params.N, 16, t, 1 << 59) for t in tabs]
    return np.stack([l for l, _ in luts]), luts[0][1]


# ---- 1. timing slots: 0 = blind rotation (+ sample extraction), 1 = keyswitch, 2 = MS noise reduction --------
@pytest.mark.parametrize("name", list(ENGINES))
def test_timing_slots_of_one_pbs_call(request, name):
    eng = request.getfixturevalue(name)
    ck, _ = request.getfixturevalue(ENGINES[name])
    cts = ck.encrypt(np.array([1, 6, 11]), 16, seed=0x71E)
    luts, stride = two_luts(eng, 2)
    want = (1, 1, 1) if eng.params.order == 1 else (1, 1, 0)   # the P-FHEVM session keys carry the MS key
    eng.timing(True)
    try:
        eng.timing_reset()
        eng.pbs(cts, luts[:1])
        assert tuple(eng.timing_stats(w)[1] for w in range(3)) == want, name
        eng.timing_reset()
        eng.pbs_many(cts, luts[:1], 2, stride)
        assert tuple(eng.timing_stats(w)[1] for w in range(3)) == want, name
    finally:
        eng.timing_reset()
        eng.timing(False)


# ---- 2. plain PBS: host buffers against device buffers (test_gpu_many_lut.py has the many-LUT half) ----------
@pytest.mark.parametrize("name", ["gate_fft_engine", "fhevm_fft_engine"])
def test_pbs_device_equals_host_call(request, name):
    import torch
    eng = request.getfixturevalue(name)
    ck, _ = request.getfixturevalue(ENGINES[name])
    cts = ck.encrypt(np.array([3, 0, 9, 14, 5]), 16, seed=0xDE71CE)
    luts, _ = two_luts(eng)
    idx = np.array([1, 0, 0, 1, 1], dtype=np.uint32)
    ref = eng.pbs(cts, luts, idx)
    assert not np.array_equal(ref, eng.pbs(cts, luts[:1]))      # the index selects: LUT 1 differs from LUT 0
    dev = torch.device("cuda", eng.device)
    d_out = eng.pbs_device(torch.from_numpy(cts.view(np.int64)).to(dev), torch.from_numpy(luts.view(np.int64)).to(dev),
                           torch.from_numpy(idx.view(np.int32)).to(dev))
    assert tuple(d_out.shape) == ref.shape == (5, eng.params.io_dim + 1)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), ref)


# ---- 3. the stage entries -------------------------------------------------------------------------------------
def test_stage_entries_fhevm_fft(fhevm_fft_engine, fhevm_fft_keys, oracle_mod):
    eng = fhevm_fft_engine
    ck, sk = fhevm_fft_keys
    p = eng.params
    luts, _ = two_luts(eng)
    small = eng.keyswitch(ck.encrypt(np.array([2, 7, 13]), 16, seed=0x57A6E))
    assert small.shape == (3, p.n + 1)
    acc = eng.blind_rotate(small, luts, np.array([0, 1, 0], dtype=np.uint32))
    assert acc.shape == (3, (p.k + 1) * p.N) and acc.any()
    big = eng.sample_extract(acc)
    prm = oracle_mod.params(tfhe_amd.PRESET_FHEVM_FFT)
    assert big.shape == (3, p.k * p.N + 1)
    assert all(np.array_equal(big[b], oracle_mod.sample_extract_torus(prm, acc[b])) for b in range(3))
    reduced, picks = eng.ms_reduce(small)
    assert reduced.shape == (3, p.n + 1) and picks.shape == (3,)
    count = sk.ms_zeros.shape[0]
    assert all(-1 <= int(z) < count for z in picks), picks


# the degree-0 extraction is the n_fn = 1 case of the many-LUT kernel on every back end: against the oracle
@pytest.mark.parametrize("name", list(ENGINES))
def test_sample_extract_equals_oracle(request, oracle_mod, name):
    eng = request.getfixturevalue(name)
    p = eng.params
    fft = p.transform == tfhe_amd.TRANSFORM_FFT64
    prm = oracle_mod.params(list(ENGINES).index(name))      # ENGINES lists the fixtures in preset order
    assert (prm.N, prm.k, prm.transform) == (p.N, p.k, p.transform)
    acc = np.random.default_rng(0x5E0).integers(1, P, (3, 2 * p.N), dtype=np.uint64)   # residues: valid on both rings
    # word 0, word N - 1 and body word 0: distinct and non-zero
    acc[:, 0] = 0x1111_0000_0000_0001 + np.arange(3, dtype=np.uint64)
    acc[:, p.N - 1] = 0x2222_0000_0000_0002 + np.arange(3, dtype=np.uint64)
    acc[:, p.N] = 0x3333_0000_0000_0003 + np.arange(3, dtype=np.uint64)
    ref = oracle_mod.sample_extract_torus if fft else oracle_mod.sample_extract
    big = eng.sample_extract(acc)
    assert big.shape == (3, p.k * p.N + 1)
    for b in range(3):
        assert np.array_equal(big[b], ref(prm, acc[b])), (name, b)


# ---- 4. the back-end table: kernel names and default latency crossovers, one batch-size decision -----------------
BR_ROWS = {"engine": (1024, "blind_rotate_lat_kernel", "blind_rotate_kernel"),
           "fhevm_engine": (512, "blind_rotate2048_lat_kernel", "blind_rotate2048_kernel"),
           "gate_fft_engine": (256, "blind_rotate_fft_lat_kernel", "blind_rotate_fft_pair_kernel"),
           "fhevm_fft_engine": (512, "blind_rotate_fft2k_kernel", "blind_rotate_fft2k_kernel")}


@pytest.mark.parametrize("name", list(ENGINES))
def test_br_kernel_names_and_crossover(request, name):
    eng = request.getfixturevalue(name)
    crossover, lat, batch = BR_ROWS[name]
    try:
        assert eng.br_kernel(crossover) == lat and eng.br_kernel(crossover + 1) == batch, name
        assert eng.br_kernel(1) == lat
        eng.set_latency_batch(0)
        assert eng.br_kernel(1) == batch
    finally:
        eng.set_latency_batch(crossover)
    assert eng.br_kernel(crossover) == lat


def test_ntt_roundtrip_in_place(fhevm_engine):
    polys = np.random.default_rng(2048).integers(0, P, (2, fhevm_engine.params.N), dtype=np.uint64)
    spec = fhevm_engine.ntt_fwd(polys)
    assert spec.shape == polys.shape and not np.array_equal(spec, polys)
    assert np.array_equal(fhevm_engine.ntt_inv(spec), polys)
