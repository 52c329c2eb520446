"""Host API contract of libtfhe_hip.so on the MI355X that no other suite pins: which timing slots one PBS call
fills (plain and many-LUT run the same stage sequence), the plain PBS through its host-buffer and device-buffer
entries, and the single-shard stage entries (blind rotate, sample extraction, noise reduction, NTT) that share one
staged-call frame.  Every comparison of ciphertexts is bit-exact."""
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
def test_stage_entries_fhevm_fft(fhevm_fft_engine, fhevm_fft_keys):
    eng = fhevm_fft_engine
    ck, sk = fhevm_fft_keys
    p = eng.params
    luts, _ = two_luts(eng)
    small = eng.keyswitch(ck.encrypt(np.array([2, 7, 13]), 16, seed=0x57A6E))
    assert small.shape == (3, p.n + 1)
    acc = eng.blind_rotate(small, luts, np.array([0, 1, 0], dtype=np.uint32))
    assert acc.shape == (3, (p.k + 1) * p.N) and acc.any()
    assert np.array_equal(eng.sample_extract(acc), eng.sample_extract_many(acc, 1, p.N)[:, 0])
    reduced, picks = eng.ms_reduce(small)
    assert reduced.shape == (3, p.n + 1) and picks.shape == (3,)
    count = sk.ms_zeros.shape[0]
    assert all(-1 <= int(z) < count for z in picks), picks


def test_ntt_roundtrip_in_place(fhevm_engine):
    polys = np.random.default_rng(2048).integers(0, P, (2, fhevm_engine.params.N), dtype=np.uint64)
    spec = fhevm_engine.ntt_fwd(polys)
    assert spec.shape == polys.shape and not np.array_equal(spec, polys)
    assert np.array_equal(fhevm_engine.ntt_inv(spec), polys)
