"""Many-LUT PBS on the MI355X (tfhe-rs apply_many_lookup_table): the multi-degree sample extraction kernel
(csrc/sample_extract_many.hip) against the existing degree-0 extraction of a host-rotated accumulator,
Engine.pbs_many against the composition of the stage-level entries, message-level decryption, the device-buffer
entry, argument errors, and the radix layer's opt-in use of it.  Every comparison of ciphertexts is bit-exact."""
import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import radix as R

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001
ENGINES = {"engine": "product_keys", "fhevm_engine": "fhevm_keys", "gate_fft_engine": "gate_fft_keys",
           "fhevm_fft_engine": "fhevm_fft_keys"}
LAT_DEFAULT = {"engine": 1024, "fhevm_engine": 512, "gate_fft_engine": 256, "fhevm_fft_engine": 512}


def rotate_down(acc, p, d):
    """X^{-d} * acc in the accumulator's own ring, per polynomial: (B, (k+1)N) -> the same shape."""
    zp = p.transform == tfhe_amd.TRANSFORM_NTT
    a = acc.reshape(acc.shape[0], p.k + 1, p.N)
    wrapped = a[:, :, :d]
    with np.errstate(over="ignore"):
        neg = np.where(wrapped == 0, np.uint64(0), np.uint64(P) - wrapped) if zp else np.uint64(0) - wrapped
    return np.concatenate([a[:, :, d:], neg.astype(np.uint64)], axis=2).reshape(acc.shape)


def extract_at(eng, acc, d):
    """The sample at degree d through the existing degree-0 extraction (and its conversion to 2^64)."""
    return eng.sample_extract(rotate_down(acc, eng.params, d))


def extract_many_ref(eng, acc, n_fn, stride):
    return np.stack([extract_at(eng, acc, f * stride) for f in range(n_fn)], axis=1)


# ---- 1. the extraction kernel alone ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ENGINES))
def test_sample_extract_many_equals_rotated_degree0(request, name):
    eng = request.getfixturevalue(name)
    p = eng.params
    N, zp = p.N, p.transform == tfhe_amd.TRANSFORM_NTT
    rng = np.random.default_rng(N + zp)
    acc = rng.integers(0, P if zp else 1 << 64, (3, (p.k + 1) * N), dtype=np.uint64)
    acc[:, ::7] = 0
    acc[0, :4] = 0
    acc[1, N - 2:N + 2] = 0
    if zp:
        acc[:, 3::11] = P - 1
        acc[2, N - 1] = P - 1
    refs = {}
    for n_fn, stride in [(1, 1), (2, 1), (2, N // 2), (2, N - 1), (4, N // 4)]:
        out = eng.sample_extract_many(acc, n_fn, stride)
        assert out.shape == (3, n_fn, p.k * N + 1)
        for f in range(n_fn):
            d = f * stride
            if d not in refs:
                refs[d] = extract_at(eng, acc, d)
            assert np.array_equal(out[:, f], refs[d]), (name, n_fn, stride, f)
    assert {0, 1, N // 2, N - 1} <= set(refs)


# ---- 2. / 3. pbs_many against the stages ----------------------------------------------------------------
def random_many_luts(N, n_fn, count, seed):
    rng = np.random.default_rng(seed)
    per = 16 // n_fn
    luts = [tfhe_amd.lut_many(N, 16, [[int(v) for v in rng.integers(0, 16, per)] for _ in range(n_fn)], 1 << 59)
            for _ in range(count)]
    return np.stack([l for l, _ in luts]), luts[0][1]


def staged_reference(eng, sk, cts, luts, idx, n_fn, stride):
    p = eng.params
    if p.order == 1:
        small = eng.keyswitch(cts)
        if sk.ms_zeros is not None:
            small, _ = eng.ms_reduce(small)
        return extract_many_ref(eng, eng.blind_rotate(small, luts, idx), n_fn, stride)
    big = extract_many_ref(eng, eng.blind_rotate(cts, luts, idx), n_fn, stride)
    return eng.keyswitch(big.reshape(-1, p.k * p.N + 1)).reshape(cts.shape[0], n_fn, p.n + 1)


@pytest.mark.parametrize("name", ["gate_fft_engine", "fhevm_fft_engine", "engine", "fhevm_engine"])
def test_pbs_many_equals_stage_composition(request, name):
    eng = request.getfixturevalue(name)
    ck, sk = request.getfixturevalue(ENGINES[name])
    N = eng.params.N
    cts = ck.encrypt(np.array([0, 3, 7, 5, 1]), 16, seed=0xA11CE)
    luts, stride = random_many_luts(N, 2, 2, seed=N)
    idx = np.array([0, 1, 1, 0, 1], dtype=np.uint32)
    outs = []
    try:
        for lat in (LAT_DEFAULT[name], 0):          # latency kernel, then the batch kernel with a ragged workgroup
            eng.set_latency_batch(lat)
            ref = staged_reference(eng, sk, cts, luts, idx, 2, stride)
            out = eng.pbs_many(cts, luts, 2, stride, idx)
            assert out.shape == ref.shape == (5, 2, eng.params.io_dim + 1)
            assert np.array_equal(out, ref), (name, lat)
            outs.append(out)
    finally:
        eng.set_latency_batch(LAT_DEFAULT[name])
    assert not np.array_equal(outs[0][:, 0], outs[0][:, 1])


@pytest.mark.parametrize("name", ["gate_fft_engine", "fhevm_fft_engine", "fhevm_engine"])
def test_pbs_many_of_one_function_is_pbs(request, name):
    eng = request.getfixturevalue(name)
    ck, _ = request.getfixturevalue(ENGINES[name])
    cts = ck.encrypt(np.arange(6) * 2, 16, seed=0xB0B)
    luts, _ = random_many_luts(eng.params.N, 1, 2, seed=5)
    idx = np.array([1, 0, 0, 1, 1, 0], dtype=np.uint32)
    out = eng.pbs_many(cts, luts, 1, eng.params.N, idx)
    assert np.array_equal(out[:, 0], eng.pbs(cts, luts, idx))


# ---- 4. message level --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fn", [2, 4])
def test_pbs_many_decrypts_to_every_table(fhevm_fft_engine, fhevm_fft_keys, n_fn):
    ck, _ = fhevm_fft_keys
    per = 16 // n_fn
    # the top entry of each table differs from entry 0 of the next: a slip across a function's boundary decrypts wrong
    tables = [[(7 * f + 3 * m + 1) % 16 for m in range(per)] for f in range(n_fn)]
    for f in range(n_fn - 1):
        assert tables[f][-1] != tables[f + 1][0]
    lut, stride = tfhe_amd.lut_many(fhevm_fft_engine.params.N, 16, tables, R.DELTA)
    m = np.repeat(np.arange(per), 3)                 # three encryptions of every message
    out = fhevm_fft_engine.pbs_many(ck.encrypt(m, 16, seed=0xD0E + n_fn), lut, n_fn, stride)
    for f in range(n_fn):
        got = ck.decrypt(out[:, f], 16)
        assert [int(v) for v in got] == [tables[f][x] for x in m], f


# ---- 5. device buffers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gate_fft_engine", "fhevm_fft_engine"])
def test_pbs_many_async_equals_host_call(request, name):
    import torch
    eng = request.getfixturevalue(name)
    ck, _ = request.getfixturevalue(ENGINES[name])
    cts = ck.encrypt(np.array([1, 6, 2, 7, 0, 4, 3]), 16, seed=0xFACE)
    luts, stride = random_many_luts(eng.params.N, 2, 2, seed=9)
    idx = np.array([0, 1, 0, 1, 1, 0, 0], dtype=np.uint32)
    ref = eng.pbs_many(cts, luts, 2, stride, idx)
    dev = torch.device("cuda", eng.device)
    d_in = torch.from_numpy(cts.view(np.int64)).to(dev)
    d_luts = torch.from_numpy(luts.view(np.int64)).to(dev)
    d_idx = torch.from_numpy(idx.view(np.int32)).to(dev)
    d_out = eng.pbs_many_device(d_in, d_luts, 2, stride, d_idx)
    assert tuple(d_out.shape) == ref.shape
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), ref)
    d_out2 = torch.zeros_like(d_out)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    eng.pbs_many_async(d_in, d_luts, d_out2, 2, stride, d_idx, stream=side)
    side.synchronize()
    assert np.array_equal(d_out2.cpu().numpy().view(np.uint64), ref)


# ---- 6. argument errors ------------------------------------------------------------------------------------
def test_pbs_many_argument_errors(fhevm_fft_engine, fhevm_fft_keys):
    eng = fhevm_fft_engine
    ck, _ = fhevm_fft_keys
    N = eng.params.N
    m = np.array([2, 5, 7])
    cts = ck.encrypt(m, 16, seed=0xE44)
    luts, stride = random_many_luts(N, 2, 2, seed=3)
    for n_fn, st, idx in [(0, stride, None), (2, N, None), (3, N // 2, None), (2, 0, None),
                          (2, stride, np.array([0, 2, 1], dtype=np.uint32))]:
        with pytest.raises(tfhe_amd.TfheError) as e:
            eng.pbs_many(cts, luts, n_fn, st, idx)
        assert e.value.code == -1
    with pytest.raises(tfhe_amd.TfheError):
        eng.sample_extract_many(np.zeros((1, 2 * N), dtype=np.uint64), 2, N)
    assert eng.pbs_many(cts[:0], luts, 2, stride).shape == (0, 2, eng.params.io_dim + 1)
    ident = eng.generate_accumulator(lambda v: v, 16)
    assert [int(v) for v in ck.decrypt(eng.pbs(cts, ident), 16)] == [2, 5, 7]


def test_pbs_many_needs_keys():
    params = tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_FFT)
    with tfhe_amd.Engine(params, 0) as eng:
        with pytest.raises(tfhe_amd.TfheError) as e:
            eng.pbs_many(np.zeros((1, params.io_dim + 1), dtype=np.uint64), np.zeros((1, params.N), dtype=np.uint64), 2,
                         params.N // 2)
        assert e.value.code == -4


# ---- 7. radix ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [8, 16])
def test_radix_many_lut_gpu(fhevm_fft_engine, fhevm_fft_keys, w):
    ck, _ = fhevm_fft_keys
    B, nb, mod = 3, w // 2, 1 << w
    a = np.array([mod - 1, 0, 0x5A5A % mod], dtype=np.uint64)
    b = np.array([1, 1, 0xC3C3 % mod], dtype=np.uint64)
    counts = {}
    for many in (False, True):
        c = R.RadixCircuit(fhevm_fft_engine, many_lut=many)
        A = R.RadixUint.encrypt(c, ck, a, w, seed=0x77, stream0=0)
        Bv = R.RadixUint.encrypt(c, ck, b, w, seed=0x77, stream0=B * nb)
        add = c.run(R.fhevm_op(c, "add", A, Bv))
        after_add = (c.pbs_count, c.launches)
        sub = c.run(R.fhevm_op(c, "sub", A, Bv))
        np.testing.assert_array_equal(add.decrypt(ck), (a + b) % np.uint64(mod))
        np.testing.assert_array_equal(sub.decrypt(ck), (a - b) % np.uint64(mod))
        counts[many] = (after_add, (c.pbs_count - after_add[0], c.launches - after_add[1]))
    (add0, sub0), (add1, sub1) = counts[False], counts[True]
    assert add1 == (add0[0] - B * nb, add0[1])
    assert sub1 == (sub0[0] - B * (nb - 1), sub0[1])
