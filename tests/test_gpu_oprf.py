"""Oblivious pseudo-random ciphertexts on the MI355X: the mask kernel (csprng.hip) word for word against the host
stream, Engine.oprf bit-exact against the oracle route of tests/oprf_ref.py at small n on both blind-rotation
kernels and in the host, async and device forms, decryption to the predicted values at the real dimensions, the
radix and integer operators on small engines, two shards, and the ABI's refusals."""
import ctypes

import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import integer as I
from tfhe_amd import radix as R
import oprf_ref as F

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5A5A5A5A5


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(torch.device("cuda", 0))


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


# ---- 1. the mask kernel ---------------------------------------------------------------------------------------
def kernel_seeds(rows):
    """distinct seeds: (0, 0), two that differ only in hi, two that differ only in the top byte of hi, then a
    counter pattern in both halves"""
    fixed = [(0, 0), (0x1122334455667788, 5), (0x1122334455667788, 6), (9, 0x01FFEEDDCCBBAA99), (9, 0x02FFEEDDCCBBAA99)]
    more = [(0x9E3779B97F4A7C15 * (i + 1) % F.M64, 0xC2B2AE3D27D4EB4F * (i + 3) % F.M64) for i in range(rows)]
    return np.array((fixed + more)[:rows], dtype=np.uint64)


@pytest.fixture(scope="module")
def keyless_engine():
    with tfhe_amd.Engine(tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_FFT), 0) as eng:
        yield eng


@pytest.mark.parametrize("dim", (1, 2, 3, 15, 16, 17, 918, 2049, 4099))
def test_mask_kernel_matches_host_stream(keyless_engine, dim):
    eng = keyless_engine
    for rows in (1, 3, 70):
        # every seed shape of kernel_seeds appears in the 70-row call; the 1- and 3-row calls start further down
        seeds = kernel_seeds(70)[{1: slice(3, 4), 3: slice(1, 4), 70: slice(0, 70)}[rows]]
        for first in (0, 1, 13, (1 << 33) - 3):
            want = np.stack([F.stream_words(s, first, dim) for s in seeds])
            got = eng.csprng_rows(seeds, dim, first)
            assert np.array_equal(got, want), f"host form, rows {rows} first_word {first}: " \
                f"{np.argwhere(got != want)[:4].tolist()}"
            d_out = to_dev(np.full((rows, dim + 2), SENTINEL, dtype=np.uint64))
            eng.csprng_rows_async(to_dev(seeds), dim, d_out, first)
            out = to_host(d_out)
            assert np.array_equal(out[:, :dim], want), f"device form, rows {rows} first_word {first}"
            assert np.all(out[:, dim:] == SENTINEL), "guard words after a row were written"


def test_mask_kernel_seed_sensitivity(keyless_engine):
    s = kernel_seeds(5)
    out = keyless_engine.csprng_rows(s, 16)
    assert len({r.tobytes() for r in out}) == 5          # hi, and the top byte of hi, reach the key schedule


# ---- 2. bit-exact against the oracle route ------------------------------------------------------------------------
def tables(N, kinds):
    luts, posts = [], []
    for kind in kinds:
        lut, post = (tfhe_amd.lut_constant(N, tfhe_amd.MU), 0) if kind == "gate" else tfhe_amd.lut_oprf(N, *kind)
        luts.append(lut)
        posts.append(post)
    return np.stack(luts), posts


def check_values(dprm, keys, out, masks, kinds, idx):
    ph = F.out_phase(dprm, keys, out)
    for l, kind in enumerate(kinds):
        sel = idx == l
        if kind == "gate":
            assert np.array_equal(tfhe_amd.decode_bool(ph[sel]), F.predict_gate(masks[sel], keys.lwe_key, dprm.N))
        else:
            v, err = F.decode(ph[sel], kind[1])
            assert int(err.max()) < 1 << (63 - kind[1])
            assert np.array_equal(v, F.predict(masks[sel], keys.lwe_key, dprm.N, kind[0]))


def all_forms(eng, seeds, luts, posts, idx):
    import torch
    host = eng.oprf(seeds, luts, posts, idx)
    d_seeds, d_luts, d_idx = to_dev(seeds), to_dev(luts), torch.from_numpy(idx.astype(np.int32)).to("cuda:0")
    d_post = to_dev(np.array([p % F.M64 for p in posts], dtype=np.uint64))
    d_out = to_dev(np.full(host.shape, SENTINEL, dtype=np.uint64))
    eng.oprf_async(d_seeds, d_luts, d_post, d_out, d_idx)
    dev = eng.oprf_device(d_seeds, d_luts, d_post, d_idx)
    torch.cuda.synchronize()
    return host, to_host(d_out), to_host(dev)


@pytest.mark.parametrize("n", (1, 2, 3, 64))
def test_oprf_bit_exact_order1(n):
    rows, kinds = 6, [(2, 5), (1, 5)]
    dprm, keys = F.small_keys(3, n)
    seeds = F.block_seeds((0x0F2F0100 + n, 3), rows)
    masks = F.masks_of(seeds, n)
    idx = (np.arange(rows) % 2).astype(np.uint32)
    luts, posts = tables(dprm.N, kinds)
    ref = F.oracle_rows(dprm, keys, masks, luts, posts, idx)
    check_values(dprm, keys, ref, masks, kinds, idx)
    params, _, sk = F.product_side(3, n)
    with tfhe_amd.Engine(params, 0) as eng:
        eng.load_bsk(sk.bsk)                      # rotation-only: order 1 needs no keyswitching key
        for lat in (1 << 20, 0):
            eng.set_latency_batch(lat)
            for name, out in zip(("host", "async", "device"), all_forms(eng, seeds, luts, posts, idx)):
                assert out.shape == (rows, dprm.k * dprm.N + 1)
                assert np.array_equal(out, ref), f"{name} form on {eng.br_kernel(rows)}: rows " \
                    f"{np.nonzero((out != ref).any(1))[0]}"
        no_index = eng.oprf(seeds, luts[:1], posts[:1])                   # lut_index null: LUT 0 everywhere
        assert np.array_equal(no_index, F.oracle_rows(dprm, keys, masks, luts[:1], posts[:1], None))


def test_oprf_bit_exact_order0():
    n, rows, kinds = 64, 6, ["gate", (2, 5)]
    dprm, keys = F.small_keys(2, n)
    seeds = F.block_seeds((0x0F2F0200, 3), rows)
    masks = F.masks_of(seeds, n)
    idx = (np.arange(rows) % 2).astype(np.uint32)
    luts, posts = tables(dprm.N, kinds)
    ref = F.oracle_rows(dprm, keys, masks, luts, posts, idx)
    check_values(dprm, keys, ref, masks, kinds, idx)
    params, _, sk = F.product_side(2, n)
    with tfhe_amd.Engine(params, 0) as eng:
        eng.load_keys(sk)
        for lat in (1 << 20, 0):
            eng.set_latency_batch(lat)
            for name, out in zip(("host", "async", "device"), all_forms(eng, seeds, luts, posts, idx)):
                assert out.shape == (rows, n + 1)
                assert np.array_equal(out, ref), f"{name} form on {eng.br_kernel(rows)}"


# ---- 3. the real dimensions ---------------------------------------------------------------------------------------
def test_oprf_real_dimensions_fhevm(fhevm_fft_engine, fhevm_fft_keys):
    ck, _ = fhevm_fft_keys
    p = ck.params
    rows, kinds = 64, [(2, 5), (1, 5)]
    seeds = F.block_seeds(F.PARENT, rows)
    masks = F.masks_of(seeds, p.n)
    idx = (np.arange(rows) % 2).astype(np.uint32)
    luts, posts = tables(p.N, kinds)
    out = fhevm_fft_engine.oprf(seeds, luts, posts, idx)
    ph = ck.phase(out)
    for l, (rb, fb) in enumerate(kinds):
        v, err = F.decode(ph[idx == l], fb)
        assert int(err.max()) < 1 << (63 - fb)
        assert np.array_equal(v, F.predict(masks[idx == l], ck.lwe_key, p.N, rb))


def test_oprf_real_dimensions_gate(gate_fft_engine, gate_fft_keys):
    ck, _ = gate_fft_keys
    p = ck.params
    seeds = F.block_seeds(F.PARENT, 64)
    out = gate_fft_engine.oprf(seeds, gate_fft_engine.gate_lut(), [0])
    assert out.shape == (64, p.n + 1)
    assert np.array_equal(ck.decrypt_bool(out), F.predict_gate(F.masks_of(seeds, p.n), ck.lwe_key, p.N))


# ---- 4. the operators ---------------------------------------------------------------------------------------------
REQUESTS = np.array([[0x0F2F0300, 0], [0x0F2F0300, 1], [0xFFFFFFFFFFFFFFFF, 0x8000000000000000]], dtype=np.uint64)


def radix_expect(ck, seeds, t):
    p = ck.params
    bits = [2] * (t // 2) + [1] * (t % 2)
    vals = []
    for s in seeds:
        masks = F.masks_of(F.block_seeds(s, len(bits)), p.n)
        vals.append(sum(int(F.predict(masks[j:j + 1], ck.lwe_key, p.N, rb)[0]) << (2 * j) for j, rb in enumerate(bits)))
    return vals


def test_radix_rand_on_device():
    params, ck, sk = F.product_side(3, 64, full=True)
    with tfhe_amd.Engine(params, 0) as eng:
        eng.load_keys(sk)
        c = R.RadixCircuit(eng)
        for w in (8, 16):
            x = R.RadixUint.rand(c, REQUESTS, w)
            assert [int(v) for v in x.decrypt(ck)] == radix_expect(ck, REQUESTS, w)
        b = c.run(R.fhevm_rand(c, "rand", REQUESTS, 1))
        masks = np.concatenate([F.masks_of(F.block_seeds(s, 1), 64) for s in REQUESTS])
        assert np.array_equal(ck.decrypt(b, R.SPACE).astype(np.int64), F.predict(masks, ck.lwe_key, params.N, 1))
        y = R.RadixUint.rand_bounded(c, REQUESTS, 8, 8)
        want = radix_expect(ck, REQUESTS, 3)
        assert [int(v) for v in y.decrypt(ck)] == want and max(want) < 8
        assert not y.blocks[:, 2:].any()
        x = R.RadixUint.rand(c, REQUESTS, 8)
        z = c.run(R.fhevm_op(c, "add", x, 1))
        assert [int(v) for v in z.decrypt(ck)] == [(v + 1) % 256 for v in radix_expect(ck, REQUESTS, 8)]


def test_integer_rand_on_device():
    params, ck, sk = F.product_side(2, 64)
    want = []
    for s in REQUESTS:
        bits = F.predict_gate(F.masks_of(F.block_seeds(s, 8), 64), ck.lwe_key, params.N)
        want.append(sum(1 << j for j in range(8) if bits[j]))
    with tfhe_amd.Engine(params, 0) as eng:
        eng.load_keys(sk)
        c = I.Circuit(eng)
        x = I.FheUint.rand(c, REQUESTS, 8)
        assert [int(v) for v in x.decrypt(ck)] == want
        y = c.run(I.fhevm_op(c, "add", x, 1))
        assert [int(v) for v in y.decrypt(ck)] == [(v + 1) % 256 for v in want]
        cd = I.Circuit(eng, device="cuda:0")                               # device-resident: oprf_device
        xd = I.FheUint.rand(cd, REQUESTS, 8)
        assert np.array_equal(to_host(xd.bits), x.bits)


# ---- 5. two shards ------------------------------------------------------------------------------------------------
def test_oprf_two_shards_keep_seed_order():
    params, _, sk = F.product_side(3, 64)
    seeds = F.block_seeds((0x0F2F0400, 0), 7)
    idx = (np.arange(7) % 2).astype(np.uint32)
    luts, posts = tables(params.N, [(2, 5), (1, 5)])
    with tfhe_amd.Engine(params, 0) as one:
        one.load_bsk(sk.bsk)
        ref = one.oprf(seeds, luts, posts, idx)
    with tfhe_amd.Engine(params, [0, 0]) as two:
        two.load_bsk(sk.bsk)
        out = two.oprf(seeds, luts, posts, idx)
    assert np.array_equal(out, ref)
    assert len({r.tobytes() for r in ref}) == 7


# ---- 6. refusals --------------------------------------------------------------------------------------------------
def test_oprf_refusals():
    L = tfhe_amd.lib()
    u64 = tfhe_amd._u64
    seeds = F.block_seeds(F.PARENT, 4)

    def call(eng, rows, luts, posts, n_lut, idx, out):
        return L.tfhe_hip_oprf(eng._h, u64(seeds), rows, u64(luts), u64(posts), n_lut,
                               idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if idx is not None else None, u64(out))

    params, _, sk = F.product_side(2, 64)                 # order 0
    luts, posts = tables(params.N, ["gate", (2, 5)])
    posts = np.array(posts, dtype=np.uint64)
    with tfhe_amd.Engine(params, 0) as eng:
        out = np.full((4, 65), SENTINEL, dtype=np.uint64)
        assert call(eng, 4, luts, posts, 2, None, out) == -4          # ENOKEYS: nothing loaded
        eng.load_bsk(sk.bsk)
        assert call(eng, 4, luts, posts, 2, None, out) == -4          # ENOKEYS: order 0 keyswitches, BSK alone
        assert b"keyswitching key" in L.tfhe_hip_last_error()
        eng.load_keys(sk)
        assert call(eng, 4, luts, posts, 0, None, out) == -1          # EINVAL: n_lut == 0
        assert call(eng, 4, luts, posts, 2, np.array([0, 1, 2, 0], dtype=np.uint32), out) == -1   # lut_index >= n_lut
        assert L.tfhe_hip_oprf(eng._h, None, 4, u64(luts), u64(posts), 2, None, u64(out)) == -1  # null buffer
        assert call(eng, 1 << 31, luts, posts, 2, None, out) == -1    # rows > 0x7FFFFFFF
        assert call(eng, 0, luts, posts, 2, None, out) == 0           # rows == 0
        assert np.all(out == SENTINEL)
        assert L.tfhe_hip_csprng_rows(eng._h, u64(seeds), 4, (1 << 60) - 3, 4, u64(out)) == -1   # past 2^60
        assert L.tfhe_hip_csprng_rows(eng._h, u64(seeds), 4, 0, 0, u64(out)) == -1
        assert L.tfhe_hip_csprng_rows(eng._h, u64(seeds), 0, 0, 4, u64(out)) == 0
        assert np.all(out == SENTINEL)
        assert call(eng, 4, luts, posts, 2, np.array([0, 1, 1, 0], dtype=np.uint32), out) == 0   # and then it works
        assert not np.any(out == SENTINEL)
