"""Oblivious pseudo-random ciphertexts (fhEVM rand / randBounded) on the CPU: the host LUT against the numpy formula,
the block seeds against the AES definition, the oracle route against the predicted value on every row, uniformity
of the prediction at the real dimensions, and the radix / integer layers on a cleartext double of Engine.oprf."""
import ctypes

import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import integer as I
from tfhe_amd import radix as R
import oprf_ref as F


# ---- the LUT ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1024, 2048))
@pytest.mark.parametrize("rb,fb", F.PAIRS)
def test_lut_oprf_matches_formula(N, rb, fb):
    lut, post = tfhe_amd.lut_oprf(N, rb, fb)
    want, want_post = F.lut_oprf(N, rb, fb)
    assert np.array_equal(lut, want) and post == want_post


@pytest.mark.parametrize("N,rb,fb", [(2048, 0, 5), (2048, 5, 5), (2048, 6, 5), (8, 5, 6), (2048, 2, 64)])
def test_lut_oprf_refusals(N, rb, fb):
    lut = np.full(N, 7, dtype=np.uint64)
    post = ctypes.c_uint64(7)
    rc = tfhe_amd.lib().tfhe_hip_lut_oprf(N, rb, fb, tfhe_amd._u64(lut), ctypes.byref(post))
    assert rc == -1 and np.all(lut == 7) and post.value == 7          # EINVAL, outputs untouched
    with pytest.raises(tfhe_amd.TfheError):
        tfhe_amd.lut_oprf(N, rb, fb)


# ---- block seeds ----------------------------------------------------------------------------------------------
def test_block_seeds_are_consecutive_stream_words():
    parent = (0xFEDCBA9876543210, 0x0123456789ABCDEF)
    got = tfhe_amd.oprf_block_seeds(parent, 9)
    assert got.shape == (9, 2) and got.dtype == np.uint64
    assert np.array_equal(got, F.aes_stream_words(parent, 18).reshape(9, 2))     # from the AES definition
    assert np.array_equal(got, F.block_seeds(parent, 9))
    assert np.array_equal(tfhe_amd.oprf_block_seeds(parent, 3), got[:3])         # a prefix of the same stream
    assert not np.array_equal(tfhe_amd.oprf_block_seeds((parent[0], parent[1] ^ 1), 9), got)


# ---- the oracle route decrypts to the prediction ----------------------------------------------------------------
@pytest.mark.parametrize("preset", (3, 2))
@pytest.mark.parametrize("rb,fb", F.PAIRS)
def test_oracle_route_decrypts_to_prediction(preset, rb, fb):
    n, rows = 24, 96
    dprm, keys = F.small_keys(preset, n)
    masks = F.masks_of(F.block_seeds(F.PARENT, rows), n)
    lut, post = F.lut_oprf(dprm.N, rb, fb)
    out = F.oracle_rows(dprm, keys, masks, lut[None], [post], None)
    v, err = F.decode(F.out_phase(dprm, keys, out), fb)
    want = F.predict(masks, keys.lwe_key, dprm.N, rb)
    print(f"preset {preset} ({rb}, {fb}): worst phase error 2^{np.log2(max(int(err.max()), 1)):.1f}, "
          f"half step 2^{63 - fb}")
    assert int(err.max()) < 1 << (63 - fb)
    assert np.array_equal(v, want)
    assert want.min() >= 0 and want.max() < 1 << rb


def test_oracle_route_gate_bits():
    n, rows = 24, 96
    dprm, keys = F.small_keys(2, n)
    masks = F.masks_of(F.block_seeds(F.PARENT, rows), n)
    out = F.oracle_rows(dprm, keys, masks, tfhe_amd.lut_constant(dprm.N, tfhe_amd.MU)[None], [0], None)
    assert np.array_equal(tfhe_amd.decode_bool(F.out_phase(dprm, keys, out)), F.predict_gate(masks, keys.lwe_key, dprm.N))


# ---- uniformity at the real dimensions ----------------------------------------------------------------------------
@pytest.mark.parametrize("preset", (tfhe_amd.PRESET_FHEVM_FFT, tfhe_amd.PRESET_GATE_FFT))
def test_prediction_is_uniform(preset):
    p = tfhe_amd.Params.preset(preset)
    ck, _ = tfhe_amd.gen_keys(p, F.KEY_SEED, with_server_key=False)
    rows = 4096
    masks = F.masks_of(F.block_seeds(F.PARENT, rows), p.n)
    for rb, q999 in ((1, 10.83), (2, 16.27), (4, 37.70)):
        v = F.predict(masks, ck.lwe_key, p.N, rb)
        counts = np.bincount(v, minlength=1 << rb)
        assert counts.shape[0] == 1 << rb
        e = rows / (1 << rb)
        chi2 = float(((counts - e) ** 2 / e).sum())
        print(f"preset {preset} random_bits {rb}: chi2 = {chi2:.2f} (99.9 % quantile {q999})")
        assert chi2 < q999


# ---- radix and integer layers on the cleartext double -------------------------------------------------------------
class ClearKey:
    def decrypt(self, cts, mm):
        return (np.asarray(cts)[..., -1] // np.uint64(R.DELTA)) % np.uint64(mm)

    def decrypt_bool(self, cts):
        b = np.asarray(cts, dtype=np.uint64)[..., -1]
        return (b != 0) & (b < np.uint64(1 << 63))


class ClearRadixCircuit(R.RadixCircuit):
    """Trivial blocks: OPRF rows from the cleartext double, tables evaluated on the body."""

    def __init__(self):
        super().__init__(F.ClearOprfEngine(n=918, N=2048, order=1, dim=3))
        self.dim = 3

    def _pbs(self, flat, tables, idx):
        assert not flat[:, :-1].any() and np.all(flat[:, -1] % np.uint64(R.DELTA) == 0)
        v = (flat[:, -1] // np.uint64(R.DELTA)).astype(np.int64)
        assert v.max(initial=0) < R.SPACE
        return self.trivial(np.array([tables[i][x] for i, x in zip(idx, v)], dtype=np.uint64))


SEEDS = np.array([[0x0F2F0002, 0], [0x0F2F0002, 1], [0xFFFFFFFFFFFFFFFF, 0x8000000000000000]], dtype=np.uint64)


def radix_expect(eng, seeds, w, t):
    """value of each request: blocks of 2 bits (then 1 if t is odd) from consecutive block seeds"""
    bits = [2] * (t // 2) + [1] * (t % 2)
    vals = []
    for s in seeds:
        masks = F.masks_of(F.block_seeds(s, len(bits)), eng.params.n)
        v = 0
        for j, rb in enumerate(bits):
            v |= int(F.predict(masks[j:j + 1], eng.lwe_key, eng.params.N, rb)[0]) << (2 * j)
        vals.append(v)
    return vals


@pytest.mark.parametrize("w", (8, 16, 256))
def test_radix_rand(w):
    c = ClearRadixCircuit()
    x = R.RadixUint.rand(c, SEEDS, w)
    assert x.blocks.shape == (3, w // 2, c.dim) and x.width == w
    want = radix_expect(c.engine, SEEDS, w, w)
    assert [int(v) for v in x.decrypt(ClearKey())] == want
    assert c.pbs_count == 3 * (w // 2) and c.launches == 1 and c.engine.calls == [3 * (w // 2)]
    assert len(set(want)) == 3
    one = c.run(R.fhevm_rand(c, "rand", (int(SEEDS[1, 0]), int(SEEDS[1, 1])), w))   # one (lo, hi) pair
    assert int(one.decrypt(ClearKey())[0]) == want[1]


def test_radix_rand_bool():
    c = ClearRadixCircuit()
    b = c.run(R.fhevm_rand(c, "rand", SEEDS, 1))
    assert b.shape == (3, c.dim)
    masks = np.concatenate([F.masks_of(F.block_seeds(s, 1), 918) for s in SEEDS])
    assert np.array_equal(ClearKey().decrypt(b, 2).astype(np.int64), F.predict(masks, c.engine.lwe_key, 2048, 1))
    assert c.pbs_count == 3


@pytest.mark.parametrize("t", (1, 3, 8))
def test_radix_rand_bounded(t):
    c = ClearRadixCircuit()
    x = R.RadixUint.rand_bounded(c, SEEDS, 8, 1 << t)
    assert x.blocks.shape == (3, 4, c.dim)
    nr = (t + 1) // 2
    assert not x.blocks[:, nr:].any()                                  # untouched high blocks: trivial zero
    got = [int(v) for v in x.decrypt(ClearKey())]
    assert got == radix_expect(c.engine, SEEDS, 8, t) and max(got) < 1 << t
    assert c.pbs_count == 3 * nr                                       # block seeds for the random blocks only
    y = c.run(R.fhevm_rand(c, "randBounded", SEEDS, 8, 1 << t))
    assert np.array_equal(y.blocks, x.blocks)


@pytest.mark.parametrize("bound", (0, 1, 3, 6, 100, 512))
def test_radix_rand_bounded_refuses(bound):
    c = ClearRadixCircuit()
    with pytest.raises(ValueError):
        R.RadixUint.rand_bounded(c, SEEDS, 8, bound)
    assert c.pbs_count == 0


def test_radix_rand_ops_table():
    assert R.RADIX_RAND_OPS == ("rand", "randBounded")
    assert not set(R.RADIX_RAND_OPS) & set(R.RADIX_OPS)
    c = ClearRadixCircuit()
    with pytest.raises(ValueError):
        c.run(R.fhevm_rand(c, "add", SEEDS, 8))
    with pytest.raises(ValueError):
        c.run(R.fhevm_rand(c, "randBounded", SEEDS, 8))
    with pytest.raises(ValueError):
        c.run(R.fhevm_op(c, "rand", R.RadixUint.trivial(c, [1], 8), 1))


def test_radix_rand_plus_one():
    c = ClearRadixCircuit()
    x = R.RadixUint.rand(c, SEEDS, 8)
    y = c.run(R.fhevm_op(c, "add", x, 1))
    want = [(v + 1) % 256 for v in radix_expect(c.engine, SEEDS, 8, 8)]
    assert [int(v) for v in y.decrypt(ClearKey())] == want


class ClearGateEngine(F.ClearOprfEngine):
    """The gate double of tests/test_integer.py (sign of the body) plus the cleartext OPRF."""

    def __init__(self):
        super().__init__(n=630, N=1024, order=0, dim=631)

    def pbs(self, cts, lut):
        cts = np.asarray(cts, dtype=np.uint64)
        assert not cts[:, :-1].any()
        body = cts[:, -1]
        out = np.zeros_like(cts)
        out[:, -1] = np.where((body != 0) & (body < np.uint64(1 << 63)), np.uint64(tfhe_amd.MU),
                              np.uint64(F.M64 - tfhe_amd.MU))
        return out


def integer_expect(eng, seeds, t):
    vals = []
    for s in seeds:
        masks = F.masks_of(F.block_seeds(s, t), eng.params.n)
        bits = F.predict_gate(masks, eng.lwe_key, eng.params.N)
        vals.append(sum(1 << j for j in range(t) if bits[j]))
    return vals


@pytest.mark.parametrize("w", (8, 16, 256))
def test_integer_rand(w):
    eng = ClearGateEngine()
    c = I.Circuit(eng)
    x = I.FheUint.rand(c, SEEDS, w)
    assert x.bits.shape == (3, w, 631)
    assert [int(v) for v in x.decrypt(ClearKey())] == integer_expect(eng, SEEDS, w)
    assert c.pbs_count == 3 * w and c.launches == 1


@pytest.mark.parametrize("t", (1, 3, 8))
def test_integer_rand_bounded(t):
    eng = ClearGateEngine()
    c = I.Circuit(eng)
    x = I.FheUint.rand_bounded(c, SEEDS, 8, 1 << t)
    assert x.bits.shape == (3, 8, 631)
    assert np.array_equal(x.bits[:, t:], c.trivial(np.zeros((3, 8 - t), dtype=bool)))   # the rest trivial false
    got = [int(v) for v in x.decrypt(ClearKey())]
    assert got == integer_expect(eng, SEEDS, t) and max(got) < 1 << t
    with pytest.raises(ValueError):
        I.FheUint.rand_bounded(c, SEEDS, 8, 12)
    with pytest.raises(ValueError):
        I.FheUint.rand_bounded(c, SEEDS, 8, 512)


def test_integer_rand_plus_one_and_device_form():
    import torch
    eng = ClearGateEngine()
    c = I.Circuit(eng)
    x = I.FheUint.rand(c, SEEDS, 8)
    y = c.run(I.fhevm_op(c, "add", x, 1))
    assert [int(v) for v in y.decrypt(ClearKey())] == [(v + 1) % 256 for v in integer_expect(eng, SEEDS, 8)]

    class TorchEngine(ClearGateEngine):                                  # oprf_device on torch CPU tensors
        def oprf_device(self, d_seeds, d_luts, d_post, d_lut_index=None):
            out = self.oprf(d_seeds.numpy().view(np.uint64), d_luts.numpy().view(np.uint64),
                            d_post.numpy().view(np.uint64))
            return torch.from_numpy(out.view(np.int64))

    cd = I.Circuit(TorchEngine(), device="cpu")
    xd = I.FheUint.rand_bounded(cd, SEEDS, 8, 8)
    assert isinstance(xd.bits, torch.Tensor)
    assert np.array_equal(xd.bits.numpy().view(np.uint64), I.FheUint.rand_bounded(c, SEEDS, 8, 8).bits)
