"""Compression of squashed ciphertexts on the MI355X (tfhe_amd/csrc/sns_pks.hip, sns_pks_api.cpp): the device
packing keyswitch over the 2^128 torus against the Python restatement of the rule (tests/sns_pks_ref.py; the same
inputs and references as the CPU tests), against the CPU pack at the preset's GLWE shape, across chunk and tile
edges, on caller streams, and chained behind the noise squashing with the squashed LWEs staying on the device."""
import ctypes

import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import sns as S
from tfhe_amd import sns_compression as SC

import sns_inputs as I
import sns_pks_ref as R
from conftest import KEY_SEED

pytestmark = pytest.mark.gpu

SETS = ("A", "B", "C")
CASES = [(n, c) for n in SETS for c in R.counts(R.make_params(n))] + [("B", 70)]   # 70: the 64-row tile edge


@pytest.fixture(scope="module")
def packers():
    made = {}

    def get(name):
        if name not in made:
            pp, key = R.keys(name)
            made[name] = SC.SquashedPacker(pp, 0).load_key(key)
        return made[name]

    yield get
    for p in made.values():
        p.close()


def same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(1))[0]
        pytest.fail(f"{what}: {bad.size} of {got.shape[0]} GLWEs differ, first {bad[:8]}")


@pytest.mark.parametrize("name,count", CASES)
def test_pack_equals_reference(packers, name, count):
    """Uniform words and the special rows (mask all 0, all 2^127, all ones, all the rounding tie) at counts 1,
    lpg - 1, lpg, lpg + 1, 2 lpg + 5; on set B also 70, where the GEMM's 64-row tile ends inside group 3."""
    for i, (lwes, ref) in enumerate(R.case(name, count)):
        same(packers(name).pack(lwes), ref, f"set {name}, count {count}, input {i}")


@pytest.fixture(scope="module")
def set_d():
    pp, key = R.keys("D")
    packer = SC.SquashedPacker(pp, 0).load_key(key)
    yield pp, key, packer
    packer.close()


@pytest.mark.parametrize("count", [5, 131])
def test_preset_glwe_shape_equals_host_and_decrypts(set_d, count):
    """Set D (k = 6, N = 1024, 128 per GLWE, 2^61 x 1): 112 column tiles, two full row tiles and a ragged one."""
    pp, key, packer = set_d
    msgs = (np.arange(count) * 7 + 1) % 16
    lwes = R.encrypt(pp, key.in_key, msgs, seed=count)
    got = packer.pack(lwes)
    same(got, SC.pack_host(pp, key.pksk, lwes), f"set D, count {count}")
    lpg, delta = pp.lwe_per_glwe, (1 << 127) // 16
    for g in range(got.shape[0]):
        m = msgs[g * lpg:(g + 1) * lpg]
        bound = R.error_bound(pp, len(m))
        assert bound < delta / 2
        ph = SC.glwe_phase128(pp.out_k, pp.out_N, key.post_packing_key, got[g])
        assert max(abs(R.centered(ph[i] - delta * int(x))) for i, x in enumerate(m)) < bound
    comp = [SC.compress_glwe(pp, got[g], min(lpg, count - g * lpg)) for g in range(got.shape[0])]
    assert np.array_equal(SC.decrypt_list(key, comp, 16), msgs)
    assert [c.bodies for c in comp] == ([5] if count == 5 else [128, 3])


def test_chunks_of_one_group(packers, monkeypatch):
    """TFHE_HIP_SNS_PKS_CHUNK = 1 (read at create): 3 lpg + 7 LWEs run as three full chunks and a ragged fourth
    through one-group workspaces; the result equals the unchunked context's and the CPU pack."""
    pp, key = R.keys("A")
    count = 3 * pp.lwe_per_glwe + 7
    lwes = R.inputs(pp, count, seed=31)[0]
    whole = packers("A").pack(lwes)
    monkeypatch.setenv("TFHE_HIP_SNS_PKS_CHUNK", "1")
    chunked = SC.SquashedPacker(pp, 0).load_key(key)
    monkeypatch.delenv("TFHE_HIP_SNS_PKS_CHUNK")
    try:
        got = chunked.pack(lwes)
        same(got, whole, "chunked against unchunked")
        same(got, SC.pack_host(pp, key.pksk, lwes), "chunked against the CPU pack")
        same(chunked.pack(lwes[-5:]), SC.pack_host(pp, key.pksk, lwes[-5:]), "a smaller call on the same context")
    finally:
        chunked.close()


SENTINEL = 0x5E5E5E5E5E5E5E5E


def test_pack_async_on_torchs_current_stream(packers):
    import torch
    pp, _ = R.keys("B")
    packer = packers("B")
    lwes, ref = R.case("B", 2 * pp.lwe_per_glwe + 5)[0]
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(lwes.view(np.int64).copy()).to(dev)
    d_out = torch.full((ref.shape[0] + 1,) + pp.glwe_shape, SENTINEL, dtype=torch.int64, device=dev)
    packer.pack_async(d_in, lwes.shape[0], d_out)            # torch's current (default) stream
    out = d_out.cpu().numpy().view(np.uint64)
    same(out[:-1], packer.pack(lwes), "pack_async against pack")
    same(out[:-1], ref, "pack_async against the reference")
    assert (out[-1] == SENTINEL).all()                       # nothing past groups * glwe_len


def test_pack_async_two_streams(packers):
    """Two calls on different streams, back to back, sharing the context's workspaces: inputs are the last 25 and
    the last 45 rows of one pool (the pointers are not allocation bases and the inputs end where the pool ends);
    outputs go into sentinel-filled buffers with room to spare."""
    import torch
    pp, key = R.keys("B")
    packer = packers("B")
    pool = R.inputs(pp, 45, seed=0x2575)[0]
    dev = torch.device("cuda", 0)
    d_pool = torch.from_numpy(pool.view(np.int64)).to(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    outs = []
    for st, cnt in ((s1, 25), (s2, 45)):
        groups = -(-cnt // pp.lwe_per_glwe)
        d_out = torch.full((groups + 2,) + pp.glwe_shape, SENTINEL, dtype=torch.int64, device=dev)
        st.wait_stream(torch.cuda.current_stream(dev))       # the pool's upload and the sentinel fill
        packer.pack_async(d_pool[-cnt:], cnt, d_out, st)
        outs.append((st, cnt, groups, d_out))
    for st, cnt, groups, d_out in outs:
        st.synchronize()
        out = d_out.cpu().numpy().view(np.uint64)
        same(out[:groups], SC.pack_host(pp, key.pksk, pool[-cnt:]), f"stream call of {cnt}")
        assert (out[groups:] == SENTINEL).all()


def test_no_key_and_empty_calls():
    import torch
    pp, key = R.keys("A")
    packer = SC.SquashedPacker(pp, 0)
    try:
        lwes = R.inputs(pp, 5)[0]
        with pytest.raises(tfhe_amd.TfheError) as e:
            packer.pack(lwes)
        assert e.value.code == -4                                        # ENOKEYS
        d = torch.zeros(lwes.size, dtype=torch.int64, device="cuda:0")
        d_out = torch.full((pp.glwe_len,), SENTINEL, dtype=torch.int64, device="cuda:0")
        with pytest.raises(tfhe_amd.TfheError) as e:
            packer.pack_async(d, 5, d_out)
        assert e.value.code == -4
        with pytest.raises(tfhe_amd.TfheError) as e:
            packer.load_key(type("K", (), {"pksk": key.pksk[:-1]}))       # wrong length
        assert e.value.code == -1
        packer.load_key(key)
        assert packer.pack(lwes[:0]).shape == (0,) + pp.glwe_shape       # count == 0: OK
        L = SC._lib()
        assert L.tfhe_hip_sns_pks_pack(packer._h, None, 0, None) == 0
        assert L.tfhe_hip_sns_pks_pack_async(packer._h, None, 0, None, None) == 0
        assert L.tfhe_hip_sns_pks_pack(packer._h, None, 1, None) == -1
        assert L.tfhe_hip_sns_pks_pack_async(packer._h, ctypes.c_void_p(d.data_ptr()), 0x80000000,
                                             ctypes.c_void_p(d_out.data_ptr()), None) == -1
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy().view(np.uint64) == SENTINEL).all()   # the refused calls wrote nothing
        same(packer.pack(lwes), SC.pack_host(pp, key.pksk, lwes), "after the refused calls")
    finally:
        packer.close()


def test_squash_and_compress_chain(oracle_mod):
    """P-FHEVM ciphertexts at a small key dimension (n = 7: the engine's shape leaves n free) through keyswitch,
    MS reduction, the 128-bit bootstrap and the packing keyswitch (in_dim 4096 = the squashing key's k N, out k = 1,
    N = 256, 2^61 x 1, 32 per GLWE): every message decrypts from the stored list, and the list is bit-equal to
    packing the host-downloaded squash output."""
    n, count = 7, 40
    sp, _, skey, _ = I.small_keys(oracle_mod, n, KEY_SEED + n)
    prm = tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM)
    prm.n = n
    glwe_key = np.random.default_rng(0x61E).integers(0, 2, prm.k * prm.N).astype(np.uint64)
    ck = tfhe_amd.ClientKey(prm, None, skey.lwe_key, glwe_key)
    sk = tfhe_amd.server_keygen(ck, KEY_SEED)
    pp = SC.SnsPksParams(sp.out_dim, 1, 256, 61, 1, 32, 128, R.NOISE_LOG2)
    assert pp.in_dim == 4096
    pkey = SC.SquashedCompressionKey(pp, R.SEED, skey.glwe_key)
    msgs = (np.arange(count) * 3 + 2) % 16
    cts = ck.encrypt(msgs, 16, seed=0xC0FFEE81)
    eng = tfhe_amd.Engine(prm, 0).load_keys(sk)
    sq = S.Squasher(sp, 0).load_key(skey)
    packer = SC.SquashedPacker(pp, 0).load_key(pkey)
    try:
        comp = SC.squash_and_compress(eng, sq, packer, cts)
        assert [c.bodies for c in comp] == [32, 8]
        assert np.array_equal(SC.decrypt_list(pkey, comp, 16), msgs)
        small, _ = eng.ms_reduce(eng.keyswitch(cts))
        squashed = sq.squash(small)
        assert np.array_equal(skey.decrypt(squashed), msgs)
        want = packer.compress_squashed_into_list(squashed)
        assert len(want) == len(comp)
        for a, b in zip(comp, want):
            assert a.bodies == b.bodies and np.array_equal(a.packed, b.packed)
        assert sum(c.nbytes for c in comp) * 50 < squashed.nbytes         # 64 KB per LWE -> ~16 B + the shared mask
    finally:
        packer.close()
        sq.close()
        eng.close()
