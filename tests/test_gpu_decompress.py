"""Decompression on the MI355X against the oracle composition of tests/test_decompress.py, every comparison an
integer equality: the unpack / extract kernel (decompress.hip) over a shape sweep, the blind rotation at LWE
dimensions away from the presets on a rotation-only engine (tfhe_hip_load_bsk), the whole path
(Decompressor.decompress / decompress_device) word for word and by decryption, and the ABI contract."""
import ctypes

import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import compression as C
import guard_rows as G
import test_decompress as T

pytestmark = pytest.mark.gpu


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(torch.device("cuda", 0))


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


# ---- 1. unpack / extract sweep ---------------------------------------------------------------------------------
# (out_k, out_N, lwe_per_glwe, storage_log, counts); the last one is the ML2048 preset's 1 x 2048 x 2048
def _counts(lpg):
    return (1, lpg - 1, lpg, lpg + 1, 2 * lpg + 3)


SWEEP = [(1, 32, 32, 1, _counts(32)), (1, 64, 64, 12, _counts(64)), (3, 32, 17, 26, _counts(17)),
         (1, 64, 5, 63, _counts(5)), (1, 64, 64, 32, _counts(64)), (1, 4096, 3, 26, _counts(3)),
         (1, 2048, 2048, 26, (1, 2048 + 3))]


@pytest.mark.parametrize("k,N,lpg,w,counts", SWEEP, ids=lambda v: str(v) if isinstance(v, int) else "c")
def test_unpack_extract_sweep(oracle_mod, k, N, lpg, w, counts):
    O = oracle_mod
    fields = (64, k, N, 4, 3, lpg, w, -48) if N != 2048 else (2048, 1, 2048, 14, 2, 2048, 26, -48)
    pp, opp = C.PksParams(*fields), O.PksParams(*fields)
    if N == 2048:
        preset = C.PksParams.preset(C.PKS_PRESET_ML2048)
        assert bytes(pp) == bytes(preset)
    packer = C.Packer(pp, 0)
    degrees = set()
    try:
        for count in counts:
            rng = np.random.default_rng(1000 * N + 10 * w + count)
            words = T.list_words(O, opp, count)
            packed = rng.integers(0, 2 ** 64, size=words, dtype=np.uint64)  # spare bits of the last words included
            ref = T.unpack_extract_ref(O, opp, packed, count)
            ref = np.stack([ref[q] for q in range(count)])
            degrees |= {q % lpg for q in range(count)}
            comp = [C.CompressedGlwe(pp, p, b) for p, b in T.split_list(O, opp, packed, count)]
            got = packer.unpack_extract(comp)
            assert got.shape == ref.shape
            assert np.array_equal(got, ref), f"host form, count {count}: rows {np.nonzero((got != ref).any(1))[0][:8]}"
            whole, d_out = G.guarded(count, ref.shape[1])
            packer.unpack_extract_async(to_dev(packed), count, d_out)
            got = to_host(d_out)
            assert np.array_equal(got, ref), f"async form, count {count}: rows {np.nonzero((got != ref).any(1))[0][:8]}"
            G.assert_guards(whole, count, f"unpack_extract_async, {k} x {N}, {lpg} per GLWE, count {count}")
    finally:
        packer.close()
    # degree 0 (every j > 0 negated) in every shape; degree N - 1 (nothing negated) wherever a group is full
    assert 0 in degrees
    assert (N - 1 in degrees) == (lpg == N)


def test_sweep_holds_both_sign_extremes():
    assert sum(lpg == N and max(counts) >= lpg for _, N, lpg, _, counts in SWEEP) >= 3


# ---- 2. rotation away from the preset n --------------------------------------------------------------------
ROTATION = [(3, 1, 6), (3, 2, 6), (3, 3, 6), (3, 64, 6),   # FFT64, N = 2048: odd and even trip counts
            (2, 1, 6), (2, 64, 6), (2, 1026, 2),          # FFT64, N = 1024; 1026 is past the latency kernel's staging
            (0, 64, 6)]                                   # NTT, N = 1024


def rotation_inputs(N, n, B, seed):
    """Masks holding 0, 2^64 - 1 and the modulus-switch rounding ties (the half-steps of the switch to 2N, from
    both sides and as negative values) among random values; 4-bit messages at 2^59 in the bodies."""
    rng = np.random.default_rng(seed)
    sh = 64 - (int(2 * N).bit_length() - 1) - 1  # bit below the kept ones: 2^sh is a rounding tie
    special = np.array([0, 2 ** 64 - 1, (1 << sh) - 1, 1 << sh, 2 ** 64 - (1 << sh), (1 << sh) + 1, 3 << sh],
                       dtype=np.uint64)
    cts = rng.integers(0, 2 ** 64, size=(B, n + 1), dtype=np.uint64)
    for q in range(B):
        for i in range(0, n, 2):
            cts[q, i] = special[(q + i // 2) % special.size]
    cts[:, n] = rng.integers(0, 16, B).astype(np.uint64) << np.uint64(59)
    return cts


@pytest.mark.parametrize("preset,n,B", ROTATION, ids=lambda v: str(v))
def test_rotation_off_preset_n(oracle_mod, preset, n, B):
    """Engine.bootstrap and blind_rotate after load_bsk alone, on the latency and the batch kernel."""
    O = oracle_mod
    prm = O.params(preset)
    dprm = T.with_n(prm, n)
    glwe_key = O.Keys(prm, T.SEED, with_bsk=False, with_ksk=False).glwe_key
    lwe_key = np.random.default_rng(n).integers(0, 2, n).astype(np.uint64)
    keys = T.rotation_keys(O, dprm, T.DK_SEED, lwe_key, glwe_key)
    cts = rotation_inputs(prm.N, n, B, 77 + n)
    lut = O.lut_from_table(prm.N, 16, [(5 * m + 3) % 16 for m in range(16)], 1 << 59)
    ref = [T.bootstrap_ref(O, dprm, keys, cts[q], lut) for q in range(B)]
    ref_acc, ref_out = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    params = T.with_n(tfhe_amd.Params.preset(preset), n)
    with tfhe_amd.Engine(params, 0) as eng:
        eng.load_bsk(keys.bsk)
        for lat in (1 << 20, 0):
            eng.set_latency_batch(lat)
            kernel = eng.br_kernel(B)
            out = eng.bootstrap(cts, lut)
            assert np.array_equal(out, ref_out), f"bootstrap on {kernel}: rows {np.nonzero((out != ref_out).any(1))[0]}"
            acc = eng.blind_rotate(cts, lut)
            assert np.array_equal(acc, ref_acc), f"blind_rotate on {kernel}"


# ---- 3. end to end ---------------------------------------------------------------------------------------------
def product_side(cs):
    cp = tfhe_amd.Params.preset(cs.preset)
    dk = C.DecompressionKey(cp, cs.pp, cs.pk.out_key, cs.glwe_key, T.DK_SEED)
    comp = [C.CompressedGlwe(cs.pp, p, b) for p, b in cs.groups]
    return dk, comp


SMALLEST_E2E = min(T.E2E_SHAPES, key=lambda s: (s[5], tfhe_amd.Params.preset(s[0]).N))  # fewest rows, then the shorter


@pytest.mark.parametrize("shape", T.E2E_SHAPES, ids=lambda s: "p%d-%dx%d-%d-%d" % s[:5])
def test_decompress_end_to_end(shape, oracle_mod, request):
    O = oracle_mod
    cs = T.case(*shape)
    dk, comp = product_side(cs)
    rows = range(cs.count)
    ref = cs.reference(rows)
    ref = np.stack([ref[q] for q in rows])
    N = cs.prm.N
    other = O.lut_from_table(N, 16, [(7 * m + 2) % 16 for m in range(16)], 1 << 59)
    with C.Decompressor(dk, 0) as dec:
        out = dec.decompress(comp)
        assert np.array_equal(out, ref), f"rows {np.nonzero((out != ref).any(1))[0][:8]}"
        assert np.array_equal(T.decode(cs.phases(out)), cs.msgs)
        d_lut = to_dev(T.identity_lut(O, N))
        assert np.array_equal(to_host(dec.decompress_device(to_dev(cs.packed), cs.count, d_lut)), ref)
        if shape == SMALLEST_E2E:  # the rotation's write-big epilogue behind the unpack kernel, between guard rows
            whole, d_out = G.guarded(cs.count, ref.shape[1])
            dec.decompress_async(to_dev(cs.packed), cs.count, d_lut, d_out)
            assert np.array_equal(to_host(d_out), ref)
            G.assert_guards(whole, cs.count, "decompress_async, shape %s" % (shape,))
        # a non-identity LUT on the odd rows, through lut_index
        idx = (np.arange(cs.count) % 2).astype(np.uint32)
        odd = [q for q in rows if q % 2]
        ref2 = ref.copy()
        r = cs.reference(odd, other)
        for q in odd:
            ref2[q] = r[q]
        out2 = dec.decompress(comp, lut=np.stack([T.identity_lut(O, N), other]), lut_index=idx)
        assert np.array_equal(out2, ref2)
        assert np.array_equal(T.decode(cs.phases(out2)), np.where(idx == 1, (7 * cs.msgs + 2) % 16, cs.msgs))
    if shape[0] == 2:  # P-GATE: back to the small key on a full compute engine
        ck, _ = request.getfixturevalue("gate_fft_keys")
        assert np.array_equal(ck.glwe_key, cs.glwe_key)
        small = request.getfixturevalue("gate_fft_engine").keyswitch(out)
        assert np.array_equal(T.decode(ck.phase(small, key=ck.lwe_key)), cs.msgs)


def test_decompress_wide_shape(oracle_mod):
    """4 x 256 (a tfhe-rs-like post-packing GLWE) into P-FHEVM-FFT, n = 1024, 259 ciphertexts."""
    cs = T.case(*T.WIDE_SHAPE)
    dk, comp = product_side(cs)
    ref = cs.reference(T.WIDE_ROWS)
    with C.Decompressor(dk, 0) as dec:
        out = dec.decompress(comp)
    for q in T.WIDE_ROWS:
        assert np.array_equal(out[q], ref[q]), q
    assert np.array_equal(T.decode(cs.phases(out)), cs.msgs)


# ---- 4. contract ---------------------------------------------------------------------------------------------
def code(f):
    with pytest.raises(tfhe_amd.TfheError) as e:
        f()
    return e.value.code


def raw_decompress(eng, pp, packed, count, luts, words=None):
    out = np.zeros((count, eng.params.k * eng.params.N + 1), dtype=np.uint64)
    luts = np.ascontiguousarray(luts, dtype=np.uint64).reshape(-1, eng.params.N)
    u = ctypes.POINTER(ctypes.c_uint64)
    tfhe_amd._check(C._lib().tfhe_hip_decompress(eng._h, ctypes.byref(pp), packed.ctypes.data_as(u),
                                                 packed.size if words is None else words, count,
                                                 luts.ctypes.data_as(u), luts.shape[0], None, out.ctypes.data_as(u)))
    return out


def test_contract(oracle_mod):
    O = oracle_mod
    cs = T.case(*T.E2E_SHAPES[2])  # P-GATE-FFT, 1 x 64
    dparams = T.with_n(tfhe_amd.Params.preset(2), 64)
    ck, sk = tfhe_amd.gen_keys(dparams, T.SEED)  # a full key set at n = 64 (its own small key)
    okeys = O.Keys(cs.dprm, T.SEED)
    lut = T.identity_lut(O, 1024)
    cts = ck.encrypt_torus(np.arange(9, dtype=np.uint64) << np.uint64(59), seed=5)
    with tfhe_amd.Engine(dparams, 0) as eng:
        # nothing loaded
        assert code(lambda: raw_decompress(eng, cs.pp, cs.packed, cs.count, lut)) == -4
        assert code(lambda: eng.bootstrap(cts, lut)) == -4
        assert code(lambda: eng.blind_rotate(cts, lut)) == -4
        # the BSK alone: rotation-only
        eng.load_bsk(sk.bsk)
        boot = eng.bootstrap(cts, lut)
        assert np.array_equal(boot, np.stack([T.bootstrap_ref(O, cs.dprm, okeys, c, lut)[1] for c in cts]))
        assert code(lambda: eng.pbs(cts, lut)) == -4
        assert code(lambda: eng.keyswitch(boot)) == -4
        assert code(lambda: eng.nand(cts, cts)) == -4
        # argument checks with a ctx: the dimension, the list size, the LUT index
        other = C.PksParams(1024, 3, 32, 4, 3, 17, 26, -48)  # out_k * out_N = 96 != 64
        ow = np.zeros(T.list_words(O, O.PksParams(1024, 3, 32, 4, 3, 17, 26, -48), 3), dtype=np.uint64)
        assert code(lambda: raw_decompress(eng, other, ow, 3, lut)) == -1
        assert "n = 64" in tfhe_amd.lib().tfhe_hip_last_error().decode()
        assert code(lambda: raw_decompress(eng, cs.pp, cs.packed, cs.count, lut, words=cs.packed.size - 1)) == -1
        # count = 0
        assert raw_decompress(eng, cs.pp, np.zeros(1, dtype=np.uint64), 0, lut, words=0).shape == (0, 1025)
        assert eng.bootstrap(cts[:0], lut).shape == (0, 1025)
        # the full key set completes the ctx; a later BSK-only load makes it rotation-only again
        eng.load_keys(sk)
        assert np.array_equal(eng.pbs(cts, lut), O.pbs_batch_fft(cs.dprm, okeys, cts, lut[None]))
        assert np.array_equal(eng.bootstrap(cts, lut), boot)
        eng.load_bsk(sk.bsk)
        assert code(lambda: eng.pbs(cts, lut)) == -4
        assert np.array_equal(eng.bootstrap(cts, lut), boot)
    # two shards on one device split the batch and give the single-shard words
    with tfhe_amd.Engine(dparams, [0, 0]) as eng2:
        eng2.load_bsk(sk.bsk)
        assert np.array_equal(eng2.bootstrap(cts, lut), boot)
        d = eng2.bootstrap_device(to_dev(cts), to_dev(lut))
        assert np.array_equal(to_host(d), boot)


def test_decompressor_contract(oracle_mod):
    """count = 0, lut_index length, and timing: one slot-3 and one slot-0 launch per decompress."""
    cs = T.case(*T.E2E_SHAPES[2])
    dk, comp = product_side(cs)
    with C.Decompressor(dk, 0) as dec:
        assert dec.decompress([]).shape == (0, 1025)
        assert dec.decompress_device(to_dev(np.zeros(1, dtype=np.uint64)), 0, to_dev(dec.identity_lut())).shape == (0, 1025)
        with pytest.raises(ValueError):
            dec.decompress(comp, lut_index=[0])
        assert code(lambda: dec.decompress(comp, lut_index=np.ones(cs.count, dtype=np.uint32))) == -1
        dec.engine.timing(True)
        dec.engine.timing_reset()
        dec.decompress(comp)
        dec.decompress(comp[:1])
        for slot in (3, 0):
            ms, launches = dec.engine.timing_stats(slot)
            assert launches == 2 and ms > 0, slot
        assert dec.engine.timing_stats(1)[1] == 0
        assert code(lambda: dec.engine.timing_stats(4)) == -1
        dec.engine.timing(False)


def test_unpack_extract_contract():
    pp = C.PksParams(64, 1, 64, 4, 3, 64, 12, -48)
    packer = C.Packer(pp, 0)
    try:
        assert packer.unpack_extract([]).shape == (0, 65)
        short = C.CompressedGlwe(pp, np.zeros(3, dtype=np.uint64), 5)  # 5 bodies take more than 3 words
        assert code(lambda: packer.unpack_extract([short])) == -1
    finally:
        packer.close()
    wide = C.Packer(C.PksParams(64, 1, 8192, 4, 3, 3, 26, -48), 0)
    try:
        w = C._lib().tfhe_hip_pks_packed_words(ctypes.byref(wide.params), 1)
        assert code(lambda: wide.unpack_extract([C.CompressedGlwe(wide.params, np.zeros(w, dtype=np.uint64), 1)])) == -5
    finally:
        wide.close()
