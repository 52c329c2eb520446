"""Compact-list expansion and casting on the MI355X (tfhe_amd/csrc/expand.hip, tfhe_hip_expand_compact*,
tfhe_hip_expand_cast*), every comparison an integer equality.  The reference of the expansion is ctlist.expand (numpy,
pinned against the reference's key pair by tests/test_ctlist.py); the reference of the full path is the host route
that existed before the device one, ctlist.expand + Engine.pbs / ctlist.cast_to_blocks."""
import ctypes

import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import ctlist
from tfhe_amd import radix as R
import guard_rows as G
import test_expand as E
from test_ctlist import _fixtures

pytestmark = pytest.mark.gpu


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(torch.device("cuda", 0))


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def idx_dev(idx):
    import torch
    return torch.from_numpy(np.ascontiguousarray(idx).astype(np.int32)).to(torch.device("cuda", 0))


def first_rows(got, ref):
    return np.nonzero((got != ref).any(1))[0][:8]


@pytest.fixture(scope="module")
def plain_engine():
    """The expansion needs no key: an engine with nothing loaded."""
    with tfhe_amd.Engine(tfhe_amd.Params.preset(tfhe_amd.PRESET_GATE_FFT), 0) as eng:
        yield eng


# ---- 1. expansion sweep ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,counts,reps", E.SWEEP, ids=lambda v: str(v) if isinstance(v, int) else "c")
def test_expand_sweep(plain_engine, N, counts, reps):
    eng = plain_engine
    degrees = set()
    for count in counts:
        cl = E.random_list(N, count, 1000 * N + count)
        ex = ctlist.expand(cl)
        words = ctlist.list_words(cl)
        d_words = to_dev(words)
        degrees |= {q % N for q in range(count)}
        for rep in reps:
            full = np.repeat(ex, rep, axis=0)
            for rows in (count * rep, count * rep - 1):
                ref = full[:rows]
                got = eng.expand_compact(words, N, count, rep, rows)
                assert got.shape == ref.shape
                assert np.array_equal(got, ref), f"host form, count {count} rep {rep} rows {rows}: rows {first_rows(got, ref)}"
                whole, d_out = G.guarded(rows, N + 1)  # rows = count * rep - 1: the kernel must stop one row early
                eng.expand_compact_async(d_words, N, count, d_out, rep, rows)
                got = to_host(d_out)
                assert np.array_equal(got, ref), f"async form, count {count} rep {rep} rows {rows}: rows {first_rows(got, ref)}"
                G.assert_guards(whole, rows, f"expand_compact_async, N {N} count {count} rep {rep} rows {rows}")
        got = to_host(eng.expand_compact_device(d_words, N, count))  # the defaults: rep 1, every row
        assert np.array_equal(got, ex), f"device form, count {count}: rows {first_rows(got, ex)}"
        assert np.array_equal(ctlist.expand_device(eng, cl), ex)
    # degree 0 (every k < N - 1 negated) in every shape; degree N - 1 (nothing negated) wherever a bin is full
    assert 0 in degrees
    assert (N - 1 in degrees) == (max(counts) >= N)


# ---- 2. the reference's own lists --------------------------------------------------------------------------------
def test_reference_fixtures_expand_on_the_device(plain_engine):
    fx = _fixtures()
    assert len(fx) == 4
    for name, data, _, _ in fx:
        cl = ctlist.load_compact_list(data)
        ex = ctlist.expand(cl)
        got = ctlist.expand_device(plain_engine, cl)
        assert got.shape == (cl.count, 2049), name
        assert np.array_equal(got, ex), f"{name}: rows {first_rows(got, ex)}"
        got2 = ctlist.expand_device(plain_engine, cl, rep=2, rows=cl.blocks)  # one row per radix block
        assert np.array_equal(got2, np.repeat(ex, 2, axis=0)[:cl.blocks]), name


# ---- 3. full path at a small shape: order 0 (rotation, then keyswitch), n = 64 -------------------------------------
def test_expand_cast_small_shape():
    cs = E.small_case()
    words = ctlist.list_words(cs.cl)
    ref_in = cs.reference_input()
    with tfhe_amd.Engine(cs.params, 0) as eng:
        eng.load_keys(cs.sk)
        kernels = set()
        for lat in (1 << 20, 0):
            eng.set_latency_batch(lat)
            kernel = eng.br_kernel(cs.rows)
            kernels.add(kernel)
            ref = eng.pbs(ref_in, cs.luts, cs.idx)
            got, err = cs.decode(ref)
            assert np.array_equal(got, cs.expected) and err < 1 << 60, f"the reference route on {kernel}"
            out = eng.expand_cast(words, cs.cl.count, cs.luts, cs.REP, lut_index=cs.idx)
            assert out.shape == ref.shape
            assert np.array_equal(out, ref), f"host form on {kernel}: rows {first_rows(out, ref)}"
            d = eng.expand_cast_device(to_dev(words), cs.cl.count, to_dev(cs.luts), cs.REP,
                                       d_lut_index=idx_dev(cs.idx))
            assert np.array_equal(to_host(d), ref), f"async form on {kernel}: rows {first_rows(to_host(d), ref)}"
            whole, d_out = G.guarded(cs.rows, ref.shape[1])
            d_words, d_luts, d_idx = to_dev(words), to_dev(cs.luts), idx_dev(cs.idx)
            eng.expand_cast_async(d_words, cs.cl.count, d_luts, d_out, cs.REP, d_lut_index=d_idx)
            assert np.array_equal(to_host(d_out), ref), f"guarded async form on {kernel}: rows {first_rows(to_host(d_out), ref)}"
            G.assert_guards(whole, cs.rows, f"expand_cast_async on {kernel}")
            # an odd block count, and one LUT for every row
            odd = eng.expand_cast(words, cs.cl.count, cs.luts, cs.REP, rows=cs.rows - 1, lut_index=cs.idx[:-1])
            assert np.array_equal(odd, ref[:-1])
            one = eng.expand_cast(words, cs.cl.count, cs.luts[1], 1)
            assert np.array_equal(one, eng.pbs(ctlist.expand(cs.cl), cs.luts[1]))
        assert len(kernels) == 2, kernels


# ---- 4. full path at P-FHEVM-FFT: order 1, casting KSK, MS noise reduction ------------------------------------------
@pytest.fixture(scope="module")
def cast_case(fhevm_fft_keys):
    """The list and keys of tests/test_gpu_ctlist.py: 43 packed LWEs, 85 radix blocks."""
    ck, _ = fhevm_fft_keys
    rng = np.random.default_rng(0xC0)
    pke_key = rng.integers(0, 2, 2048).astype(np.uint64)
    cpk = ctlist.gen_compact_public_key(pke_key, rng)
    vals = [1, 255, 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 12345678901234567890]
    kinds = [(ctlist.KIND_BOOLEAN, 1), (0, 4), (0, 16), (0, 32), (0, 32)]
    cl = ctlist.encrypt_compact(cpk, ctlist.pack_blocks(ctlist.value_blocks(vals, kinds)), kinds, rng)
    assert (cl.count, cl.blocks) == (43, 85)
    with tfhe_amd.Engine(ck.params, 0) as cast:
        cast.load_keys(ctlist.casting_keys(ck, pke_key, seed=0x5EED))
        yield ck, cl, vals, kinds, cast


def test_cast_list_to_blocks_fhevm(cast_case):
    ck, cl, vals, kinds, cast = cast_case
    ref = ctlist.cast_to_blocks(cast, ctlist.expand(cl), cl.blocks)
    assert ref.shape == (85, 2049)
    out = ctlist.cast_list_to_blocks(cast, cl)
    assert out.shape == ref.shape
    assert np.array_equal(out, ref), f"host form: rows {first_rows(out, ref)}"
    d = ctlist.cast_list_to_blocks_device(cast, cl)
    assert tuple(d.shape) == ref.shape and d.is_cuda
    assert np.array_equal(to_host(d), ref), f"device form: rows {first_rows(to_host(d), ref)}"
    d2 = ctlist.cast_list_to_blocks_device(cast, cl, d_words=to_dev(ctlist.list_words(cl)))
    assert np.array_equal(to_host(d2), ref)
    assert np.array_equal(ctlist.cast_list_to_blocks(cast, cl, 84), ref[:84])
    assert ctlist.unpack_values(ck.decrypt(out, R.SPACE), kinds) == vals


# ---- 5. contract ---------------------------------------------------------------------------------------------------
def code(f):
    with pytest.raises(tfhe_amd.TfheError) as e:
        f()
    return e.value.code


def last_error():
    return tfhe_amd.lib().tfhe_hip_last_error().decode()


def test_expand_compact_contract(plain_engine):
    eng = plain_engine
    cl = E.random_list(8, 11, 5)
    w = ctlist.list_words(cl)
    assert w.size == 27
    assert code(lambda: eng.expand_compact(w[:-1], 8, 11)) == -1 and "list_words" in last_error()
    assert code(lambda: eng.expand_compact(w, 8, 12)) == -1
    assert code(lambda: eng.expand_compact(w, 8, 11, rep=0)) == -1 and "rep" in last_error()
    assert code(lambda: eng.expand_compact(w, 8, 11, rep=2, rows=23)) == -1 and "rows" in last_error()
    assert code(lambda: eng.expand_compact(w, 4, 11)) == -1
    assert code(lambda: eng.expand_compact(w, 48, 11)) == -1
    assert code(lambda: eng.expand_compact(np.zeros(8192 + 3, dtype=np.uint64), 8192, 3)) == -5
    assert "4096" in last_error()
    L, u = tfhe_amd.lib(), ctypes.POINTER(ctypes.c_uint64)
    out = np.zeros((11, 9), dtype=np.uint64)
    assert L.tfhe_hip_expand_compact(eng._h, None, 27, 8, 11, 1, 11, out.ctypes.data_as(u)) == -1
    assert "null buffer" in last_error()
    assert L.tfhe_hip_expand_compact(eng._h, w.ctypes.data_as(u), 27, 8, 11, 1, 11, None) == -1
    assert L.tfhe_hip_expand_compact_async(eng._h, None, 27, 8, 11, 1, 11, None, None) == -1
    # rows == 0, count == 0
    assert eng.expand_compact(w, 8, 11, rows=0).shape == (0, 9)
    assert eng.expand_compact(np.zeros(0, dtype=np.uint64), 8, 0).shape == (0, 9)
    assert tuple(eng.expand_compact_device(to_dev(w), 8, 11, rows=0).shape) == (0, 9)
    assert code(lambda: eng.expand_compact(w, 8, 0)) == -1
    # a P-GATE ctx has io_dim = n = 630: no compact list has that dimension (checked before the keys)
    lut = np.zeros(1024, dtype=np.uint64)
    assert code(lambda: eng.expand_cast(w, 11, lut)) == -1 and "io_dim" in last_error()
    d = to_dev(w)
    assert code(lambda: eng.expand_cast_device(d, 11, to_dev(lut))) == -1 and "io_dim" in last_error()


def test_expand_cast_contract():
    cs = E.small_case()
    w = ctlist.list_words(cs.cl)
    d_w, d_luts = to_dev(w), to_dev(cs.luts)
    with tfhe_amd.Engine(cs.params, 0) as eng:
        # nothing loaded, then the BSK alone: refused like pbs -- but the list checks come first
        for load in (lambda: None, lambda: eng.load_bsk(cs.sk.bsk)):
            load()
            assert code(lambda: eng.expand_cast(w, cs.cl.count, cs.luts, 2)) == -4
            assert code(lambda: eng.expand_cast_device(d_w, cs.cl.count, d_luts, 2)) == -4
            assert code(lambda: eng.expand_cast(w[:-1], cs.cl.count, cs.luts, 2)) == -1
        assert eng.expand_compact(w, 64, cs.cl.count).shape == (70, 65)  # the stage-level call needs no key
        eng.load_keys(cs.sk)
        ref = eng.expand_cast(w, cs.cl.count, cs.luts, 2, lut_index=cs.idx)
        assert code(lambda: eng.expand_cast(w[:-1], cs.cl.count, cs.luts, 2)) == -1 and "list_words" in last_error()
        assert code(lambda: eng.expand_cast_device(d_w[:-1], cs.cl.count, d_luts, 2)) == -1
        assert code(lambda: eng.expand_cast(w, cs.cl.count, cs.luts, 0)) == -1
        assert code(lambda: eng.expand_cast(w, cs.cl.count, cs.luts, 2, rows=141)) == -1
        assert code(lambda: eng.expand_cast(w, cs.cl.count, np.zeros((0, 1024), dtype=np.uint64), 2)) == -1
        assert "n_lut" in last_error()
        bad = cs.idx.copy()
        bad[77] = 2
        assert code(lambda: eng.expand_cast(w, cs.cl.count, cs.luts, 2, lut_index=bad)) == -1
        assert "lut_index[77]" in last_error()
        with pytest.raises(ValueError):
            eng.expand_cast(w, cs.cl.count, cs.luts, 2, lut_index=cs.idx[:-1])
        L, u = tfhe_amd.lib(), ctypes.POINTER(ctypes.c_uint64)
        lp = cs.luts.ctypes.data_as(u)
        assert L.tfhe_hip_expand_cast(eng._h, None, w.size, 70, 2, 140, lp, 2, None, lp) == -1
        assert "null buffer" in last_error()
        # rows above 0x7FFFFFFF is a case of its own: count, list_words and rep pass, rows <= count * rep; the checks
        # precede device work, so the buffers are never read
        big = (eng._h, lp, 1 << 31, 1 << 30, 4, 1 << 31, lp, 2, None, lp)
        assert L.tfhe_hip_expand_cast(*big) == -1 and "too many rows" in last_error()
        v = ctypes.c_void_p(cs.luts.ctypes.data)
        assert L.tfhe_hip_expand_cast_async(eng._h, v, 1 << 31, 1 << 30, 4, 1 << 31, v, 2, None, v, None) == -1
        assert "too many rows" in last_error()
        assert L.tfhe_hip_expand_compact(eng._h, lp, 1 << 31, 64, 1 << 30, 4, 1 << 31, lp) == -1
        assert "too many rows" in last_error()
        # rows == 0, count == 0; n_lut == 0 is refused even then
        assert code(lambda: eng.expand_cast(w, cs.cl.count, np.zeros((0, 1024), dtype=np.uint64), 2, rows=0)) == -1
        assert "n_lut" in last_error()
        assert eng.expand_cast(w, cs.cl.count, cs.luts, 2, rows=0).shape == (0, 65)
        assert eng.expand_cast(np.zeros(0, dtype=np.uint64), 0, cs.luts).shape == (0, 65)
        assert tuple(eng.expand_cast_device(d_w, cs.cl.count, d_luts, 2, rows=0).shape) == (0, 65)
        # a later BSK-only load makes the ctx rotation-only again
        eng.load_bsk(cs.sk.bsk)
        assert code(lambda: eng.expand_cast(w, cs.cl.count, cs.luts, 2)) == -4
    # two shards on one device give the single-shard words through the async form
    d_idx = idx_dev(cs.idx)
    with tfhe_amd.Engine(cs.params, [0, 0]) as eng2:
        eng2.load_keys(cs.sk)
        d = eng2.expand_cast_device(d_w, cs.cl.count, d_luts, 2, d_lut_index=d_idx)
        assert np.array_equal(to_host(d), ref), f"rows {first_rows(to_host(d), ref)}"
        assert np.array_equal(eng2.expand_cast(w, cs.cl.count, cs.luts, 2, lut_index=cs.idx), ref)
        assert np.array_equal(to_host(eng2.expand_compact_device(d_w, 64, cs.cl.count)), ctlist.expand(cs.cl))


def test_timing_slots(cast_case):
    """An order-1 engine with the MS noise reduction on: the expansion in slot 3, the PBS in slots 1, 2 and 0."""
    _, cl, _, _, cast = cast_case
    cast.timing(True)
    cast.timing_reset()
    try:
        ctlist.cast_list_to_blocks(cast, cl)
        ctlist.cast_list_to_blocks(cast, cl, 3)
        for slot in (3, 1, 2, 0):
            ms, launches = cast.timing_stats(slot)
            assert launches == 2 and ms > 0, slot
        ctlist.expand_device(cast, cl)
        ctlist.expand_device(cast, cl, rep=2, rows=5)
        assert cast.timing_stats(3)[1] == 4
        for slot in (1, 2, 0):
            assert cast.timing_stats(slot)[1] == 2, slot
        assert code(lambda: cast.timing_stats(4)) == -1
    finally:
        cast.timing(False)
        cast.timing_reset()
