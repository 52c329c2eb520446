"""The level assembly kernel (tfhe_amd/csrc/lincomb.hip) on the MI355X: sparse linear combinations of LWE rows
through Engine.lincomb* against radix.lincomb_ref bit for bit, the argument contract of the C entry points, and
tfhe_hip_lincomb_pbs_async against its two halves."""
import ctypes

import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import radix as R

pytestmark = pytest.mark.gpu

BUF_ROWS = (1, 4, 9)
COEFS = (0, 1, 4, 1 << 63, (1 << 64) - 1)
SENTINEL = 0x5E5E5E5E5E5E5E5E
EINVAL = -1


def make_case(dim, counts, seed, with_bias):
    """Three source buffers of 1, 4 and 9 rows and a term description with ``counts[r]`` terms in row r.  The first two
    terms of a row name the same source, which is also the first source of every other row with terms; the coefficients
    walk through COEFS first."""
    rng = np.random.default_rng(seed)
    bufs = [rng.integers(0, 1 << 64, (n, dim), dtype=np.uint64) for n in BUF_ROWS]
    row_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    T = int(row_start[-1])
    term_buf = rng.integers(0, 3, T).astype(np.uint32)
    term_row = np.array([rng.integers(0, BUF_ROWS[b]) for b in term_buf], dtype=np.uint32)
    term_coef = rng.integers(0, 1 << 64, T, dtype=np.uint64)
    term_coef[:len(COEFS)] = np.array(COEFS, dtype=np.uint64)[:T]
    for r, n in enumerate(counts):
        t = int(row_start[r])
        if n >= 1:
            term_buf[t], term_row[t] = 2, 7
        if n >= 2:
            term_buf[t + 1], term_row[t + 1] = 2, 7
    bias = rng.integers(0, 1 << 64, len(counts), dtype=np.uint64) if with_bias else None
    if with_bias and len(counts) > 1:
        bias[-1] = 0
    return bufs, row_start, term_buf, term_row, term_coef, bias


def ragged_counts(rows):
    """0 .. 6 terms a row: six in row 0, none in row 1, then every count in turn."""
    return [(6, 0, 3, 1, 2, 4, 5)[r % 7] for r in range(rows)]


def to_device(bufs):
    import torch
    return [torch.from_numpy(b.view(np.int64)).to("cuda:0") for b in bufs]


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


# ---- 4. the kernel against lincomb_ref --------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 2, 3, 257])
@pytest.mark.parametrize("dim", [2049, 919, 631])
def test_lincomb_matches_ref(fhevm_fft_engine, dim, rows):
    import torch
    eng = fhevm_fft_engine
    cases = [ragged_counts(rows)] + ([[0]] if rows == 1 else [])   # one row: six terms, and none
    for counts in cases:
        for with_bias in (False, True):
            case = make_case(dim, counts, seed=dim * 1000 + rows, with_bias=with_bias)
            bufs = case[0]
            want = R.lincomb_ref(*case, dim)
            if rows > 1:
                assert 0 in counts and max(counts) == 6
            d_bufs = to_device(bufs)
            got = to_host(eng.lincomb_device(d_bufs, *case[1:], dim=dim))
            np.testing.assert_array_equal(got, want, err_msg=f"lincomb_device, bias {with_bias}")
            # into the middle of a larger tensor: the rows around the output stay as they were
            guard = torch.full((rows + 2, dim), SENTINEL, dtype=torch.int64, device="cuda:0")
            eng.lincomb_async(d_bufs, *case[1:], guard[1:-1])
            g = to_host(guard)
            np.testing.assert_array_equal(g[1:-1], want, err_msg="lincomb_async")
            assert np.all(g[0] == SENTINEL) and np.all(g[-1] == SENTINEL)
            np.testing.assert_array_equal(eng.lincomb(bufs, *case[1:], dim=dim), want, err_msg="host form")
            for b, d in zip(bufs, d_bufs):
                np.testing.assert_array_equal(to_host(d), b, err_msg="a source was written")


def test_lincomb_zero_rows(fhevm_fft_engine):
    eng = fhevm_fft_engine
    bufs = [np.ones((2, 631), dtype=np.uint64)]
    out = eng.lincomb_device(to_device(bufs), [0], [], [], [], None, dim=631)
    assert tuple(out.shape) == (0, 631)
    assert eng.lincomb(bufs, [0], [], [], [], None, dim=631).shape == (0, 631)
    assert tuple(eng.lincomb_device([], [0], [], [], []).shape) == (0, eng.params.io_dim + 1)
    # no source at all: every row trivial
    out = to_host(eng.lincomb_device([], [0, 0, 0], [], [], [], [5, 7], dim=919))
    assert not out[:, :-1].any() and out[:, -1].tolist() == [5, 7]


# ---- 5. the contract --------------------------------------------------------------------------------------------
def test_lincomb_contract(fhevm_fft_engine):
    import torch
    eng, L, dim = fhevm_fft_engine, tfhe_amd.lib(), 631
    bufs, row_start, term_buf, term_row, term_coef, bias = case = make_case(dim, ragged_counts(3), seed=5, with_bias=True)
    want = R.lincomb_ref(*case, dim)
    d_bufs = to_device(bufs)
    d_out = torch.full((3, dim), SENTINEL, dtype=torch.int64, device="cuda:0")
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)

    def raw(dim=dim, d_bufs_arg=True, rs=row_start, tb=term_buf, tr=term_row, tc=term_coef, bs=bias, rows=3, out=d_out,
            n_buf=3):
        """tfhe_hip_lwe_lincomb_async with any argument replaced; None = a null pointer."""
        ptrs = (ctypes.c_void_p * 3)(*[b.data_ptr() for b in d_bufs])
        nrow = (ctypes.c_size_t * 3)(*BUF_ROWS)
        def p(a, t):
            return None if a is None else np.ascontiguousarray(a).ctypes.data_as(t)
        keep = [np.ascontiguousarray(a) if a is not None else None for a in (rs, tb, tr, tc, bs)]
        return L.tfhe_hip_lwe_lincomb_async(
            eng._h, dim, ptrs if d_bufs_arg else None, nrow, n_buf, p(keep[0], u32p), p(keep[1], u32p), p(keep[2], u32p),
            p(keep[3], u64p), p(keep[4], u64p), rows, ctypes.c_void_p(out.data_ptr()) if out is not None else None,
            ctypes.c_void_p(tfhe_amd._stream_handle(None, eng.device)))

    def works():
        d_out.fill_(SENTINEL)
        assert raw() == 0
        np.testing.assert_array_equal(to_host(d_out), want)

    def bad(v, i, x):
        w = np.array(v).copy()
        w[i] = x
        return w

    works()
    refusals = {
        "null output": dict(out=None),
        "null row_start": dict(rs=None),
        "null term_row": dict(tr=None),
        "null term_coef": dict(tc=None),
        "null term_buf": dict(tb=None),
        "null d_bufs": dict(d_bufs_arg=False),
        "dim == 0": dict(dim=0),
        "row_start[0] != 0": dict(rs=bad(row_start, 0, 1)),
        "row_start decreases": dict(rs=bad(row_start, 2, 5)),          # 0, 6, 5, 9
        "term_buf >= n_buf": dict(tb=bad(term_buf, 4, 3)),
        "term_buf >= a smaller n_buf": dict(n_buf=2),                  # the terms name buffer 2
        "term_row >= buf_rows": dict(tb=bad(term_buf, 3, 1), tr=bad(term_row, 3, 4)),
        "rows beyond 32 bits": dict(rows=1 << 32),
        "rows beyond the launch limit": dict(rows=1 << 31),
    }
    for name, kw in refusals.items():
        d_out.fill_(SENTINEL)
        assert raw(**kw) == EINVAL, name
        assert L.tfhe_hip_last_error(), name
        torch.cuda.synchronize()
        assert np.all(to_host(d_out) == np.uint64(SENTINEL)), f"{name}: something was launched"
        works()
    # an output that overlaps a source: valid pointers, refused (last rows of buffer 2, and the whole of buffer 1)
    for src, lo in ((d_bufs[2], 6), (d_bufs[1], 1)):
        before = to_host(src).copy()
        with pytest.raises(tfhe_amd.TfheError) as e:
            eng.lincomb_async(d_bufs, row_start, term_buf, term_row, term_coef, bias, src[lo:lo + 3])
        assert e.value.code == EINVAL and "overlaps" in str(e.value)
        np.testing.assert_array_equal(to_host(src), before)
        works()
    # the same checks through the Python methods and through the fused call
    with pytest.raises(tfhe_amd.TfheError) as e:
        eng.lincomb_device(d_bufs, bad(row_start, 2, 5), term_buf, term_row, term_coef, bias, dim=dim)
    assert e.value.code == EINVAL
    one_row, one_term, one_coef = np.array([0, 1], dtype=np.uint32), np.array([1], dtype=np.uint32), np.ones(1, dtype=np.uint64)
    host_out = np.zeros((1, dim), dtype=np.uint64)
    assert L.tfhe_hip_lwe_lincomb(eng._h, dim, tfhe_amd._u64(bufs[0]), 1, one_row.ctypes.data_as(u32p),
                                  one_term.ctypes.data_as(u32p), tfhe_amd._u64(one_coef), None, 1,
                                  tfhe_amd._u64(host_out)) == EINVAL   # the host form: row 1 of a one-row buffer
    assert not host_out.any()
    io = eng.params.io_dim + 1
    d_io = to_device([np.zeros((n, io), dtype=np.uint64) for n in BUF_ROWS])
    d_luts = to_device([tfhe_amd.lut_constant(eng.params.N, tfhe_amd.MU)[None]])[0]
    with pytest.raises(tfhe_amd.TfheError) as e:
        eng.lincomb_pbs_device(d_io, row_start, term_buf, bad(term_row, 3, 9), term_coef, bias, d_luts)
    assert e.value.code == EINVAL
    works()


# ---- 6. the fused call against its halves -------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [5, 300, 600])
def test_lincomb_pbs_equals_its_halves(fhevm_fft_engine, fhevm_fft_keys, rows):
    """5 and 300 rows straddle the latency-kernel switch of the N = 1024 FFT engine (256); this engine (N = 2048)
    switches at 512 (pbs_fft2k.hip ENGINE_FFT2K), so 600 rows cover its batch configuration."""
    import torch
    eng = fhevm_fft_engine
    ck, _ = fhevm_fft_keys
    rng = np.random.default_rng(rows)
    x = ck.encrypt(rng.integers(0, 4, 40), R.SPACE, seed=0x11C0 + rows)
    y = ck.encrypt(rng.integers(0, 4, 24), R.SPACE, seed=0x11C1 + rows, stream0=40)
    bufs = [x, y]
    # 4 x + y (bivariate), a clean block alone, 3 - y, and a trivial row, in turn
    kinds = np.arange(rows) % 4
    ix, iy = rng.integers(0, 40, rows), rng.integers(0, 24, rows)
    rs, tb, tr, tc, bias = [0], [], [], [], []
    for k, i, j in zip(kinds, ix, iy):
        terms = [[(0, i, 4), (1, j, 1)], [(0, i, 1)], [(1, j, (1 << 64) - 1)], []][k]
        for b, r, c in terms:
            tb.append(b), tr.append(r), tc.append(c)
        rs.append(len(tb))
        bias.append([0, 0, 3 * R.DELTA, 9 * R.DELTA][k])
    desc = (np.array(rs, dtype=np.uint32), np.array(tb, dtype=np.uint32), np.array(tr, dtype=np.uint32),
            np.array(tc, dtype=np.uint64), np.array(bias, dtype=np.uint64))
    tables = [R.T_AND, R.T_MSG, R.T_CMP]
    luts = np.stack([tfhe_amd.lut_from_table(eng.params.N, R.SPACE, list(t), R.DELTA) for t in tables])
    idx = rng.integers(0, 3, rows).astype(np.uint32)
    d_bufs = to_device(bufs)
    d_luts = to_device([luts])[0]
    d_idx = torch.from_numpy(idx.view(np.int32)).to("cuda:0")

    fused = to_host(eng.lincomb_pbs_device(d_bufs, *desc, d_luts, d_idx))
    lin = eng.lincomb_device(d_bufs, *desc)
    assembled = R.lincomb_ref(bufs, *desc, eng.params.io_dim + 1)
    np.testing.assert_array_equal(to_host(lin), assembled)
    halves = to_host(eng.pbs_device(lin, d_luts, d_idx))
    host = eng.pbs(assembled, luts, idx)
    np.testing.assert_array_equal(fused, halves)
    np.testing.assert_array_equal(fused, host)
    # and the rows mean what they say
    vx, vy = ck.decrypt(x, R.SPACE).astype(np.int64)[ix], ck.decrypt(y, R.SPACE).astype(np.int64)[iy]
    v = np.choose(kinds, [4 * vx + vy, vx, 3 - vy, np.full(rows, 9)])
    want = np.array([tables[t][int(a)] for t, a in zip(idx, v)])
    np.testing.assert_array_equal(ck.decrypt(fused, R.SPACE), want)
