"""The device-buffer entry points (pbs_async, bootstrap_async, pbs_many_async) on the MI355X, judged on what they write
OUTSIDE their output as well as inside it.  The output of every call is the middle of a sentinel-filled tensor
(tests/guard_rows.py; tests/test_guard_rows.py shows the checker catching planted writes), so a missing b < B guard of
a padded workgroup, a 16-column tile that stores past column n of the last row, or a rows = B * n_fn slip of the
many-LUT keyswitch shows as a written guard word.  After each call:

  a. the guard rows in front of and behind the B (or B * n_fn) output rows are untouched;
  b. the payload equals the oracle's rows, word for word (every row for B = 1 and 5, rows KS_ROWS_257 for B = 257);
  c. the whole payload equals the host-buffer call of the same engine (this covers the rows b leaves out);
  d. (B = 5) the payload does not depend on what lies around the B input rows: the same rows between two different
     sets of random neighbours give the same words.

Which kernel is the last writer into the caller's buffer depends on the entry point and the parameter order: the
blind-rotation kernel in its write-big mode (bootstrap_async always, pbs_async at order 1), a keyswitch kernel over
rows of n + 1 words (pbs_async and pbs_many_async at order 0: ks_gemm_kernel on the matrix cores, keyswitch_kernel on
the VALU), or sample_extract_many_kernel (pbs_many_async at order 1: its Z_p form on the NTT engines, its torus form
on the FFT64 ones).  Each test prints the writer of every combination it ran (pytest -s).

Engines: presets 0 - 3 at n = 16 (n + 1 = 17: the body alone in a second 16-column tile) and n = 15 (one full
tile), both keyswitch kernels on the two order-0 presets, both rotation kernels everywhere; multi-bit keys of
g = 2, 3, 4 at n = 12.  At these n the default noise-reduction bound of an order-1 engine is an early-out
(offpreset_cases.MsCase), which the references assert on the oracle: keyswitch, then the rotation.

Out of scope here: bases that are only 8-byte aligned (the guards are whole rows in an even count, so the view keeps
the 16-byte alignment of a fresh allocation), in-place calls, sharded engines, timing."""
import ctypes
import functools

import numpy as np
import pytest

import tfhe_amd
from conftest import KEY_SEED
import guard_rows as G
import offpreset_cases as C
import test_decompress as T
from test_gpu_many_lut import rotate_down
from test_gpu_offpreset_n import BR_NAMES, bad_rows, both_rotation_kernels, open_engine
from test_multibit import DELTA, TABLE, toy_params, _toy_cts

pytestmark = pytest.mark.gpu

NS = (16, 15)
BATCHES = (1, 5, 257)
B_MAX = 257                       # crosses the 256-row matrix-core tile and the 64-row VALU tile; runs on a side stream
B_NEIGHBOURS = 5                  # the batch of check d; pads the 8-, 4- and 2-per-workgroup rotation shapes
LUT_INDEX = (np.arange(B_MAX) % 3).astype(np.uint32)
KS_NAMES = {"mfma": "ks_gemm_kernel", "valu": "keyswitch_kernel"}
MB_KERNEL = "blind_rotate_fft2k_mb_kernel"
MB_BATCHES = (1, 2, 5)            # two ciphertexts per workgroup: 1 and 5 leave a padding half
# (preset, n, keyswitch kernel): the VALU kernel where the keyswitch is the last writer (order 0: presets 0 and 2)
CLASSIC = [(p, n, k) for p in C.PRESETS for n in NS for k in (("mfma", "valu") if p in (0, 2) else ("mfma",))]


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64, order="C").view(np.int64)).to(G.DEVICE)  # a copy: some are frozen


def idx_dev(idx):
    import torch
    return torch.from_numpy(np.ascontiguousarray(idx, dtype=np.uint32).view(np.int32)).to(G.DEVICE)


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def many_luts(N, n_fn, seed):
    """Three many-LUTs of n_fn random tables each (lut_many) -> ([3][N], stride = N / n_fn)."""
    rng = np.random.default_rng(seed)
    made = [tfhe_amd.lut_many(N, 16, [[int(v) for v in rng.integers(0, 16, 16 // n_fn)] for _ in range(n_fn)],
                              1 << T.DELTA_LOG) for _ in range(3)]
    assert all(stride == N // n_fn for _, stride in made)
    return np.stack([lut for lut, _ in made]), N // n_fn


class Entry:
    """One entry point with its inputs: ``cts`` [rows][in_len] (a batch of B is its first B rows, LUT of row r =
    luts[LUT_INDEX[r]]), per_ct output rows of row_len words per ciphertext, the device-buffer call
    run_async(eng, d_in, d_luts, d_out, d_idx, stream), the host-buffer call run_host(eng, cts, idx) and the oracle's
    output of some rows, {row: [per_ct * row_len]} (None: no oracle of this engine, checks a, c and d only)."""

    def __init__(self, name, cts, luts, per_ct, row_len, run_async, run_host, ref=None):
        self.name, self.cts, self.luts, self.per_ct, self.row_len = name, cts, luts, per_ct, row_len
        self.run_async, self.run_host, self.ref = run_async, run_host, ref


def pbs_entry(cts, luts, row_len, ref=None):
    return Entry("pbs_async", cts, luts, 1, row_len,
                 lambda eng, d_in, d_luts, d_out, d_idx, st: eng.pbs_async(d_in, d_luts, d_out, d_idx, stream=st),
                 lambda eng, c, idx: eng.pbs(c, luts, idx), ref)


def bootstrap_entry(cts, luts, row_len, ref=None):
    return Entry("bootstrap_async", cts, luts, 1, row_len,
                 lambda eng, d_in, d_luts, d_out, d_idx, st: eng.bootstrap_async(d_in, d_luts, d_out, d_idx, stream=st),
                 lambda eng, c, idx: eng.bootstrap(c, luts, idx), ref)


def many_entry(cts, luts, stride, n_fn, row_len, ref=None):
    return Entry(f"pbs_many_async n_fn = {n_fn}", cts, luts, n_fn, row_len,
                 lambda eng, d_in, d_luts, d_out, d_idx, st:
                     eng.pbs_many_async(d_in, d_luts, d_out, n_fn, stride, d_idx, stream=st),
                 lambda eng, c, idx: eng.pbs_many(c, luts, n_fn, stride, idx), ref)


# ---- the oracle's side, once per (preset, n) ------------------------------------------------------------------------
class Case:
    """257 encryptions of 4-bit messages at 2^59 under the oracle's keys (rows 0 - 3: the edge messages 0, 15, 8, 7 of
    offpreset_cases.PbsCase), under the input-side key for pbs / pbs_many and under the small key for bootstrap;
    three LUTs and three many-LUTs per n_fn through LUT_INDEX; the oracle's outputs of rows KS_ROWS_257, which hold
    rows 0 - 4 (all of B = 1 and 5) and 256, the last row."""

    def __init__(self, preset, n):
        O = C.oracle()
        ks = self.ks = C.keyset(preset, n)
        prm, okeys = ks.prm, ks.okeys
        N, self.order1 = prm.N, prm.order == 1
        self.io_len, self.big_len, self.small_len = (ks.big_dim if self.order1 else n) + 1, ks.big_dim + 1, n + 1
        rng = np.random.default_rng(0xDB0F + 100 * preset + n)
        msgs = rng.integers(0, 16, B_MAX).astype(np.uint64)
        msgs[:4] = [0, 15, 8, 7]
        torus = np.ascontiguousarray(msgs << np.uint64(T.DELTA_LOG))
        self.cts = C._frozen(okeys.encrypt(torus, seed=0xC0FFEE01 + n))
        assert self.cts.shape == (B_MAX, self.io_len)
        if self.order1:                    # the rotation's own input: under the small key
            small = np.zeros((B_MAX, n + 1), dtype=np.uint64)
            O.lib().or_lwe_encrypt(ctypes.c_uint32(n), O._p(okeys.lwe_key), ctypes.c_int32(prm.lwe_noise_log2),
                                   ctypes.c_uint64(0xC0FFEE51 + n), ctypes.c_uint64(0), O._p(torus),
                                   ctypes.c_size_t(B_MAX), O._p(small))
            self.small = C._frozen(small)
        else:
            self.small = self.cts
        self.luts = C._frozen(np.stack([O.lut_from_table(N, 16, t, 1 << T.DELTA_LOG) for t in C.PBS_TABLES]))
        self.many = {n_fn: many_luts(N, n_fn, 0x3A17 + 10 * preset + n_fn) for n_fn in (2, 4)}

        rows = C.KS_ROWS_257
        assert set(range(B_NEIGHBOURS)) <= set(rows) and B_MAX - 1 in rows
        extract = O.sample_extract_torus if prm.transform == 1 else O.sample_extract

        def keyswitch(big):
            return O.keyswitch(prm, okeys, big)

        def rotate(ct, lut):               # -> (accumulator, its degree-0 sample)
            return T.bootstrap_ref(O, prm, okeys, ct, lut)

        if self.order1:
            # keyswitch -> [noise reduction: nothing to do at this n under the default bound] -> rotation
            rot_in = {r: keyswitch(self.cts[r]) for r in rows}
            stacked = np.stack([rot_in[r] for r in rows])
            reduced, picks = O.ms_reduce(prm, okeys, stacked)
            assert (picks == -1).all() and np.array_equal(reduced, stacked), "the default bound is no early-out here"
            self.ref_pbs = {r: rotate(rot_in[r], self.luts[LUT_INDEX[r]])[1] for r in rows}
        else:
            rot_in = {r: self.cts[r] for r in rows}
            self.ref_pbs = dict(zip(rows, O.pbs_batch(prm, okeys, self.cts[list(rows)], self.luts, LUT_INDEX[list(rows)])))
        self.ref_boot = {r: rotate(self.small[r], self.luts[LUT_INDEX[r]])[1] for r in rows}
        self.ref_many = {}
        for n_fn, (mluts, stride) in self.many.items():
            ref = {}
            for r in rows:
                acc = rotate(rot_in[r], mluts[LUT_INDEX[r]])[0]
                # the sample at degree f * stride = the degree-0 sample of X^{-f stride} * acc (rotate_down, extract_at
                # of tests/test_gpu_many_lut.py), here with the oracle's extraction
                big = [extract(prm, rotate_down(acc[None], ks.params, f * stride)[0]) for f in range(n_fn)]
                ref[r] = np.concatenate(big if self.order1 else [keyswitch(b) for b in big])
            self.ref_many[n_fn] = ref

    def entries(self):
        return (pbs_entry(self.cts, self.luts, self.io_len, self.ref_pbs),
                bootstrap_entry(self.small, self.luts, self.big_len, self.ref_boot), self.many_entry(2))

    def many_entry(self, n_fn):
        mluts, stride = self.many[n_fn]
        return many_entry(self.cts, mluts, stride, n_fn, self.io_len, self.ref_many[n_fn])


@functools.lru_cache(maxsize=None)
def case(preset, n):
    return Case(preset, n)


# ---- one guarded call ---------------------------------------------------------------------------------------------
class Streams:
    """The B = 257 calls run on a side stream that first waits for torch's current stream (the uploads and the
    sentinel fill), the others on the current stream; both are synchronised before anything is read."""

    def __init__(self, big_batch):
        import torch
        self.torch, self.big_batch = torch, big_batch
        self.side = torch.cuda.Stream(G.DEVICE)

    def run(self, B, call):
        cur = self.torch.cuda.current_stream(G.DEVICE)
        if B == self.big_batch:
            self.side.wait_stream(cur)
            call(self.side)
            self.side.synchronize()
        else:
            call(None)
            cur.synchronize()


def guarded_call(eng, ent, B, streams, fill_seed, what):
    """ent's device-buffer call on the first B rows, the input between random neighbours of fill_seed, the output
    between guard rows -> the payload [B][per_ct * row_len]; asserts check a and that the input is as uploaded."""
    idx = LUT_INDEX[:B]
    d_luts, d_idx = to_dev(ent.luts), idx_dev(idx)
    whole_in, d_in = G.embedded(ent.cts[:B], fill_seed=fill_seed)
    before = to_host(whole_in)
    whole, d_out = G.guarded(B * ent.per_ct, ent.row_len)
    assert d_in.is_contiguous() and d_out.is_contiguous() and d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    streams.run(B, lambda st: ent.run_async(eng, d_in, d_luts, d_out, d_idx, st))
    G.assert_guards(whole, B * ent.per_ct, what)
    assert np.array_equal(to_host(whole_in), before), f"{what}: the input tensor was written"
    return to_host(d_out).reshape(B, ent.per_ct * ent.row_len)


def check_entry(eng, ent, B, streams, what, big_batch=B_MAX, ref_rows=C.KS_ROWS_257):
    got = guarded_call(eng, ent, B, streams, 1, what)                                          # a
    if ent.ref is not None:                                                                    # b
        for r in (ref_rows if B == big_batch else range(B)):
            want = ent.ref[r]
            assert np.array_equal(got[r], want), f"{what}: row {r} differs from the oracle in words {np.nonzero(got[r] != want)[0][:8]}"
    host = ent.run_host(eng, ent.cts[:B], LUT_INDEX[:B]).reshape(B, -1)                       # c
    assert np.array_equal(got, host), f"{what}: rows {bad_rows(got, host)} differ from the host-buffer call"
    if B == B_NEIGHBOURS:                                                                      # d
        other = guarded_call(eng, ent, B, streams, 2, what + ", other input neighbours")
        assert np.array_equal(other, got), f"{what}: rows {bad_rows(other, got)} depend on the input's neighbours"
    return got


def writer(ent, order1, br_name, ks_kernel, zp):
    """The kernel that stores into the caller's buffer (pbs_device, bootstrap_device in csrc/api.cpp)."""
    if ent.name.startswith("bootstrap") or (order1 and ent.name.startswith("pbs_async")):
        return br_name + " (write-big)"
    if order1:
        return "sample_extract_many_kernel, " + ("Z_p form" if zp else "torus form")
    return KS_NAMES[ks_kernel]


# ---- classic keys ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,n,kernel", CLASSIC, ids=[f"p{p}-n{n}-{k}" for p, n, k in CLASSIC])
def test_classic_engines_write_their_rows_only(preset, n, kernel):
    cs = case(preset, n)
    zp = cs.ks.params.transform == tfhe_amd.TRANSFORM_NTT
    streams = Streams(B_MAX)
    table = []
    with open_engine(cs.ks, kernel) as eng:
        try:
            for br_name in both_rotation_kernels(eng, preset, B_MAX):
                for ent in cs.entries():
                    for B in BATCHES:
                        assert eng.br_kernel(B) == br_name
                        check_entry(eng, ent, B, streams, f"{ent.name} on {br_name}, {kernel} keyswitch, B = {B}")
                    table.append((ent.name, br_name, writer(ent, cs.order1, br_name, kernel, zp)))
            # four functions, once per engine: B * n_fn = 1028 rows through the last writer, on the batch kernel
            ent = cs.many_entry(4)
            assert eng.br_kernel(B_MAX) == br_name == BR_NAMES[preset][1]
            check_entry(eng, ent, B_MAX, streams, f"{ent.name} on {br_name}, {kernel} keyswitch, B = {B_MAX}")
            table.append((ent.name, br_name, writer(ent, cs.order1, br_name, kernel, zp)))
        finally:
            eng.set_latency_batch(C.LAT_DEFAULT[preset])
    assert len(table) == 7
    for name, br_name, w in table:
        print(f"last writer | {name} | preset {preset}, n = {n} | {br_name} | {kernel} | {w}")


def test_classic_cases_cover_every_kernel():
    """12 classic cases: both n on every preset, the VALU keyswitch where the keyswitch writes the caller's buffer."""
    assert len(CLASSIC) == 12
    assert {(p, k) for p, _, k in CLASSIC} == {(0, "mfma"), (0, "valu"), (1, "mfma"), (2, "mfma"), (2, "valu"), (3, "mfma")}
    assert {p for p in C.PRESETS if C.oracle().params(p).order == 0} == {0, 2}
    assert set(BR_NAMES) == set(C.PRESETS)


# ---- multi-bit keys -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", (2, 3, 4))
def test_multibit_engine_writes_its_rows_only(g):
    """toy n = 12, N = 2048, order 1.  The host-buffer calls are judged by tests/test_gpu_multibit.py against the exact
    arbiter; here the device-buffer calls equal them and touch nothing else.  Every wave of the kernel reads both
    ciphertexts of its workgroup, so a padding half reads a clamped row: check d at B = 5."""
    N = 2048
    ck, sk = tfhe_amd.gen_keys(toy_params(12), KEY_SEED, grouping=g)
    msgs = np.array([0, 7, 3, 5, 1])                                  # < 8: the first half of the space, for n_fn = 2
    tables = [TABLE, [(5 * v + 2) % 16 for v in range(16)], [(15 - v) % 16 for v in range(16)]]
    luts = np.stack([tfhe_amd.lut_from_table(N, 16, t, DELTA) for t in tables])
    mluts, stride = many_luts(N, 2, 0x3B17 + g)
    big = ck.encrypt(msgs, 16, seed=0xDB10 + g)
    small = _toy_cts(ck, msgs, seed=0xDB20 + g)
    assert big.shape == (5, N + 1) and small.shape == (5, 13)
    entries = (pbs_entry(big, luts, N + 1), bootstrap_entry(small, luts, N + 1), many_entry(big, mluts, stride, 2, N + 1))
    streams = Streams(None)
    with tfhe_amd.Engine(ck.params, 0) as eng:
        eng.load_keys(sk)
        assert eng.grouping == g
        for ent in entries:
            for B in MB_BATCHES:
                assert eng.br_kernel(B) == MB_KERNEL
                got = check_entry(eng, ent, B, streams, f"{ent.name} on {MB_KERNEL}, g = {g}, B = {B}", big_batch=None)
                idx = LUT_INDEX[:B]
                if ent.name == "bootstrap_async":
                    staged = eng.sample_extract(eng.blind_rotate(small[:B], luts, idx))
                    assert np.array_equal(got, staged), f"g = {g}, B = {B}: rows {bad_rows(got, staged)}"
                if ent.name == "pbs_async":
                    assert list(ck.decrypt(got, 16)) == [tables[int(i)][int(m)] for m, i in zip(msgs[:B], idx)]
            w = "sample_extract_many_kernel, torus form" if ent.per_ct > 1 else MB_KERNEL + " (write-big)"
            print(f"last writer | {ent.name} | g = {g}, n = 12 | {MB_KERNEL} | mfma | {w}")
