"""Packing keyswitch away from its one preset (tfhe_amd/csrc/pks.hip, the pks_* half of ks_mfma.hip,
pks_api.cpp), bit-exact against the oracle (or_pks_pack) with synthetic keys:

* a parameter sweep over both GEMMs tfhe_hip_pks_create chooses between (matrix cores: base <= 2^15,
  <= 8 levels, in_dim * level % 64 == 0; VALU + offset correction otherwise), with k > 1, lwe_per_glwe < N,
  many groups, and row counts across the 64-row VALU tile and the 256-row matrix-core tile;
* both GEMMs against each other at the production shape;
* the chunk loop of pack_device (a call whose T workspace exceeds PKS_T_BUDGET);
* workspace regrowth on one context;
* the call patterns that the header promises are ordered on a context's workspaces and key: calls on different
  streams, a regrowth and a key load issued straight behind an async call.

Key words and LWE words include the edges of the byte recoding and of the signed decomposition; the builders
and their CPU-side checks (digit coverage, the two-chunk arithmetic) are also run without a GPU from
tests/test_compression.py.  Every comparison is an integer equality."""
import functools
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT
from tfhe_amd import compression as C
from test_gpu_keyswitch import _edge_rows

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
EINVAL = -1                                                 # TFHE_HIP_EINVAL
# (in_dim, out_k, out_N, base_log, level, lwe_per_glwe) -> the GEMM tfhe_hip_pks_create must choose
SWEEP = {
    "mfma_k64_smallest": ((64, 1, 32, 4, 1, 32), "mfma"),
    "mfma_k3_17_per_glwe": ((64, 3, 64, 7, 3, 17), "mfma"),
    "mfma_base15": ((16, 1, 64, 15, 4, 64), "mfma"),
    "base16_x3_k3": ((64, 3, 32, 16, 3, 32), "valu"),      # two digit bytes cannot hold +2^15
    "base16_x1": ((256, 1, 64, 16, 1, 17), "valu"),
    "valu_K48": ((48, 1, 32, 5, 1, 32), "valu"),           # in_dim * level % 64 != 0
    "valu_base17": ((64, 1, 64, 17, 3, 64), "valu"),
    "valu_base31": ((32, 1, 32, 31, 2, 5), "valu"),
    "level9": ((64, 1, 32, 2, 9, 32), "valu"),             # the key planes stop at 8 levels
}
# 2^16 x 3 at k = 2, N = 32 has (k+1)N = 96, no multiple of the GEMMs' 64-column tile: the C ABI refuses it
# (pks_valid), so the sweep runs 2^16 x 3 at k = 3 above and tests/test_compression.py pins the refusal
REFUSED_FIELDS = (64, 2, 32, 16, 3, 32)
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257)                # + lwe_per_glwe + 3: a partial last group
EDGE_KEY_WORDS = np.array([0, U64, 0x7F7F7F7F7F7F7F7F, 0x8080808080808080, 0xFFFFFFFFFFFFFF80,
                           0x7FFFFFFFFFFFFFFF, 0x8000000000000000, 0x7F807F807F807F80], dtype=np.uint64)


def make_params(in_dim, out_k, out_N, base_log, level, lpg):
    """(product params, oracle params): the two ctypes structs have the same fields."""
    from oracle import oracle as O
    f = (in_dim, out_k, out_N, base_log, level, lpg, 26, -48)
    return C.PksParams(*f), O.PksParams(*f)


def expected_path(pp):
    """The selection rule of tfhe_hip_pks_create, restated."""
    return "mfma" if pp.base_log <= 15 and pp.level <= 8 and (pp.in_dim * pp.level) % 64 == 0 else "valu"


def synthetic_key(pp, seed):
    """Uniform words, then rows of one edge word each (the balanced byte recoding's carry through all eight
    planes, byte 0xFF plus carry, the dropped top carry), then rows cycling through the edge words."""
    rng = np.random.default_rng(seed)
    K, Nc = pp.in_dim * pp.level, pp.glwe_len
    k = rng.integers(0, U64, size=(K, Nc), dtype=np.uint64, endpoint=True)
    e = EDGE_KEY_WORDS.size
    k[:e] = EDGE_KEY_WORDS[:, None]
    k[e:2 * e] = EDGE_KEY_WORDS[(np.arange(e)[:, None] + np.arange(Nc)[None, :]) % e]
    return types.SimpleNamespace(pksk=np.ascontiguousarray(k.reshape(-1)))


def half_digit_rows(pp):
    """Rows whose digits sit at the ends of the balanced range: every state digit B/2 (the top level stays
    +B/2; below it the carry rule turns B/2 into -B/2), and B/2 alternating with 0 from either end (+B/2 with
    no carry at any level)."""
    B2, L, bl = 1 << (pp.base_log - 1), pp.level, pp.base_log
    nonrep = 64 - bl * L
    pats = [[1] * L, [(l + 1) % 2 for l in range(L)], [l % 2 for l in range(L)]]
    rows = []
    for pat in pats:
        state = sum(B2 << (bl * l) for l in range(L) if pat[l])
        rows.append(np.full(pp.in_dim + 1, (state << nonrep) & U64, dtype=np.uint64))
    return np.stack(rows)


N_EDGE = 8


def synthetic_lwes(pp, count, seed):
    """Uniform rows with N_EDGE edge rows in front: 0, 2^64-1, 2^63, rounding ties of the closest-representable
    step and one below (test_gpu_keyswitch._edge_rows at prec = base_log * level), digits of +-B/2."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, U64, size=(count, pp.in_dim + 1), dtype=np.uint64, endpoint=True)
    edges = np.concatenate([_edge_rows(pp.in_dim, pp.base_log * pp.level, rng), half_digit_rows(pp)])
    assert edges.shape[0] == N_EDGE
    n = min(count, N_EDGE)
    x[:n] = edges[:n]
    return x


def digit_set(pp, words):
    from oracle import oracle as O
    return {d for w in np.unique(words) for d in O.decompose(int(w), pp.base_log, pp.level)}


def check_digit_coverage(pp, lwes):
    """CPU-side: the inputs really hold the digits the sweep is about, so no seed passes a wrong digit split by
    luck.  +B/2 always; -B/2 wherever it exists (a one-level decomposition has no -B/2: the carry that makes
    it needs a level above, so there the most negative digit, -B/2 + 1, is required instead); at 2^16 a digit
    in 32640..32768, the range whose high byte would be +128."""
    B2 = 1 << (pp.base_log - 1)
    ds = digit_set(pp, lwes[:16, :pp.in_dim])
    assert B2 in ds
    assert (-B2 if pp.level > 1 else -B2 + 1) in ds
    if pp.base_log == 16:
        assert any(32640 <= d <= 32768 for d in ds)
        assert (-32768 if pp.level > 1 else -32767) in ds


@functools.lru_cache(maxsize=None)
def sweep_inputs(name):
    """-> (pp, opp, key, lwes) of one sweep case; built once, never modified."""
    fields, _ = SWEEP[name]
    pp, opp = make_params(*fields)
    seed = 1000 + sorted(SWEEP).index(name)
    lwes = synthetic_lwes(pp, max(ROW_COUNTS + (pp.lwe_per_glwe + 3,)), seed)
    if pp.level == 1:   # -B/2 + 1: state digit B/2 + 1 (carry), no level above to carry into
        lwes[N_EDGE, :pp.in_dim] = np.uint64((((1 << (pp.base_log - 1)) + 1) << (64 - pp.base_log)) & U64)
    lwes.setflags(write=False)
    return pp, opp, synthetic_key(pp, seed + 50), lwes


def row_counts(pp):
    return sorted(set(ROW_COUNTS + (pp.lwe_per_glwe + 3,)))


def read_t_budget():
    """PKS_T_BUDGET (bytes of T workspace per chunk of groups) from its definition in pks_api.cpp."""
    src = open(os.path.join(ROOT, "tfhe_amd", "csrc", "pks_api.cpp")).read()
    m = re.search(r"constexpr\s+size_t\s+PKS_T_BUDGET\s*=\s*(\d+)ull\s*<<\s*(\d+)\s*;", src)
    assert m, "PKS_T_BUDGET definition not found"
    return int(m.group(1)) << int(m.group(2))


CHUNK_FIELDS = (64, 2, 4096, 8, 1, 4096)   # one group's T = 4096 x 3 * 4096 x 8 B = 384 MiB: one group per chunk


def chunk_plan(pp, count):
    """pack_device's chunking, restated: (groups per chunk, rows per launch, launches)."""
    per_group = pp.lwe_per_glwe * pp.glwe_len * 8
    gpc = max(1, read_t_budget() // per_group)
    rows = min(count, gpc * pp.lwe_per_glwe)
    return gpc, rows, -(-count // rows)


def check_chunk_plan():
    """CPU-side: the chunk test's call spans exactly two chunks of one group each at the budget in the source."""
    pp, _ = make_params(*CHUNK_FIELDS)
    count = pp.lwe_per_glwe + 3
    assert read_t_budget() // (pp.lwe_per_glwe * pp.glwe_len * 8) == 1
    assert chunk_plan(pp, count) == (1, pp.lwe_per_glwe, 2)
    return pp, count


def _packer(pp, key, valu=False):
    if valu:
        os.environ["TFHE_HIP_PKS_VALU"] = "1"
    try:
        p = C.Packer(pp, 0)
    finally:
        if valu:
            del os.environ["TFHE_HIP_PKS_VALU"]
    try:
        return p.load_key(key)
    except Exception:
        p.close()
        raise


def _assert_groups_equal_oracle(oracle_mod, pp, opp, key, lwes, got, cache=None, tag=""):
    lpg = pp.lwe_per_glwe
    groups = -(-lwes.shape[0] // lpg)
    assert got.shape == (groups, pp.glwe_len), tag
    for g in range(groups):
        part = lwes[g * lpg:(g + 1) * lpg]
        ck = (g, part.shape[0])
        if cache is None or ck not in cache:
            ref = oracle_mod.pks_pack(opp, key, part)
            if cache is not None:
                cache[ck] = ref
        else:
            ref = cache[ck]
        bad = np.flatnonzero(got[g] != ref)
        assert bad.size == 0, f"{tag} group {g} of {groups}: {bad.size} of {ref.size} words differ, first at {bad[:4]}"


# ---- 1. parameter sweep ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SWEEP))
def test_sweep_vs_oracle(oracle_mod, name):
    """Every word of every output GLWE equals the oracle's, at every row count, on the GEMM the selection
    rule names for these parameters."""
    pp, opp, key, lwes = sweep_inputs(name)
    assert expected_path(pp) == SWEEP[name][1]
    check_digit_coverage(pp, lwes)
    packer = _packer(pp, key)
    try:
        cache = {}
        for count in row_counts(pp):
            got = packer.pack(lwes[:count])
            _assert_groups_equal_oracle(oracle_mod, pp, opp, key, lwes[:count], got, cache, f"{name} count {count}")
    finally:
        packer.close()


@pytest.mark.parametrize("name", ["mfma_k64_smallest", "mfma_k3_17_per_glwe", "mfma_base15"])
def test_sweep_forced_valu_vs_oracle(oracle_mod, name):
    """TFHE_HIP_PKS_VALU=1 at the matrix-core points: the VALU GEMM, its offset correction and the shift-sum at
    k = 3 and 17 LWEs per GLWE."""
    pp, opp, key, lwes = sweep_inputs(name)
    packer = _packer(pp, key, valu=True)
    try:
        for count in (65, 257):
            got = packer.pack(lwes[:count])
            _assert_groups_equal_oracle(oracle_mod, pp, opp, key, lwes[:count], got, None, f"{name} valu count {count}")
    finally:
        packer.close()


# ---- 2. both GEMMs at the production shape -----------------------------------------------------------------
def test_both_gemms_agree_at_preset(oracle_mod):
    """Preset parameters, synthetic random key, one full group + 300 with the edge rows in front: the
    matrix-core and the VALU GEMM give the same words everywhere; the first 8 LWEs of the partial second
    group, packed on their own, equal the oracle on both."""
    pp = C.PksParams.preset(C.PKS_PRESET_ML2048)
    opp = oracle_mod.pks_params(0)
    assert expected_path(pp) == "mfma"
    key = synthetic_key(pp, 77)
    lwes = synthetic_lwes(pp, 2048 + 300, 78)
    check_digit_coverage(pp, lwes)
    tail_ref = oracle_mod.pks_pack(opp, key, lwes[2048:2056])
    out = []
    for valu in (False, True):
        packer = _packer(pp, key, valu=valu)
        try:
            out.append(packer.pack(lwes))
            assert np.array_equal(packer.pack(lwes[2048:2056])[0], tail_ref), f"valu={valu}"
        finally:
            packer.close()
    assert out[0].shape == (2, pp.glwe_len)
    bad = np.argwhere(out[0] != out[1])
    assert bad.size == 0, f"{bad.shape[0]} words differ between the GEMMs, first at {bad[:4].tolist()}"


# ---- 3. chunk loop ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunk_case(oracle_mod):
    pp, count = check_chunk_plan()
    opp = make_params(*CHUNK_FIELDS)[1]
    key = synthetic_key(pp, 91)
    lwes = synthetic_lwes(pp, count, 92)
    lpg = pp.lwe_per_glwe
    # the full first group on the CPU: 1.9 s measured (4096 x 64 x 12288 multiply-adds), done once for both GEMMs
    ref = [oracle_mod.pks_pack(opp, key, lwes[:lpg]), oracle_mod.pks_pack(opp, key, lwes[lpg:])]
    return pp, key, lwes, ref


@pytest.mark.parametrize("valu", [False, True], ids=["mfma", "valu"])
def test_chunk_loop(chunk_case, valu):
    """lwe_per_glwe + 3 LWEs where the T budget holds one group: two launches, the second on the 3 left over.
    Both groups equal the oracle, and group 0 equals a single-group pack of the same LWEs."""
    pp, key, lwes, ref = chunk_case
    lpg = pp.lwe_per_glwe
    assert chunk_plan(pp, lwes.shape[0])[1:] == (lpg, 2)
    packer = _packer(pp, key, valu=valu)
    try:
        got = packer.pack(lwes)
        single = packer.pack(lwes[:lpg])
    finally:
        packer.close()
    assert got.shape == (2, pp.glwe_len)
    assert np.array_equal(got[1], ref[1])
    assert np.array_equal(got[0], single[0])
    assert np.array_equal(got[0], ref[0])


# ---- 4. workspace regrowth -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mfma_k64_smallest", "valu_K48"])
def test_workspace_regrowth(oracle_mod, name):
    """5, 300, then 5 LWEs on one context: the digit and T workspaces are freed and reallocated in between."""
    pp, opp, key, _ = sweep_inputs(name)
    lwes = synthetic_lwes(pp, 300, 555)
    packer = _packer(pp, key)
    try:
        for i, count in enumerate((5, 300, 5)):
            part = lwes[:count] if i < 2 else lwes[295:300]
            _assert_groups_equal_oracle(oracle_mod, pp, opp, key, part, packer.pack(part), None, f"{name} step {i}")
    finally:
        packer.close()


# ---- 5. ordering across streams --------------------------------------------------------------------------
# These pin the call patterns of the contract in include/tfhe_hip.h (tfhe_hip_pks_pack_async, tfhe_hip_pks_load_key).
# They do not prove the ordering: launches this small may finish before the next call arrives.  The ordering itself
# is the device slot's ws_begin / ws_end / ws_host_wait (host_common.h), shared with the other contexts.
SENTINEL = 0x5E5E5E5E5E5E5E5E
ORDER_CASES = ["mfma_k64_smallest", "valu_K48"]


class _AsyncPack:
    """Device input and a sentinel-filled output with two spare GLWEs for one pack_async call."""

    def __init__(self, pp, lwes):
        import torch
        dev = torch.device("cuda", 0)
        self.pp, self.lwes = pp, lwes
        self.groups = -(-lwes.shape[0] // pp.lwe_per_glwe)
        self.d_in = torch.from_numpy(np.ascontiguousarray(lwes).view(np.int64).copy()).to(dev)
        self.d_out = torch.full((self.groups + 2, pp.glwe_len), SENTINEL, dtype=torch.int64, device=dev)

    def issue(self, packer, stream):
        packer.pack_async(self.d_in, self.lwes.shape[0], self.d_out, stream)

    def check(self, oracle_mod, opp, key, tag):
        out = self.d_out.cpu().numpy().view(np.uint64)
        _assert_groups_equal_oracle(oracle_mod, self.pp, opp, key, self.lwes, out[:self.groups], None, tag)
        assert (out[self.groups:] == SENTINEL).all(), tag
        return out[:self.groups]


@pytest.mark.parametrize("name", ORDER_CASES)
def test_pack_stream_ordering(oracle_mod, name):
    """An async pack of 257 LWEs on a side stream, then AT ONCE, without a synchronisation, a host pack of 65 others;
    then the 257 and the 65 async on two side streams, back to back.  All four results equal the oracle."""
    import torch
    pp, opp, key, lwes = sweep_inputs(name)
    X, Y = lwes[:257], synthetic_lwes(pp, 65, 556)
    packer = _packer(pp, key)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        x1, x2, y2 = _AsyncPack(pp, X), _AsyncPack(pp, X), _AsyncPack(pp, Y)
        torch.cuda.synchronize()                    # uploads and sentinel fills
        x1.issue(packer, s1)
        got_y = packer.pack(Y)
        s1.synchronize()
        _assert_groups_equal_oracle(oracle_mod, pp, opp, key, Y, got_y, None, f"{name}: host pack behind an async call")
        x1.check(oracle_mod, opp, key, f"{name}: async pack with a host call behind it")
        x2.issue(packer, s1)
        y2.issue(packer, s2)
        s1.synchronize()
        s2.synchronize()
        x2.check(oracle_mod, opp, key, f"{name}: async pack on s1")
        y2.check(oracle_mod, opp, key, f"{name}: async pack on s2 behind s1")
    finally:
        packer.close()


@pytest.mark.parametrize("name", ORDER_CASES)
def test_regrow_behind_async_call(oracle_mod, name):
    """A fresh context: 5 LWEs async on one stream, at once 300 async on another (the workspaces are freed and
    reallocated behind the first call), then 5 on the first stream again.  All three equal the oracle."""
    import torch
    pp, opp, key, _ = sweep_inputs(name)
    lwes = synthetic_lwes(pp, 300, 555)
    packer = _packer(pp, key)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        calls = [(_AsyncPack(pp, lwes[:5]), s1), (_AsyncPack(pp, lwes), s2), (_AsyncPack(pp, lwes[295:300]), s1)]
        torch.cuda.synchronize()
        for call, st in calls:
            call.issue(packer, st)
        s1.synchronize()
        s2.synchronize()
        for i, (call, _) in enumerate(calls):
            call.check(oracle_mod, opp, key, f"{name} step {i}")
    finally:
        packer.close()


@pytest.mark.parametrize("name", ORDER_CASES)
def test_load_key_behind_async_call(oracle_mod, name):
    """An async pack of 257 LWEs under key A, at once load_key(B), then a host pack of the same LWEs: the async result
    is the oracle's under A, the host result the oracle's under B, and the two differ."""
    import torch
    pp, opp, key_a, lwes = sweep_inputs(name)
    key_b = synthetic_key(pp, 557)
    X = lwes[:257]
    packer = _packer(pp, key_a)
    try:
        s1 = torch.cuda.Stream()
        xa = _AsyncPack(pp, X)
        torch.cuda.synchronize()
        xa.issue(packer, s1)
        packer.load_key(key_b)
        got_b = packer.pack(X)
        s1.synchronize()
        got_a = xa.check(oracle_mod, opp, key_a, f"{name}: async pack under key A")
        _assert_groups_equal_oracle(oracle_mod, pp, opp, key_b, X, got_b, None, f"{name}: host pack under key B")
        assert not np.array_equal(got_a, got_b)
    finally:
        packer.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------
def test_refused_loads_leave_the_resident_key():
    """tfhe_hip_pks_load_key with a null context, null words and the lengths len - 1, len + 1 and 0: EINVAL each, and
    the pack under the resident key is what it was."""
    from tfhe_amd import _u64
    pp, _, key, lwes = sweep_inputs("mfma_k64_smallest")
    load = C._lib().tfhe_hip_pks_load_key
    words = np.ascontiguousarray(key.pksk)
    packer = _packer(pp, key)
    try:
        before = packer.pack(lwes[:65])
        assert load(None, _u64(words), words.size) == EINVAL
        assert load(packer._h, None, words.size) == EINVAL
        for wrong in (words.size - 1, words.size + 1, 0):
            assert load(packer._h, _u64(words), wrong) == EINVAL
        assert np.array_equal(packer.pack(lwes[:65]), before)
    finally:
        packer.close()
