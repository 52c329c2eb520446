"""Encrypted matrix x clear matrix on the device (tfhe_amd/csrc/matmul.hip, matmul_api.cpp, tfhe_amd/matmul.py):

1. the expand kernel against the host expand;
2. the dot kernel, bit-exact against the numpy restatement (tests/matmul_ref.py) on full-range inputs, at the smallest
   shapes that reach each seam of the tiling;
3. an independent structure check against compression.extract_lwe;
4. the device chain against the CPU chain, word for word on the compressed output;
5. the reference's message-level criterion on the decrypted result;
6. the ordering contract of the context.

Every comparison of ciphertext words is an integer equality."""
import functools

import numpy as np
import pytest

import matmul_ref as REF
from tfhe_amd import compression as C
from tfhe_amd import matmul as MM

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
SENTINEL = 0x5E5E5E5E5E5E5E5E


def full_range(rng, shape):
    return rng.integers(0, U64, size=shape, dtype=np.uint64, endpoint=True)


# ---- 1. expand ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [39, 33, 64])
@pytest.mark.parametrize("N", [64, 2048])
def test_expand_kernel_equals_host_expand(N, w):
    """G = 3 seeded GLWEs with arbitrary stored bits: masks (csprng.hip) and unpacked bodies equal the host's."""
    mp = MM.MatmulParams(N, 20, w, -48)
    rng = np.random.default_rng(100 + N + w)
    seeds, packed = full_range(rng, (3, 2)), full_range(rng, (3, mp.body_words))
    with MM.MatMul(mp, None, 0) as mm:
        got = mm.expand(seeds, packed)
    want = MM.expand_host(mp, seeds, packed)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{bad.shape[0]} words differ, first at {bad[:4].tolist()}"


# ---- 2. dot, bit-exact -------------------------------------------------------------------------------------------
# name -> (N, R, K, C, col_stride)
DOT_SHAPES = {
    "tiles_4i_ragged_kblock_ragged_ctile": (256, 2, 259, 67, 67),
    "one_of_everything": (64, 1, 1, 1, 1),
    "preset_N_one_block": (2048, 1, 2048, 5, 5),
    "col_stride_above_C": (64, 2, 64, 3, 5),
}


@functools.lru_cache(maxsize=None)
def dot_inputs(name):
    """Random full-range u64 GLWEs (no valid encryption is needed; full-range words expose any carry or sign slip) and
    int32 weights over the full range with the special values planted -> (mp, glwes, W, reference); built once."""
    N, R, K, Cc, _ = DOT_SHAPES[name]
    rng = np.random.default_rng(200 + sorted(DOT_SHAPES).index(name))
    glwes = full_range(rng, (R, -(-K // N), 2, N))
    W = REF.plant_weights(rng.integers(-2 ** 31, 2 ** 31, size=(K, Cc), dtype=np.int64))
    ref = REF.dot_closed(glwes, W, N)
    for a in (glwes, W, ref):
        a.setflags(write=False)
    return MM.MatmulParams(N, 20, 39, -48), glwes, W, ref


@pytest.mark.parametrize("name", list(DOT_SHAPES))
def test_dot_kernel_equals_restatement(name):
    mp, glwes, W, ref = dot_inputs(name)
    R, Cc, stride = DOT_SHAPES[name][1], DOT_SHAPES[name][3], DOT_SHAPES[name][4]
    if name != "one_of_everything":
        assert {int(x) for x in np.unique(W)} >= set(REF.SPECIAL_WEIGHTS)
    out = np.full((R, stride, mp.N + 1), SENTINEL, dtype=np.uint64)
    with MM.MatMul(mp, None, 0) as mm:
        mm.dot(mm.clear_matrix(W), glwes, col_stride=stride, out=out)
    bad = np.argwhere(out[:, :Cc] != ref)
    assert bad.size == 0, f"{name}: {bad.shape[0]} of {ref.size} words differ, first at (r, c, i) = {bad[:4].tolist()}"
    assert (out[:, Cc:] == SENTINEL).all(), f"{name}: the LWEs past C were written"


# ---- 3. structure ------------------------------------------------------------------------------------------------
def test_unit_columns_extract_single_coefficients():
    """W[t][c] = 1 for (t, c) in (0, 0), (1, 1), (N - 1, 2), K = N: output LWE c is the sample extraction of
    coefficient t, as compression.extract_lwe computes it."""
    N = 256
    mp = MM.MatmulParams(N, 20, 39, -48)
    pp = C.PksParams(N, 1, N, 14, 2, N, 26, -48)
    glwe = full_range(np.random.default_rng(300), (2, N))
    ts = (0, 1, N - 1)
    W = np.zeros((N, len(ts)), dtype=np.int64)
    for c, t in enumerate(ts):
        W[t, c] = 1
    with MM.MatMul(mp, None, 0) as mm:
        out = mm.dot(mm.clear_matrix(W), glwe.reshape(1, 1, 2, N))
    for c, t in enumerate(ts):
        assert np.array_equal(out[0, c], C.extract_lwe(pp, glwe, t)), f"coefficient {t}"


# ---- 4 / 5. the chain --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_chain():
    """The chain case on the device: one multiply call, one with the row chunk forced to 1, and a second matrix
    resident on the same context."""
    case = REF.chain_case()
    packer = C.Packer(case.pp, 0)
    try:
        packer.load_key(case.pkey.compression_key)
        with MM.MatMul(case.mp, packer, 0) as mm:
            w1, w2 = mm.clear_matrix(case.W), mm.clear_matrix(case.W2)
            assert mm._rows_per_chunk(REF.CHAIN_R, 512) == REF.CHAIN_R
            whole = mm.multiply(case.enc, w1)
            mm.rows_per_chunk = 1
            assert mm._rows_per_chunk(REF.CHAIN_R, 512) == 1
            by_row = mm.multiply(case.enc, w1)
            second = mm.multiply(case.enc, w2)
    finally:
        packer.close()
    return case, whole, by_row, second


def test_device_chain_equals_cpu_chain(device_chain):
    """N = 256, R = 2, K = 259, C = 261: two GLWE groups per row with 5 bodies in the last; every compressed word
    equals the CPU chain's (host expand, host dot, the oracle's packing keyswitch, host compression)."""
    case, whole, by_row, second = device_chain
    assert [[cg.bodies for cg in row] for row in whole] == [[256, 5], [256, 5]]
    REF.assert_results_equal(whole, case.cpu_result, "one multiply call")
    REF.assert_results_equal(by_row, case.cpu_result, "row chunk forced to 1")
    REF.assert_results_equal(second, case.cpu_result2, "second resident matrix")


def test_device_chain_decrypts_to_the_product(device_chain):
    """The reference's own criterion (ml/extensions/tests/test_matmul.py:64-186, conftest.py:7-8): with bits_reserved =
    bit width of max |X.W| + 1, the decrypted values agree with X.W on the 12 most significant bits, the shift computed
    as the reference computes it, on all but at most 1 % of the entries."""
    case, whole, _, _ = device_chain
    got = MM.decrypt_matrix(whole, case.pkey, REF.CHAIN_C)
    assert got.shape == case.expected.shape and got.dtype == np.int64
    bad = REF.msb_mismatches(got, case.expected, case.width)
    print(f"bit width {case.width}, {bad} of {got.size} entries differ on the 12 MSBs, max |error| "
          f"{np.abs(got - case.expected).max()}")
    assert bad <= got.size // 100


# ---- 6. ordering -------------------------------------------------------------------------------------------------
# As the ordering tests of tests/test_gpu_pks_params.py, this pins the call pattern of the contract in
# include/tfhe_hip.h; launches this small may finish before the next call arrives.  The ordering itself is the device
# slot's ws_begin / ws_end / ws_host_wait (host_common.h).
def test_dot_stream_ordering_and_destroy_in_flight():
    """Two dot_async calls on different streams with no synchronisation between them, then the matrix and the context
    are destroyed with the work still in flight (destroy waits); both results equal the restatement and the LWEs past
    C keep the sentinel."""
    import torch
    name = "tiles_4i_ragged_kblock_ragged_ctile"
    mp, glwes, W, ref = dot_inputs(name)
    _, R, _, Cc, _ = DOT_SHAPES[name]
    stride = Cc + 2
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(glwes.view(np.int64).copy()).to(dev)
    outs = [torch.full((R, stride, mp.N + 1), SENTINEL, dtype=torch.int64, device=dev) for _ in range(2)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()                     # uploads and sentinel fills
    mm = MM.MatMul(mp, None, 0)
    try:
        clear = mm.clear_matrix(W)
        mm.dot_async(clear, d_in, R, stride, outs[0], s1)
        mm.dot_async(clear, d_in, R, stride, outs[1], s2)
    finally:
        mm.close()
    s1.synchronize()
    s2.synchronize()
    for i, o in enumerate(outs):
        got = o.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:, :Cc], ref), f"call {i}"
        assert (got[:, Cc:] == SENTINEL).all(), f"call {i}"
