"""Device-resident radix circuits (RadixCircuit(engine, device=...)) on the MI355X at the production fhEVM
parameters: the same operations on the same encrypted inputs as the host mode, bit for bit; no host-array entry
point on the way; wrap() / tensor(); and the reference KATs up to euint8 by decryption."""
import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import radix as R
from conftest import load_kats
from test_radix import _w, supported

pytestmark = pytest.mark.gpu

B = 3
DEVICE = "cuda:0"


def g_select_uint(c, cond, x, y):
    return R.RadixUint(c, (yield from R.g_select(c, cond, x.blocks, y.blocks)))


def inputs(w):
    rng = np.random.default_rng(100 + w)
    a = rng.integers(0, 1 << w, B, dtype=np.uint64)
    b = rng.integers(0, 1 << w, B, dtype=np.uint64)
    b[0] = a[0]
    s = np.array([1, w - 1, 6], dtype=np.uint64)
    cond = np.array([1, 0, 1], dtype=np.uint64)
    return a, b, s, cond


def run_ops(c, ck, w):
    """One run_many of every operation of the comparison -> {name: result}."""
    a, b, s, cond = inputs(w)
    nb = w // 2
    A = R.RadixUint.encrypt(c, ck, a, w, seed=0xD0 + w, stream0=0)
    Bv = R.RadixUint.encrypt(c, ck, b, w, seed=0xD0 + w, stream0=B * nb)
    S = R.RadixUint.encrypt(c, ck, s, w, seed=0xD0 + w, stream0=2 * B * nb)
    C = c._ingest(ck.encrypt(cond, R.SPACE, 0xD0 + w, 3 * B * nb))
    seeds = [[0x5EED0000 + w, 1], [2, 3], [4, 5]]
    ops = {"add": R.fhevm_op(c, "add", A, Bv), "sub": R.fhevm_op(c, "sub", A, Bv), "neg": R.fhevm_op(c, "neg", A),
           "not": R.fhevm_op(c, "not", A), "mul": R.fhevm_op(c, "mul", A, Bv), "lt": R.fhevm_op(c, "lt", A, Bv),
           "eq": R.fhevm_op(c, "eq", A, Bv), "max": R.fhevm_op(c, "max", A, Bv), "shl 1": R.fhevm_op(c, "shl", A, 1),
           "shl 3": R.fhevm_op(c, "shl", A, 3), "rotr 5": R.fhevm_op(c, "rotr", A, 5), "shr enc": R.fhevm_op(c, "shr", A, S),
           "div 7": R.fhevm_op(c, "div", A, 7), "rem 1000": R.fhevm_op(c, "rem", A, 1000),
           "select": g_select_uint(c, C, A, Bv), "rand": R.fhevm_rand(c, "rand", seeds, w),
           "rand_bounded": R.fhevm_rand(c, "randBounded", seeds, w, 1 << (w - 3))}
    return dict(zip(ops, c.run_many(list(ops.values()))))


def host_words(r):
    return r.to_host() if isinstance(r, R.RadixUint) else np.asarray(r)


def check_values(ck, w, res):
    a, b, s, cond = inputs(w)
    m = (1 << w) - 1
    M = np.uint64(m)
    ai = [int(x) for x in a]
    d1000 = 1000 % (1 << w)
    want = {"add": (a + b) & M, "sub": (a - b) & M, "neg": (np.uint64(0) - a) & M, "not": ~a & M, "mul": (a * b) & M,
            "max": np.maximum(a, b), "shl 1": (a << np.uint64(1)) & M, "shl 3": (a << np.uint64(3)) & M,
            "rotr 5": np.array([((x >> 5) | (x << (w - 5))) & m for x in ai], dtype=np.uint64),
            "shr enc": a >> (s % np.uint64(w)), "div 7": a // np.uint64(7), "rem 1000": a % np.uint64(d1000),
            "select": np.where(cond == 1, a, b)}
    for name, v in want.items():
        np.testing.assert_array_equal(res[name].decrypt(ck), v, err_msg=f"w = {w}: {name}")
    np.testing.assert_array_equal(ck.decrypt(host_words(res["lt"]), R.SPACE).astype(bool), a < b)
    np.testing.assert_array_equal(ck.decrypt(host_words(res["eq"]), R.SPACE).astype(bool), a == b)
    assert res["rand"].width == w and res["rand_bounded"].width == w
    assert np.all(res["rand_bounded"].decrypt(ck) < np.uint64(1 << (w - 3)))


@pytest.fixture(scope="module")
def host_results(fhevm_fft_engine, fhevm_fft_keys):
    """Host mode's results per width, computed once (before any test patches the host entry points)."""
    ck, _ = fhevm_fft_keys
    out = {}
    for w in (8, 32):
        c = R.RadixCircuit(fhevm_fft_engine)
        res = run_ops(c, ck, w)
        cm = R.RadixCircuit(fhevm_fft_engine, many_lut=True)
        a, b, _, _ = inputs(w)
        A = R.RadixUint.encrypt(cm, ck, a, w, seed=0xD0 + w, stream0=0)
        Bv = R.RadixUint.encrypt(cm, ck, b, w, seed=0xD0 + w, stream0=B * (w // 2))
        res["add many"] = cm.run(R.fhevm_op(cm, "add", A, Bv))
        out[w] = ({k: host_words(v) for k, v in res.items()}, (c.pbs_count, c.launches), (cm.pbs_count, cm.launches))
    return out


def device_against_host(eng, ck, w, host_results):
    words, counts, counts_many = host_results[w]
    c = R.RadixCircuit(eng, device=DEVICE)
    res = run_ops(c, ck, w)
    for name, r in res.items():
        assert isinstance(r.blocks if isinstance(r, R.RadixUint) else r, R.LinBlocks), name
        np.testing.assert_array_equal(host_words(r), words[name], err_msg=f"w = {w}: {name}")
    assert (c.pbs_count, c.launches) == counts
    assert c.max_terms <= 5
    check_values(ck, w, res)
    cm = R.RadixCircuit(eng, many_lut=True, device=DEVICE)
    a, b, _, _ = inputs(w)
    A = R.RadixUint.encrypt(cm, ck, a, w, seed=0xD0 + w, stream0=0)
    Bv = R.RadixUint.encrypt(cm, ck, b, w, seed=0xD0 + w, stream0=B * (w // 2))
    add = cm.run(R.fhevm_op(cm, "add", A, Bv))
    np.testing.assert_array_equal(add.to_host(), words["add many"])
    np.testing.assert_array_equal(add.decrypt(ck), (a + b) & np.uint64((1 << w) - 1))
    assert (cm.pbs_count, cm.launches) == counts_many


# ---- 7. device mode against host mode -----------------------------------------------------------------------------
@pytest.mark.parametrize("w", [8, 32])
def test_device_mode_equals_host_mode(fhevm_fft_engine, fhevm_fft_keys, host_results, w):
    device_against_host(fhevm_fft_engine, fhevm_fft_keys[0], w, host_results)


# ---- 8. no host entry points ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [8, 32])
def test_device_mode_uses_no_host_entry_point(fhevm_fft_engine, fhevm_fft_keys, host_results, monkeypatch, w):
    def refuse(name):
        def f(self, *args, **kwargs):
            raise AssertionError(f"Engine.{name} (host arrays) called by a device-resident circuit")
        return f

    for name in ("pbs", "pbs_many", "oprf"):
        monkeypatch.setattr(tfhe_amd.Engine, name, refuse(name))
    with pytest.raises(AssertionError):
        fhevm_fft_engine.pbs(None, None)
    device_against_host(fhevm_fft_engine, fhevm_fft_keys[0], w, host_results)


# ---- 9. wrap() and tensor() -----------------------------------------------------------------------------------------
def test_wrap_and_tensor(fhevm_fft_engine, fhevm_fft_keys):
    import torch
    ck, _ = fhevm_fft_keys
    w, nb = 8, 4
    a, b, _, _ = inputs(w)
    c = R.RadixCircuit(fhevm_fft_engine, device=DEVICE)
    cts = [ck.encrypt(R.RadixUint._digits(v, w).reshape(-1), R.SPACE, 0x77A9, k * B * nb).reshape(B, nb, -1)
           for k, v in enumerate((a, b))]
    tensors = [torch.from_numpy(ct.view(np.int64)).to(DEVICE) for ct in cts]
    A, Bv = (R.RadixUint(c, c.wrap(t)) for t in tensors)
    assert A.blocks.shape == (B, nb, 2049)
    assert A.tensor().data_ptr() == tensors[0].data_ptr()      # an untouched value is its buffer, not a copy
    s = c.run(R.fhevm_op(c, "add", A, Bv))
    np.testing.assert_array_equal(s.decrypt(ck), (a + b) & np.uint64(255))
    t = s.tensor()
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and tuple(t.shape) == (B, nb, 2049)
    np.testing.assert_array_equal(t.cpu().numpy().view(np.uint64), s.to_host())
    # a value that is still a linear map (not: 3 - a) materialises through the kernel
    n = c.run(R.fhevm_op(c, "not", A))
    want = (np.uint64(0) - cts[0]).astype(np.uint64)
    want[..., -1] += np.uint64(3 * R.DELTA)
    np.testing.assert_array_equal(n.tensor().cpu().numpy().view(np.uint64), want)
    with pytest.raises(ValueError):
        c.wrap(tensors[0][..., :-1])
    with pytest.raises(ValueError):
        R.RadixCircuit(fhevm_fft_engine).wrap(tensors[0])


# ---- 10. the reference KATs up to euint8 ----------------------------------------------------------------------------
def test_radix_kats_device_mode(fhevm_fft_engine, fhevm_fft_keys):
    ck, _ = fhevm_fft_keys
    kats = [k for k in load_kats(max_width=8) if supported(k)]
    assert len(kats) > 100 and any(k["result_type"] == "ebool" for k in kats)
    c = R.RadixCircuit(fhevm_fft_engine, device=DEVICE)
    ops, stream = [], 0
    for k in kats:
        args = []
        for t, v in zip(k["types"], k["args"]):
            if t.startswith("e"):
                w = _w(t)
                args.append(R.RadixUint.encrypt(c, ck, [v], w, seed=0x5AD1, stream0=stream))
                stream += w // 2
            else:
                args.append(int(v))
        ops.append(R.fhevm_op(c, k["op"], *args))
    res = c.run_many(ops)
    bad = []
    for k, r in zip(kats, res):
        if k["result_type"] == "ebool":
            got = int(ck.decrypt(host_words(r), R.SPACE)[0])
            ok = got == int(bool(k["expect"]))
        else:
            got = int(r.decrypt(ck)[0])
            ok = got == k["expect"]
        if not ok:
            bad.append((k["source"], k["op"], k["types"], k["args"], k["expect"], got))
    assert not bad, f"{len(bad)} of {len(kats)} failed: {bad[:5]}"
    assert c.launches <= 40
