"""Compression of squashed ciphertexts, the parts that need no GPU (tfhe_amd/csrc/client.cpp, sns_pks_api.cpp):
the CPU pack, the stored form and the key against the Python restatement of the rule (tests/sns_pks_ref.py),
decryption of valid encryptions within a derived bound, argument checks, and an ASan + UBSan run of the new host
code as a stand-alone program (tools/sanitize/sns_pks_san.cpp).  The device side: tests/test_gpu_sns_compression.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import sns_compression as SC

import sns_pks_ref as R
from conftest import ROOT

CPU_SETS = ("A", "B", "C")
CASES = [(n, c) for n in CPU_SETS for c in R.counts(R.make_params(n))]


def test_preset_and_key_length():
    p = SC.SnsPksParams.preset()
    assert (p.in_dim, p.out_k, p.out_N, p.base_log, p.level, p.lwe_per_glwe, p.storage_log, p.noise_log2) == \
        (4096, 6, 1024, 61, 1, 128, 128, -62)
    L = SC._lib()
    assert L.tfhe_hip_sns_pksk_len(ctypes.byref(p)) == 4096 * 1 * 7 * 2 * 1024     # 470 MB
    assert L.tfhe_hip_sns_pksk_len(None) == 0
    with pytest.raises(tfhe_amd.TfheError) as e:
        SC.SnsPksParams.preset(3)
    assert e.value.code == -1
    # an euint64 (32 blocks): ~2 MB of squashed LWEs against one partial GLWE of the stored form
    assert SC.packed_words(p, 128) * 8 == (6 * 1024 + 128) * 16


def test_reference_digits_recompose():
    """The restated decomposition itself: digits are balanced and recompose to the closest representable value."""
    rng = np.random.default_rng(1)
    for name in CPU_SETS:
        pp = R.make_params(name)
        b, L = pp.base_log, pp.level
        prec = b * L
        words = [int(lo) | (int(hi) << 64) for lo, hi in rng.integers(0, 2 ** 64, size=(50, 2), dtype=np.uint64)]
        for a in words + R.special_masks(pp):
            d = R.digits(a, b, L)
            assert all(-(1 << (b - 1)) <= x <= (1 << (b - 1)) for x in d)
            got = sum(x << (128 - b * (l + 1)) for l, x in enumerate(d))
            want = (((a >> (128 - prec - 1)) + 1) >> 1) << (128 - prec)
            assert (got - want) % (1 << 128) == 0
        tie = R.digits(1 << (127 - prec), b, L)          # half of the last kept bit rounds up
        assert tie[-1] == 1 and not any(tie[:-1])


@pytest.mark.parametrize("name,count", CASES)
def test_pack_host_equals_reference(name, count):
    pp, key = R.keys(name)
    for lwes, ref in R.case(name, count):
        got = SC.pack_host(pp, key.pksk, lwes)
        assert got.shape == ref.shape == (-(-count // pp.lwe_per_glwe), pp.out_k + 1, 2, pp.out_N)
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("name", CPU_SETS)
def test_stored_form_equals_reference(name):
    pp, key = R.keys(name)
    lpg = pp.lwe_per_glwe
    _, ref = R.case(name, lpg)[0]
    glwe = ref[0]
    for bodies in (1, 7, lpg):
        assert SC.packed_words(pp, bodies) == R.packed_words(pp, bodies) == \
            -(-(pp.out_k * pp.out_N + bodies) * pp.storage_log // 64)
        comp = SC.compress_glwe(pp, glwe, bodies)
        assert comp.packed.size == R.packed_words(pp, bodies) and comp.nbytes == 8 * comp.packed.size
        assert np.array_equal(comp.packed, R.compress(pp, glwe, bodies))
        back = comp.extract()
        assert np.array_equal(back, R.extract(pp, comp.packed, bodies))
        # extract(compress(x)) = x rounded to storage_log bits, unused body coefficients zero
        vals = R.stored_values(pp, glwe, bodies)
        w = R.planes_to_ints(back).reshape(-1)
        n = pp.out_k * pp.out_N + bodies
        assert [int(x) for x in w[:n]] == [(v << (128 - pp.storage_log)) & R.U128 for v in vals]
        assert not any(int(x) for x in w[n:])
    # the edge words of the switch: all ones rounds up and wraps to 0, the tie rounds up
    s = pp.storage_log
    edge = np.zeros((pp.out_k + 1) * pp.out_N, dtype=object)
    edge[:4] = [R.U128, (1 << (127 - s)) if s < 128 else 1, (1 << 127) - 1, 1 << 127]
    g = R.ints_to_planes(edge.reshape(pp.out_k + 1, pp.out_N))
    assert np.array_equal(SC.compress_glwe(pp, g, 1).packed, R.compress(pp, g, 1))


def test_stored_values_straddle_three_words():
    """storage_log 75 (set B): some value starts late enough in a word to end in the word after the next."""
    pp = R.make_params("B")
    n = pp.out_k * pp.out_N + pp.lwe_per_glwe
    assert any((i * 75) % 64 + 75 > 128 for i in range(n))


@pytest.mark.parametrize("name", CPU_SETS)
def test_keygen_rows_encrypt_the_key_bits(name):
    pp, key = R.keys(name)
    assert set(np.unique(key.post_packing_key)) <= {0, 1} and 0 < key.post_packing_key.sum() < key.post_packing_key.size
    rows = key.pksk.reshape(pp.in_dim, pp.level, pp.out_k + 1, 2, pp.out_N)
    bound = 8 * 2.0 ** (64 + pp.noise_log2)
    seen = set()
    for j in list(range(0, pp.in_dim, 7)) + [pp.in_dim - 1]:
        for l in range(pp.level):
            ph = SC.glwe_phase128(pp.out_k, pp.out_N, key.post_packing_key, rows[j, l])
            want = int(key.in_key[j]) << (128 - pp.base_log * (l + 1))
            assert abs(R.centered(ph[0] - want)) < bound, (j, l)
            assert max(abs(R.centered(x)) for x in ph[1:]) < bound, (j, l)
            seen.add(int(key.in_key[j]))
    assert seen == {0, 1}
    # the library's phase against the restated one, on one row
    assert SC.glwe_phase128(pp.out_k, pp.out_N, key.post_packing_key, rows[1, 0]) == \
        R.phase(pp, key.post_packing_key, rows[1, 0])


def test_keygen_deterministic_per_seed():
    pp, key = R.keys("A")
    again = SC.SquashedCompressionKey(pp, R.SEED, key.in_key)
    other = SC.SquashedCompressionKey(pp, R.SEED + 1, key.in_key)
    assert np.array_equal(again.pksk, key.pksk) and np.array_equal(again.post_packing_key, key.post_packing_key)
    assert not np.array_equal(other.pksk, key.pksk)
    assert not np.array_equal(other.post_packing_key, key.post_packing_key)
    fresh = SC.SquashedCompressionKey(pp, None, key.in_key)          # OS entropy
    assert not np.array_equal(fresh.pksk, key.pksk)
    no_key = SC.SquashedCompressionKey(pp, R.SEED, key.in_key, with_key=False)
    assert no_key.pksk is None and np.array_equal(no_key.post_packing_key, key.post_packing_key)


def decrypt_errors(pp, key, glwe, msgs, msg_modulus=16):
    """max |phase - delta m| over the used coefficients, max |phase| over the unused ones"""
    delta = (1 << 127) // msg_modulus
    ph = SC.glwe_phase128(pp.out_k, pp.out_N, key.post_packing_key, glwe)
    used = max(abs(R.centered(ph[i] - delta * int(m))) for i, m in enumerate(msgs))
    rest = max([abs(R.centered(x)) for x in ph[len(msgs):]] or [0])
    return used, rest


@pytest.mark.parametrize("name", CPU_SETS)
def test_valid_encryptions_decrypt_after_pack_and_after_the_stored_form(name):
    pp, key = R.keys(name)
    lpg, delta = pp.lwe_per_glwe, (1 << 127) // 16
    count = lpg + 3
    msgs = (np.arange(count) * 5 + 3) % 16
    lwes = R.encrypt(pp, key.in_key, msgs)
    glwes = SC.pack_host(pp, key.pksk, lwes)
    for g in range(2):
        m = msgs[g * lpg:(g + 1) * lpg]
        bound = R.error_bound(pp, len(m))
        assert bound < delta / 2                          # the check below cannot pass vacuously
        # before the stored form there is no storage rounding: the bound's last term only helps afterwards
        pre = bound - ((pp.out_k * pp.out_N + 1) * 2.0 ** (127 - pp.storage_log) if pp.storage_log < 128 else 0)
        used, rest = decrypt_errors(pp, key, glwes[g], m)
        assert used < pre and rest < pre, (g, used, rest, pre)
        comp = SC.compress_glwe(pp, glwes[g], len(m))
        used, _ = decrypt_errors(pp, key, comp.extract(), m)
        assert used < bound, (g, used, bound)
    comp = [SC.compress_glwe(pp, glwes[g], min(lpg, count - g * lpg)) for g in range(2)]
    assert np.array_equal(SC.decrypt_list(key, comp, 16), msgs)


INVALID = {
    "in_dim % 16": dict(in_dim=72), "in_dim 0": dict(in_dim=0), "out_k 0": dict(out_k=0),
    "out_N not a power of two": dict(out_N=96), "out_N < 32": dict(out_N=16, out_k=3, lwe_per_glwe=16),
    "(k+1)N % 64": dict(out_k=2, out_N=32), "base_log 1": dict(base_log=1), "base_log 64": dict(base_log=64),
    "level 0": dict(level=0), "prec 128": dict(base_log=32, level=4), "lwe_per_glwe 0": dict(lwe_per_glwe=0),
    "lwe_per_glwe > N": dict(lwe_per_glwe=33), "storage_log 1": dict(storage_log=1),
    "storage_log 129": dict(storage_log=129), "noise_log2 0": dict(noise_log2=0), "noise_log2 -64": dict(noise_log2=-64),
}


@pytest.mark.parametrize("what", sorted(INVALID))
def test_invalid_parameters_return_einval(what):
    """Every clause of the validity rule, refused by keygen, create, pack_host, compress and extract before any
    device work (create checks its parameters before it asks for a device)."""
    pp = R.make_params("A")
    for f, v in INVALID[what].items():
        setattr(pp, f, v)
    L = SC._lib()
    buf = np.zeros(1 << 16, dtype=np.uint64)
    u = tfhe_amd._u64(buf)
    h = ctypes.c_void_p()
    calls = (lambda: L.tfhe_hip_sns_pks_keygen(ctypes.byref(pp), 1, u, u, None),
             lambda: L.tfhe_hip_sns_pks_create(ctypes.byref(pp), 0, ctypes.byref(h)),
             lambda: L.tfhe_hip_sns_pks_pack_host(ctypes.byref(pp), u, u, 1, u),
             lambda: L.tfhe_hip_sns_pks_compress(ctypes.byref(pp), u, 1, u),
             lambda: L.tfhe_hip_sns_pks_extract(ctypes.byref(pp), u, 1, u))
    for call in calls:
        assert call() == -1, what
    assert not h.value


def test_valid_edges_of_the_rule_are_accepted():
    """The inclusive ends: base_log 2 and 63, the largest reachable precision 126 (127 is prime) as 63 x 2 and as
    2 x 63, storage_log 2 and 128, lwe_per_glwe 1 and N, noise_log2 -1 and -63."""
    in_key = np.ones(64, dtype=np.uint64)
    for fields in ((64, 1, 32, 63, 2, 1, 2, -1), (64, 1, 32, 2, 1, 32, 128, -63), (64, 1, 32, 2, 63, 32, 128, -62)):
        pp = SC.SnsPksParams(*fields)
        key = SC.SquashedCompressionKey(pp, 1, in_key, with_key=False)
        assert key.post_packing_key.size == pp.out_k * pp.out_N


def test_bad_buffers_and_counts_fail_cleanly():
    pp, key = R.keys("A")
    L = SC._lib()
    u = tfhe_amd._u64(np.zeros(1 << 14, dtype=np.uint64))
    P = ctypes.byref(pp)
    assert L.tfhe_hip_sns_pks_pack_host(P, u, u, 0, u) == 0                  # count == 0: nothing to do
    assert L.tfhe_hip_sns_pks_pack_host(P, None, None, 0, None) == 0
    assert L.tfhe_hip_sns_pks_pack_host(P, None, u, 1, u) == -1
    assert L.tfhe_hip_sns_pks_pack_host(P, u, None, 1, u) == -1
    assert L.tfhe_hip_sns_pks_pack_host(P, u, u, 1, None) == -1
    assert L.tfhe_hip_sns_pks_pack_host(P, u, u, 0x80000000, u) == -1
    assert L.tfhe_hip_sns_pks_compress(P, u, pp.out_N + 1, u) == -1
    assert L.tfhe_hip_sns_pks_extract(P, u, pp.out_N + 1, u) == -1
    assert L.tfhe_hip_sns_pks_compress(P, None, 1, u) == -1
    assert L.tfhe_hip_glwe_phase128(0, 32, u, u, u) == -1
    assert L.tfhe_hip_glwe_phase128(1, 32, None, u, u) == -1
    assert L.tfhe_hip_sns_pks_keygen(P, 1, None, u, None) == -1
    bad_key = np.full(pp.in_dim, 2, dtype=np.uint64)
    with pytest.raises(tfhe_amd.TfheError) as e:
        SC.SquashedCompressionKey(pp, 1, bad_key)
    assert e.value.code == -1
    # device entry points on a null ctx
    assert L.tfhe_hip_sns_pks_pack(None, u, 1, u) == -1
    assert L.tfhe_hip_sns_pks_pack_async(None, None, 1, None, None) == -1
    assert L.tfhe_hip_sns_pks_load_key(None, u, 1) == -1
    L.tfhe_hip_sns_pks_destroy(None)


def test_packer_without_gpu_raises_not_aborts():
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("GPU present: covered by the gpu tests")
    except ImportError:
        pass
    with pytest.raises(tfhe_amd.TfheError):
        SC.SquashedPacker(R.make_params("A"), 0)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_new_host_code_clean_under_asan_ubsan(tmp_path):
    """keygen, pack_host, compress, extract and the 128-bit phase at set A, plus a storage width that straddles
    words, as a stand-alone program built with -fsanitize=address,undefined (no Python, no preload)."""
    exe = str(tmp_path / "sns_pks_san")
    csrc = os.path.join(ROOT, "tfhe_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tools", "sanitize", "sns_pks_san.cpp"), os.path.join(csrc, "client.cpp"),
                    "-o", exe, "-pthread"], check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "SNS PKS SANITIZE OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
