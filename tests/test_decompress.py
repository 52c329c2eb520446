"""Decompression (tfhe-rs CompressedCiphertextList::get / DecompressionKey::unpack) without a GPU: the reference
recipe that tests/test_gpu_decompress.py compares the device against, checked here by decryption, plus the host
pieces of the product (list layout, argument checks that precede device work, the decompression key).

The reference is a composition of oracle functions: or_pks_extract -> the extraction formula (restated below, not
imported from the product) -> or_blind_rotate_fft / or_blind_rotate -> or_sample_extract_torus / or_sample_extract,
with a bootstrapping key from or_server_keygen(dprm, seed, post_packing_key, glwe_key, bsk, NULL), dprm = the compute
preset with n = out_k * out_N.

Settings of the message-level checks: 4-bit messages at Delta = 2^59 (half-step 2^58), inputs encrypted under the
compute GLWE key at the preset's glwe_noise_log2, packing keyswitch 2^4 x 3 with noise 2^-48.

The ABI check `out_k * out_N != n` needs a ctx, and a ctx needs a device: it is in the GPU contract test.
"""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

import tfhe_amd
from tfhe_amd import compression as C

SEED = 0x7F4E0001
PKS_SEED = 0x7F4E0D01
DK_SEED = 0x7F4E0D02
DELTA_LOG = 59  # 4-bit messages with one padding bit

# (compute preset, out_k, out_N, lwe_per_glwe, storage_log, count): the end-to-end shapes of the GPU test
E2E_SHAPES = [(3, 1, 64, 64, 12, 2 * 64 + 3), (3, 3, 32, 17, 26, 2 * 17 + 3),
              (2, 1, 64, 64, 12, 2 * 64 + 3), (2, 3, 32, 17, 26, 2 * 17 + 3)]
# the tfhe-rs-like shape: 4 x 256 into P-FHEVM-FFT (n = 1024); the rows compared word for word
WIDE_SHAPE = (3, 4, 256, 256, 12, 259)
WIDE_ROWS = (0, 1, 255, 256, 258)


def oracle():
    from oracle import oracle as O
    O.lib()
    return O


# ---- the reference rule -------------------------------------------------------------------------------------
def extract_rule(k, N, glwe, i):
    """Sample extraction at degree i of a native-torus GLWE ((k+1) x N): a'[cN + j] = a_c[i - j] for j <= i,
    -a_c[N + i - j] for j > i (mod 2^64); b' = body[i]."""
    g = np.asarray(glwe, dtype=np.uint64).reshape(k + 1, N)
    out = np.empty(k * N + 1, dtype=np.uint64)
    for c in range(k):
        for j in range(N):
            out[c * N + j] = g[c][i - j] if j <= i else np.uint64((-int(g[c][N + i - j])) % (1 << 64))
    out[k * N] = g[k][i]
    return out


def extract_rows(k, N, glwe, degrees):
    """extract_rule for several degrees at once -> (len(degrees), kN + 1); checked against it below."""
    g = np.asarray(glwe, dtype=np.uint64).reshape(k + 1, N)
    i = np.asarray(degrees, dtype=np.int64).reshape(-1, 1)
    src = i - np.arange(N, dtype=np.int64)[None, :]
    out = np.empty((i.shape[0], k * N + 1), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for c in range(k):
            v = g[c][src % N]
            out[:, c * N:(c + 1) * N] = np.where(src < 0, np.uint64(0) - v, v)
    out[:, k * N] = g[k][i[:, 0]]
    return out


def group_sizes(lpg, count):
    return [min(lpg, count - g) for g in range(0, count, lpg)]


def list_words(O, opp, count):
    L = O.lib()
    L.or_pks_packed_words.restype = ctypes.c_size_t
    return sum(L.or_pks_packed_words(ctypes.byref(opp), ctypes.c_uint32(b)) for b in group_sizes(opp.lwe_per_glwe, count))


def split_list(O, opp, packed, count):
    """The concatenated words of a list -> [(words of group g, bodies_g)]."""
    L = O.lib()
    L.or_pks_packed_words.restype = ctypes.c_size_t
    out, off = [], 0
    for b in group_sizes(opp.lwe_per_glwe, count):
        n = L.or_pks_packed_words(ctypes.byref(opp), ctypes.c_uint32(b))
        out.append((packed[off:off + n], b))
        off += n
    assert off == len(packed)
    return out


def unpack_extract_ref(O, opp, packed, count, rows=None):
    """or_pks_extract -> extract_rule for the rows asked for (default all): {row: LWE}."""
    rows = list(range(count) if rows is None else rows)
    groups, out = split_list(O, opp, packed, count), {}
    for g in sorted({q // opp.lwe_per_glwe for q in rows}):
        mine = [q for q in rows if q // opp.lwe_per_glwe == g]
        glwe = O.pks_extract(opp, np.ascontiguousarray(groups[g][0]), groups[g][1])
        lwes = extract_rows(opp.out_k, opp.out_N, glwe, [q % opp.lwe_per_glwe for q in mine])
        out.update(zip(mine, lwes))
    return out


def with_n(prm, n):
    d = type(prm).from_buffer_copy(prm)
    d.n = n
    return d


def rotation_keys(O, dprm, seed, lwe_key, glwe_key):
    """Oracle keys of a rotation-only context: the BSK of or_server_keygen with a NULL keyswitching key."""
    k = O.Keys.__new__(O.Keys)
    k.prm, k.seed = dprm, seed
    k.lwe_key = np.ascontiguousarray(lwe_key, dtype=np.uint64).copy()
    k.glwe_key = np.ascontiguousarray(glwe_key, dtype=np.uint64).copy()
    k.bsk = np.zeros(O.lib().or_bsk_len(ctypes.byref(dprm)), dtype=np.uint64)
    k.ksk, k._bsk_ntt, k.ms_zeros = None, None, None
    O.lib().or_server_keygen(ctypes.byref(dprm), ctypes.c_uint64(seed), O._p(k.lwe_key), O._p(k.glwe_key), O._p(k.bsk),
                             None)
    return k


def bootstrap_ref(O, dprm, keys, lwe, lut):
    """(accumulator, extracted LWE) of one ciphertext on the oracle of the parameter set's transform."""
    if dprm.transform == 1:
        acc = O.blind_rotate_fft(dprm, keys, lwe, lut)
        return acc, O.sample_extract_torus(dprm, acc)
    acc = O.blind_rotate(dprm, keys, lwe, lut)
    return acc, O.sample_extract(dprm, acc)


def identity_lut(O, N, msg_modulus=16):
    return O.lut_from_table(N, msg_modulus, list(range(msg_modulus)), (1 << 63) // msg_modulus)


def decode(phases):
    ph = np.asarray(phases, dtype=np.uint64)
    return ((ph + np.uint64(1 << (DELTA_LOG - 1))) >> np.uint64(DELTA_LOG)) & np.uint64(15)


class Case:
    """One decompression set-up: compute keys, packing keys, a compressed list of `count` 4-bit messages (packed by
    the oracle) and the oracle's decompression key."""

    def __init__(self, preset, out_k, out_N, lpg, w, count):
        O = oracle()
        self.O, self.count, self.preset = O, count, preset
        self.prm = O.params(preset)
        ck = O.Keys(self.prm, SEED, with_bsk=False, with_ksk=False)
        self.glwe_key = ck.glwe_key
        big = self.prm.k * self.prm.N
        self.fields = (big, out_k, out_N, 4, 3, lpg, w, -48)
        self.opp = O.PksParams(*self.fields)
        self.pp = C.PksParams(*self.fields)
        self.pk = O.PksKeys(self.opp, PKS_SEED, self.glwe_key)
        rng = np.random.default_rng(count * 131 + out_N)
        self.msgs = rng.integers(0, 16, count).astype(np.uint64)
        self.msgs[:4] = [0, 15, 8, 7][:min(4, count)]
        lwes = np.zeros((count, big + 1), dtype=np.uint64)
        m = self.msgs << np.uint64(DELTA_LOG)
        O.lib().or_lwe_encrypt(ctypes.c_uint32(big), O._p(self.glwe_key), ctypes.c_int32(self.prm.glwe_noise_log2),
                               ctypes.c_uint64(SEED + 1), ctypes.c_uint64(0), O._p(m), ctypes.c_size_t(count),
                               O._p(lwes))
        self.groups = []
        for g, b in enumerate(group_sizes(lpg, count)):
            glwe = O.pks_pack(self.opp, self.pk, lwes[g * lpg:g * lpg + b])
            self.groups.append((O.pks_compress(self.opp, glwe, b), b))
        self.packed = np.concatenate([p for p, _ in self.groups])
        self.dprm = with_n(self.prm, out_k * out_N)
        self.dkeys = rotation_keys(O, self.dprm, DK_SEED, self.pk.out_key, self.glwe_key)
        self._ref = {}

    def reference(self, rows, lut=None):
        """{row: decompressed LWE} by the oracle composition (identity LUT by default); cached per LUT."""
        O = self.O
        lut = identity_lut(O, self.prm.N) if lut is None else lut
        cache = self._ref.setdefault(lut.tobytes(), {})
        todo = [q for q in rows if q not in cache]
        for q, lwe in unpack_extract_ref(O, self.opp, self.packed, self.count, todo).items():
            cache[q] = bootstrap_ref(O, self.dprm, self.dkeys, lwe, lut)[1]
        return {q: cache[q] for q in rows}

    def phases(self, big_lwes):
        """b - <a, S> under the compute GLWE key."""
        O, dim = self.O, self.prm.k * self.prm.N
        cts = np.ascontiguousarray(big_lwes, dtype=np.uint64).reshape(-1, dim + 1)
        out = np.zeros(cts.shape[0], dtype=np.uint64)
        O.lib().or_lwe_phase(ctypes.c_uint32(dim), O._p(self.glwe_key), O._p(cts), ctypes.c_size_t(cts.shape[0]), O._p(out))
        return out


@lru_cache(maxsize=None)
def case(*shape):
    return Case(*shape)


# ---- tests -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", E2E_SHAPES, ids=lambda s: "p%d-%dx%d-%d-%d" % s[:5])
def test_oracle_recipe_decrypts_every_message(shape):
    """The condition under which the GPU test's message-level assertions mean anything: at each end-to-end shape the
    oracle composition returns every message, with the phase error under the half-step 2^58."""
    cs = case(*shape)
    ref = cs.reference(range(cs.count))
    ph = cs.phases(np.stack([ref[q] for q in range(cs.count)]))
    err = (ph - (cs.msgs << np.uint64(DELTA_LOG))).view(np.int64)
    print("worst phase error 2^%.1f" % np.log2(np.abs(err).max()))
    assert np.array_equal(decode(ph), cs.msgs)
    assert np.abs(err).max() < 1 << (DELTA_LOG - 1)


def test_oracle_recipe_decrypts_wide_shape_rows():
    """4 x 256 into P-FHEVM-FFT: the rows the GPU test compares word for word (first, second, last of a full group,
    first and last of the remainder group)."""
    cs = case(*WIDE_SHAPE)
    ref = cs.reference(WIDE_ROWS)
    ph = cs.phases(np.stack([ref[q] for q in WIDE_ROWS]))
    assert np.array_equal(decode(ph), cs.msgs[list(WIDE_ROWS)])


@pytest.mark.parametrize("fields,count", [((64, 1, 64, 4, 3, 64, 12, -48), 131), ((64, 3, 32, 4, 3, 17, 26, -48), 37),
                                          ((64, 1, 64, 4, 3, 5, 63, -48), 13), ((2048, 1, 2048, 14, 2, 2048, 26, -48), 2051),
                                          ((64, 1, 64, 4, 3, 64, 12, -48), 64), ((64, 1, 64, 4, 3, 64, 12, -48), 0)])
def test_list_words_is_the_sum_over_groups(fields, count):
    """packed_words of a concatenated list: lwe_per_glwe bodies in every group but the last, the remainder there;
    the product's list builder and the ABI's size check agree with it."""
    O = oracle()
    pp, opp = C.PksParams(*fields), O.PksParams(*fields)
    L = C._lib()
    sizes = group_sizes(pp.lwe_per_glwe, count)
    want = sum(L.tfhe_hip_pks_packed_words(ctypes.byref(pp), b) for b in sizes)
    assert want == list_words(O, opp, count)
    comp = [C.CompressedGlwe(pp, np.full(L.tfhe_hip_pks_packed_words(ctypes.byref(pp), b), g + 1, dtype=np.uint64), b)
            for g, b in enumerate(sizes)]
    packed, n = C.concat_list(pp, comp)
    assert (packed.size, n) == (want, count)
    # the size check precedes the null-ctx check, so its verdict is visible without a device
    for words, ok in ((want, True), (want + 1, False), (max(want, 1) - 1, want == 0)):
        rc = L.tfhe_hip_decompress(None, ctypes.byref(pp), None, words, count, None, 0, None, None)
        msg = L.tfhe_hip_last_error().decode()
        assert rc == -1
        assert ("null ctx" in msg) == ok and ("packed_words" in msg) == (not ok), (words, msg)


def test_concat_list_refuses_a_short_inner_group():
    pp = C.PksParams(64, 1, 64, 4, 3, 64, 12, -48)
    short = C.CompressedGlwe(pp, np.zeros(3, dtype=np.uint64), 5)
    with pytest.raises(ValueError):
        C.concat_list(pp, [short, short])


def test_abi_checks_before_device_work():
    """null ctx, invalid parameters, wrong packed_words (EINVAL) and out_N > 4096 (EUNSUPPORTED), on both forms of
    both entry points, with no device in the process."""
    L = C._lib()
    pp = C.PksParams(64, 1, 64, 4, 3, 64, 12, -48)
    words = L.tfhe_hip_pks_packed_words(ctypes.byref(pp), 3)
    buf = np.zeros(max(words, 65 * 3), dtype=np.uint64)
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    v = ctypes.c_void_p(buf.ctypes.data)

    def err(rc):
        return rc, L.tfhe_hip_last_error().decode()

    for rc, msg in (err(L.tfhe_hip_decompress(None, ctypes.byref(pp), p, words, 3, p, 1, None, p)),
                    err(L.tfhe_hip_decompress_async(None, ctypes.byref(pp), v, words, 3, v, 1, None, v, None)),
                    err(L.tfhe_hip_pks_unpack_extract(None, p, words, 3, p)),
                    err(L.tfhe_hip_pks_unpack_extract_async(None, v, words, 3, v, None))):
        assert rc == -1 and "null ctx" in msg, msg
    rc, msg = err(L.tfhe_hip_decompress(None, ctypes.byref(pp), p, words + 1, 3, p, 1, None, p))
    assert rc == -1 and "packed_words" in msg
    rc, msg = err(L.tfhe_hip_decompress(None, ctypes.byref(pp), p, words, 1 << 31, p, 1, None, p))
    assert rc == -1 and "too many" in msg
    rc, msg = err(L.tfhe_hip_decompress(None, None, p, words, 3, p, 1, None, p))
    assert rc == -1 and "invalid packing parameters" in msg
    bad = C.PksParams(64, 2, 32, 4, 3, 17, 26, -48)  # (k+1)N = 96: refused by the packing parameter check
    rc, msg = err(L.tfhe_hip_decompress(None, ctypes.byref(bad), p, words, 3, p, 1, None, p))
    assert rc == -1 and "invalid packing parameters" in msg
    wide = C.PksParams(64, 1, 8192, 4, 3, 64, 12, -48)
    ww = L.tfhe_hip_pks_packed_words(ctypes.byref(wide), 3)
    for f in (lambda: L.tfhe_hip_decompress(None, ctypes.byref(wide), p, ww, 3, p, 1, None, p),
              lambda: L.tfhe_hip_decompress_async(None, ctypes.byref(wide), v, ww, 3, v, 1, None, v, None)):
        rc, msg = err(f())
        assert rc == -5 and "4096" in msg, msg
    top = C.PksParams(64, 1, 4096, 4, 3, 3, 26, -48)  # the largest covered size passes on to the ctx check
    tw = L.tfhe_hip_pks_packed_words(ctypes.byref(top), 3)
    rc, msg = err(L.tfhe_hip_decompress(None, ctypes.byref(top), p, tw, 3, p, 1, None, p))
    assert rc == -1 and "null ctx" in msg
    for name in ("tfhe_hip_load_bsk", "tfhe_hip_load_bsk_device"):
        rc, msg = err(getattr(tfhe_amd.lib(), name)(None, None, 0))
        assert rc == -1 and "load_bsk" in msg
    L2 = tfhe_amd.lib()
    rc, msg = err(L2.tfhe_hip_bootstrap(None, p, 1, p, 1, None, p))
    assert rc == -1 and "bootstrap: null ctx" in msg


@pytest.mark.parametrize("preset,fields", [(3, (2048, 1, 64, 4, 3, 64, 12, -48)), (2, (1024, 3, 32, 4, 3, 17, 26, -48))])
def test_decompression_key_matches_oracle(preset, fields):
    """DecompressionKey's BSK (tfhe_hip_server_keygen_k with a null KSK) equals the oracle's byte for byte, and its
    .params are the compute parameters with n = out_k * out_N."""
    O = oracle()
    prm, cp = O.params(preset), tfhe_amd.Params.preset(preset)
    glwe_key = O.Keys(prm, SEED, with_bsk=False, with_ksk=False).glwe_key
    pp = C.PksParams(*fields)
    ppk = C.CompressionKey(pp, PKS_SEED, glwe_key, with_key=False).post_packing_key
    dk = C.DecompressionKey(cp, pp, ppk, glwe_key, DK_SEED)
    want = {f: getattr(cp, f) for f, _ in cp._fields_}
    want["n"] = pp.out_k * pp.out_N
    assert dk.params.as_dict() == want and cp.n != want["n"]
    ok = rotation_keys(O, with_n(prm, want["n"]), DK_SEED, ppk, glwe_key)
    assert dk.bsk.tobytes() == ok.bsk.tobytes()
    with pytest.raises(ValueError):
        C.DecompressionKey(cp, pp, ppk[:-1], glwe_key, DK_SEED)


def test_extract_rule_agrees_with_the_product_statement():
    """The rule restated above and the product's host statement (compression.extract_lwe) are the same function, at
    the degrees where everything / nothing is negated and in between."""
    pp = C.PksParams(64, 3, 32, 4, 3, 17, 26, -48)
    g = np.random.default_rng(4).integers(0, 2 ** 64, size=4 * 32, dtype=np.uint64)
    for i in (0, 1, 16, 31):
        assert np.array_equal(extract_rule(3, 32, g, i), C.extract_lwe(pp, g, i))
    # the vectorised form the references use is the rule, at every degree
    assert np.array_equal(extract_rows(3, 32, g, range(32)), np.stack([extract_rule(3, 32, g, i) for i in range(32)]))
    z = extract_rows(3, 32, g, [0, 31]).reshape(2, -1)
    with np.errstate(over="ignore"):
        assert np.array_equal(z[0, 1:32], (np.uint64(0) - g[:32][::-1])[:31])  # degree 0: every j > 0 negated
    assert np.array_equal(z[1, :32], g[:32][::-1])                             # degree N - 1: nothing negated
