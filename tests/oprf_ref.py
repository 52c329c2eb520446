"""Oblivious pseudo-random ciphertexts (fhEVM rand / randBounded) restated in numpy from the conventions in
include/tfhe_hip.h (not from the C++): the staircase LUT, the block seeds of a request, the value a row must decrypt
to, and the CPU-oracle route of one row.  Also the parameter pairs, seeds and small key sets shared by
tests/test_oprf.py (CPU) and tests/test_gpu_oprf.py (device).

The seeded mask stream itself is tests/test_seeded.py's subject (``tfhe_hip_csprng_words``, pinned to FIPS-197
there); this helper reads it through ``stream_words``."""
import ctypes
import functools

import numpy as np

import tfhe_amd
import test_decompress as TD

M64 = 1 << 64
PAIRS = ((1, 5), (2, 5), (4, 5), (1, 3))       # (random_bits, full_bits)
KEY_SEED = 0x0F2F0001
PARENT = (0x0F2F0002, 0)
BSK_SEED = 0x0F2F0003


def lut_oprf(N, random_bits, full_bits):
    """lut[x] = (2 floor(x / (2N/p)) + 1) delta/2, post_add = (p - 1) delta/2"""
    p, half = 1 << random_bits, 1 << (63 - full_bits)
    box = 2 * N // p
    lut = np.array([(2 * (x // box) + 1) * half % M64 for x in range(N)], dtype=np.uint64)
    return lut, (p - 1) * half % M64


def stream_words(seed, first, count):
    s = np.array([int(seed[0]) % M64, int(seed[1]) % M64], dtype=np.uint64)
    out = np.zeros(count, dtype=np.uint64)
    tfhe_amd._check(tfhe_amd.lib().tfhe_hip_csprng_words(tfhe_amd._u64(s), first, count, tfhe_amd._u64(out)))
    return out


def aes_stream_words(seed, count):
    """The first `count` words of the seed's stream from the AES definition: key = the seed's 16 bytes little
    endian, block b = AES(b as a little-endian counter), the stream starts at byte 1."""
    key = (int(seed[0]) | int(seed[1]) << 64).to_bytes(16, "little")
    out = ctypes.create_string_buffer(16)
    blocks = b""
    for b in range((8 * count + 1 + 15) // 16):
        tfhe_amd._check(tfhe_amd.lib().tfhe_hip_aes128_block(key, b.to_bytes(16, "little"), out))
        blocks += out.raw
    return np.frombuffer(blocks[1:1 + 8 * count], dtype="<u8").astype(np.uint64)


def block_seeds(parent, count):
    """block j: (lo, hi) = words (2j, 2j + 1) of the parent's stream"""
    return stream_words(parent, 0, 2 * count).reshape(count, 2)


def masks_of(seeds, n):
    return np.stack([stream_words(s, 0, n) for s in np.asarray(seeds, dtype=np.uint64).reshape(-1, 2)])


def rotation_index(masks, lwe_key, N):
    """x = (-sum a~_i s_i) mod 2N, a~ the standard modulus switch of the mask"""
    from oracle import oracle as O
    sw = O.mod_switch(np.asarray(masks, dtype=np.uint64), 2 * N).astype(np.int64)
    return (-(sw * np.asarray(lwe_key, dtype=np.int64)[None, :]).sum(axis=1)) % (2 * N)


def predict(masks, lwe_key, N, random_bits):
    """The value v (of v * delta) each row encrypts."""
    x = rotation_index(masks, lwe_key, N)
    p = 1 << random_bits
    box = 2 * N // p
    return np.where(x < N, x // box + p // 2, p // 2 - 1 - (x - N) // box).astype(np.int64)


def predict_gate(masks, lwe_key, N):
    """gate encoding: the bit is true iff x < N"""
    return rotation_index(masks, lwe_key, N) < N


def decode(phases, full_bits):
    """closest multiple of delta = 2^(64 - full_bits) -> (value, |phase error|)"""
    sh = 64 - full_bits
    ph = np.asarray(phases, dtype=np.uint64)
    v = ((ph + np.uint64(1 << (sh - 1))) >> np.uint64(sh)).astype(np.int64) % (1 << full_bits)
    err = (ph - (v.astype(np.uint64) << np.uint64(sh))).astype(np.int64)
    return v, np.abs(err)


# ---- key sets at a small n ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_keys(preset, n, full=False):
    """(oracle params at n, oracle keys) of `preset` with the small key cut to n: order 1 (KS -> PBS) a rotation-only
    set (BSK alone) unless `full`, order 0 the full server keys."""
    from oracle import oracle as O
    prm = O.params(preset)
    dprm = TD.with_n(prm, n)
    glwe_key = O.Keys(prm, KEY_SEED, with_bsk=False, with_ksk=False).glwe_key
    lwe_key = np.random.default_rng(1000 * preset + n).integers(0, 2, n).astype(np.uint64)
    if prm.order == 1 and not full:
        return dprm, TD.rotation_keys(O, dprm, BSK_SEED, lwe_key, glwe_key)
    return dprm, O.Keys.from_secret(dprm, BSK_SEED, lwe_key, glwe_key)


def product_side(preset, n, full=False):
    """(product params at n, ClientKey, ServerKey without modulus-switch zeros) of small_keys(preset, n, full)"""
    _, keys = small_keys(preset, n, full)
    params = TD.with_n(tfhe_amd.Params.preset(preset), n)
    ck = tfhe_amd.ClientKey(params, None, keys.lwe_key, keys.glwe_key)
    return params, ck, tfhe_amd.ServerKey(params, keys.bsk, keys.ksk, None)


def oracle_rows(dprm, keys, masks, luts, post_adds, lut_index):
    """The oracle route, row by row: order 1 blind rotation + sample extraction + post-add on (mask, 0); order 0 the
    full PBS without noise reduction + post-add.  -> rows x (io_dim + 1)"""
    from oracle import oracle as O
    masks = np.asarray(masks, dtype=np.uint64)
    cts = np.concatenate([masks, np.zeros((masks.shape[0], 1), dtype=np.uint64)], axis=1)
    luts = np.asarray(luts, dtype=np.uint64).reshape(-1, dprm.N)
    idx = np.zeros(masks.shape[0], dtype=np.uint32) if lut_index is None else np.asarray(lut_index, dtype=np.uint32)
    if dprm.order == 1:
        out = np.stack([TD.bootstrap_ref(O, dprm, keys, cts[q], luts[idx[q]])[1] for q in range(cts.shape[0])])
    else:
        out = O.pbs_batch_fft(dprm, keys, cts, luts, idx, ms=False)
    post = np.array([int(v) % M64 for v in post_adds], dtype=np.uint64)
    with np.errstate(over="ignore"):
        out[:, -1] += post[idx]
    return out


def out_phase(dprm, keys, rows):
    key, dim = (keys.lwe_key, dprm.n) if dprm.order == 0 else (keys.glwe_key, dprm.k * dprm.N)
    return keys.phase(rows, key, dim)


# ---- cleartext doubles of Engine.oprf: trivial blocks / bits of `predict` under a fixed key ----------------------
class ClearOprfEngine:
    """``oprf`` returns noise-free rows (0, ..., 0, body) whose body is what the real rows decrypt to under
    ``lwe_key``: v * delta for a staircase LUT (random_bits and delta read back from the LUT and its post-add), the
    gate encoding +-1/8 for the constant LUT."""

    def __init__(self, n=918, N=2048, order=1, dim=None, seed=7):
        from types import SimpleNamespace
        self.params = SimpleNamespace(k=1, N=N, n=n, order=order)
        self.dim = dim if dim is not None else (N + 1 if order == 1 else n + 1)
        self.lwe_key = np.random.default_rng(seed).integers(0, 2, n).astype(np.uint64)
        self.calls = []

    def gate_lut(self):
        return tfhe_amd.lut_constant(self.params.N, tfhe_amd.MU)

    def oprf(self, seeds, luts, post_adds, lut_index=None):
        seeds = np.asarray(seeds, dtype=np.uint64).reshape(-1, 2)
        luts = np.asarray(luts, dtype=np.uint64).reshape(-1, self.params.N)
        idx = np.zeros(seeds.shape[0], dtype=np.int64) if lut_index is None else np.asarray(lut_index, dtype=np.int64)
        self.calls.append(seeds.shape[0])
        masks = masks_of(seeds, self.params.n)
        out = np.zeros((seeds.shape[0], self.dim), dtype=np.uint64)
        for l in range(luts.shape[0]):
            sel = idx == l
            half = int(luts[l, 0])                          # delta / 2 (the gate LUT: 1/8)
            post = int(post_adds[l]) % M64
            if post == 0:
                assert np.array_equal(luts[l], tfhe_amd.lut_constant(self.params.N, tfhe_amd.MU))
                bits = predict_gate(masks[sel], self.lwe_key, self.params.N)
                out[sel, -1] = np.where(bits, np.uint64(tfhe_amd.MU), np.uint64(M64 - tfhe_amd.MU))
                continue
            p = post // half + 1
            rb = p.bit_length() - 1
            assert p == 1 << rb and np.array_equal(luts[l], lut_oprf(self.params.N, rb, 63 - half.bit_length() + 1)[0])
            v = predict(masks[sel], self.lwe_key, self.params.N, rb).astype(np.uint64)
            out[sel, -1] = v * np.uint64(2 * half)
        return out
