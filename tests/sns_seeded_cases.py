"""Keys and inputs shared by tests/test_sns_seeded.py (CPU) and tests/test_gpu_sns_seeded.py (device): seeded squashing
keys at a small LWE dimension, seeded ct128 packing keys at small shapes, their host decompressions (computed once and
left read-only), and noiseless small-key ciphertexts."""
import functools

import numpy as np

from tfhe_amd import sns as S
from tfhe_amd import sns_compression as SC

RNG_SEED = 0x5EED128                                   # ChaCha streams: GLWE keys and noise (public: test data)
MASK_SEED = 0x0123456789ABCDEF_FEDCBA9876543210        # the AES-CTR compression seed
MASK_SEED_TOP = MASK_SEED ^ (0xFF << 120)              # differs from MASK_SEED in the top byte only
PKS_NOISE_LOG2 = -62


def squash_params(n: int) -> S.SnsParams:
    sp = S.SnsParams.preset(0)
    sp.n = n
    return sp


def lwe_key(n: int) -> np.ndarray:
    """binary, with both values from n = 2 on, element 0 set"""
    key = np.random.default_rng(1000 + n).integers(0, 2, n).astype(np.uint64)
    key[0] = 1
    if n > 1:
        key[1] = 0
    return key


@functools.lru_cache(maxsize=None)
def squash_keys(n: int, mask_seed: int = MASK_SEED):
    """(params, client SquashedKey without a BSK, CompressedSquashedKey, its host decompression)"""
    sp = squash_params(n)
    key = S.SquashedKey(sp, RNG_SEED, lwe_key(n), with_bsk=False)
    ckey = key.compress(mask_seed)
    dk = ckey.decompress()
    ckey.bodies.setflags(write=False)
    dk.bsk.setflags(write=False)
    return sp, key, ckey, dk


def packing_params(in_dim, out_k, out_N, level, base_log=None, lwe_per_glwe=None, storage_log=128) -> SC.SnsPksParams:
    base_log = base_log if base_log is not None else (61 if level == 1 else 120 // level)
    return SC.SnsPksParams(in_dim, out_k, out_N, base_log, level, lwe_per_glwe or min(out_N, 32), storage_log,
                           PKS_NOISE_LOG2)


@functools.lru_cache(maxsize=None)
def packing_keys(in_dim, out_k, out_N, level, base_log=None, lwe_per_glwe=None, in_key_seed=7):
    """(params, client SquashedCompressionKey without the key words, CompressedSquashedCompressionKey, its host
    decompression) for a random binary input key"""
    pp = packing_params(in_dim, out_k, out_N, level, base_log, lwe_per_glwe)
    in_key = np.random.default_rng([in_key_seed, in_dim]).integers(0, 2, in_dim).astype(np.uint64)
    key = SC.SquashedCompressionKey(pp, RNG_SEED, in_key, with_key=False)
    ckey = key.compress(MASK_SEED)
    dk = ckey.decompress()
    ckey.bodies.setflags(write=False)
    dk.pksk.setflags(write=False)
    return pp, key, ckey, dk


def small_inputs(n: int, msgs, seed: int = 3, key=None) -> np.ndarray:
    """Noiseless small-key encryptions of msgs (mod 16, one padding bit) under `key` (lwe_key(n) by default): mask
    uniform, b = <a, s> + m 2^59."""
    rng = np.random.default_rng([seed, n, len(msgs)])
    cts = rng.integers(0, 2 ** 64, size=(len(msgs), n + 1), dtype=np.uint64)
    s = lwe_key(n) if key is None else np.asarray(key, dtype=np.uint64)
    with np.errstate(over="ignore"):
        cts[:, n] = (cts[:, :n] * s).sum(axis=1, dtype=np.uint64) + (np.asarray(msgs, dtype=np.uint64) << np.uint64(59))
    return cts
