"""Switch-and-squash: noise squashing of P-FHEVM ciphertexts into 128-bit LWEs on the MI355X
(include/tfhe_hip.h tfhe_hip_sns_*; kernels tfhe_amd/csrc/sns.hip).

fhEVM's sns-worker (coprocessor-docker-compose.yml:124-140) squashes each 64-bit ciphertext before
threshold decryption.  Here: `squash_noise(engine, squasher, cts)` = keyswitch to the small key and
modulus-switch noise reduction on the P-FHEVM engine, then the 128-bit bootstrap with the identity
LUT on the squasher; `SquashedKey.decrypt` recovers the message from the (k*N+1) x 128-bit LWE.
The GLWE ring is the native 2^128 torus, as in tfhe-rs: a coefficient is one u128 word, held as
(lo, hi) u64 pairs in the LWEs and as [lo][N], [hi][N] planes in keys and accumulators.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import RngKey, _c_u64, _check, _stream_handle, _u64, lib, rng_key

SNS_PRESET_FHEVM = 0
SEEDED_GUARD_WORDS = 64  # TFHE_HIP_SEEDED_GUARD_WORDS
_U64P = ctypes.POINTER(ctypes.c_uint64)


class SnsParams(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("k", ctypes.c_uint32), ("N", ctypes.c_uint32), ("base_log", ctypes.c_uint32),
                ("level", ctypes.c_uint32), ("noise_log2", ctypes.c_int32)]

    @classmethod
    def preset(cls, which: int = SNS_PRESET_FHEVM) -> "SnsParams":
        p = cls()
        _check(_lib().tfhe_hip_sns_params_preset(which, ctypes.byref(p)))
        return p

    @property
    def out_dim(self) -> int:
        return self.k * self.N


_BOUND = None


def _lib():
    global _BOUND
    L = lib()
    if _BOUND is None:
        P = ctypes.POINTER(SnsParams)
        L.tfhe_hip_sns_params_preset.argtypes = [ctypes.c_int, P]
        L.tfhe_hip_sns_bsk_len.argtypes = [P]
        L.tfhe_hip_sns_bsk_len.restype = ctypes.c_size_t
        L.tfhe_hip_sns_keygen.argtypes = [P, ctypes.c_uint64, _U64P, _U64P, _U64P]
        L.tfhe_hip_sns_keygen_k.argtypes = [P, ctypes.POINTER(RngKey), _U64P, _U64P, _U64P]
        L.tfhe_hip_sns_create.argtypes = [P, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.tfhe_hip_sns_destroy.argtypes = [ctypes.c_void_p]
        L.tfhe_hip_sns_load_key.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t]
        L.tfhe_hip_sns_squash.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, ctypes.c_uint32, _U64P]
        L.tfhe_hip_sns_squash_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                                                ctypes.c_void_p, ctypes.c_void_p]
        L.tfhe_hip_sns_blind_rotate.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, ctypes.c_uint32, _U64P]
        L.tfhe_hip_sns_phase.argtypes = [P, _U64P, _U64P, ctypes.c_size_t, _U64P]
        L.tfhe_hip_sns_seeded_bodies_len.argtypes = [P]
        L.tfhe_hip_sns_seeded_bodies_len.restype = ctypes.c_size_t
        L.tfhe_hip_sns_seeded_keygen.argtypes = [P, ctypes.c_uint64, _U64P, _U64P, _U64P, _U64P]
        L.tfhe_hip_sns_seeded_keygen_k.argtypes = [P, ctypes.POINTER(RngKey), _U64P, _U64P, _U64P, _U64P]
        L.tfhe_hip_sns_decompress_bsk.argtypes = [P, _U64P, _U64P, _U64P]
        L.tfhe_hip_csprng_words128.argtypes = [_U64P, ctypes.c_uint64, ctypes.c_size_t, _U64P]
        L.tfhe_hip_sns_load_key_seeded.argtypes = [ctypes.c_void_p, _U64P, _U64P, ctypes.c_size_t]
        L.tfhe_hip_sns_seeded_load_stats.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_double)] * 3
        L.tfhe_hip_sns_seeded_expand_bsk.argtypes = [ctypes.c_void_p, _U64P, _U64P, _U64P]
        _BOUND = True
    return L


class SquashedKey:
    """128-bit GLWE key (client side) and the squashing BSK (server side) for a small LWE key."""

    def __init__(self, params: SnsParams, seed: Optional[int], lwe_key: np.ndarray, with_bsk: bool = True):
        L = _lib()
        self.params, self.seed = params, seed
        self.lwe_key = _c_u64(lwe_key)
        self.glwe_key = np.zeros(params.k * params.N, dtype=np.uint64)
        self.bsk = np.zeros(L.tfhe_hip_sns_bsk_len(ctypes.byref(params)), dtype=np.uint64) if with_bsk else None
        rk = rng_key(seed)  # None: 192 bits of OS entropy (production); an int: the public test stream
        self._rk = rk       # compress() draws the same GLWE key from it
        _check(L.tfhe_hip_sns_keygen_k(ctypes.byref(params), ctypes.byref(rk), _u64(self.lwe_key), _u64(self.glwe_key),
                                     _u64(self.bsk) if with_bsk else None))

    def compress(self, mask_seed: Optional[int] = None) -> "CompressedSquashedKey":
        """The seeded form of this key's squashing BSK (the CompressedNoiseSquashingKey::new role): a fresh key under
        the same GLWE key, bodies only, its masks the 128-bit AES-CTR stream of `mask_seed` (OS entropy when None; a
        given seed makes every mask public, test data only).  Parity with tfhe-rs unpinned at the byte level."""
        import os
        p = self.params
        ms = int.from_bytes(os.urandom(16), "little") if mask_seed is None else int(mask_seed)
        bodies = np.zeros((p.n, p.level, p.k + 1, p.N, 2), dtype=np.uint64)
        glwe = np.zeros_like(self.glwe_key)
        _check(_lib().tfhe_hip_sns_seeded_keygen_k(ctypes.byref(p), ctypes.byref(self._rk), _u64(seed_words(ms)),
                                                   _u64(self.lwe_key), _u64(glwe), _u64(bodies)))
        assert np.array_equal(glwe, self.glwe_key)
        return CompressedSquashedKey(p, ms, bodies)

    def phase(self, cts: np.ndarray) -> list:
        p = self.params
        c = _c_u64(cts).reshape(-1, p.out_dim + 1, 2)
        out = np.zeros((c.shape[0], 2), dtype=np.uint64)
        _check(_lib().tfhe_hip_sns_phase(ctypes.byref(p), _u64(self.glwe_key), _u64(c), c.shape[0], _u64(out)))
        return [int(o[0]) | (int(o[1]) << 64) for o in out]

    def decrypt(self, cts: np.ndarray, msg_modulus: int = 16) -> np.ndarray:
        """round(phase / (2^127 / msg_modulus)) mod msg_modulus (one padding bit)."""
        delta = (1 << 127) // msg_modulus
        return np.array([((ph + delta // 2) // delta) % msg_modulus for ph in self.phase(cts)], dtype=np.uint64)


def seed_words(seed: int) -> np.ndarray:
    """A 128-bit compression seed as the (lo, hi) u64 pair of the C interface."""
    if not 0 <= seed < 1 << 128:
        raise ValueError(f"compression seed out of range: {seed}")
    return np.array([seed & ((1 << 64) - 1), seed >> 64], dtype=np.uint64)


def stream_words128(seed: int, first: int, count: int) -> np.ndarray:
    """u128 mask words first .. first + count - 1 of a seed's stream as (count, 2) u64 pairs (lo, hi): word w is
    bytes 16 w + 1 .. 16 w + 16 of the AES-CTR table, little endian (include/tfhe_hip.h)."""
    out = np.zeros((count, 2), dtype=np.uint64)
    _check(_lib().tfhe_hip_csprng_words128(_u64(seed_words(seed)), first, count, _u64(out)))
    return out


class CompressedSquashedKey:
    """The seeded squashing key a server ingests without any secret: bodies [n][L][k+1][N] of u128 words as (lo, hi)
    pairs and the 128-bit seed of their masks (include/tfhe_hip.h, the seeded squashing key; parity unpinned).
    `Squasher.load_compressed_key` expands it on the device; `decompress()` is the host route and its reference."""

    def __init__(self, params: SnsParams, seed: int, bodies: np.ndarray):
        b = _c_u64(bodies)
        if b.size != _lib().tfhe_hip_sns_seeded_bodies_len(ctypes.byref(params)) or b.size == 0:
            raise ValueError("CompressedSquashedKey: the bodies do not match the parameters")
        self.params, self.seed = params, int(seed)
        self.bodies = b.reshape(params.n, params.level, params.k + 1, params.N, 2)
        seed_words(self.seed)

    def decompress(self) -> "DecompressedSquashedKey":
        p = self.params
        bsk = np.zeros(_lib().tfhe_hip_sns_bsk_len(ctypes.byref(p)), dtype=np.uint64)
        _check(_lib().tfhe_hip_sns_decompress_bsk(ctypes.byref(p), _u64(seed_words(self.seed)), _u64(self.bodies),
                                                  _u64(bsk)))
        return DecompressedSquashedKey(p, bsk)


class DecompressedSquashedKey:
    """Standard-domain words of a squashing BSK in the layout `Squasher.load_key` reads ([i][c*L+l][j][lo, hi][N])."""

    def __init__(self, params: SnsParams, bsk: np.ndarray):
        self.params, self.bsk = params, bsk


class Squasher:
    """Device context for noise squashing (one GPU)."""

    def __init__(self, params: SnsParams, device: int = 0):
        self.params, self.device = params, device
        h = ctypes.c_void_p()
        _check(_lib().tfhe_hip_sns_create(ctypes.byref(params), device, ctypes.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            _lib().tfhe_hip_sns_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_key(self, key: SquashedKey) -> "Squasher":
        b = _c_u64(key.bsk)
        _check(_lib().tfhe_hip_sns_load_key(self._h, _u64(b), b.size))
        return self

    def load_compressed_key(self, key: CompressedSquashedKey) -> "Squasher":
        """Bodies and seed go up, the masks are generated into the key layout on the device
        (tfhe_amd/csrc/seeded_keys128.hip) and the usual conversion follows: the same resident key as
        `load_key(key.decompress())`, bit for bit."""
        b = _c_u64(key.bodies).ravel()
        _check(_lib().tfhe_hip_sns_load_key_seeded(self._h, _u64(seed_words(key.seed)), _u64(b), b.size))
        return self

    def seeded_load_stats(self) -> dict:
        """Device milliseconds of the last load_compressed_key: upload, expansion, conversion."""
        v = [ctypes.c_double() for _ in range(3)]
        _check(_lib().tfhe_hip_sns_seeded_load_stats(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("upload_ms", "expand_ms", "convert_ms"), (x.value for x in v)))

    def seeded_expand(self, key: CompressedSquashedKey):
        """Test aid: the loader's expansion alone -> (key words in the loader's layout, guard words behind them)."""
        b = _c_u64(key.bodies).ravel()
        n = _lib().tfhe_hip_sns_bsk_len(ctypes.byref(self.params))
        out = np.zeros(n + SEEDED_GUARD_WORDS, dtype=np.uint64)
        _check(_lib().tfhe_hip_sns_seeded_expand_bsk(self._h, _u64(seed_words(key.seed)), _u64(b), _u64(out)))
        return out[:n], out[n:]

    def squash(self, small: np.ndarray, msg_modulus: int = 16) -> np.ndarray:
        """small-key ciphertexts (B x (n+1)) -> B x (k N + 1) x 2 u64 (128-bit LWEs, (lo, hi))."""
        p = self.params
        x = _c_u64(small).reshape(-1, p.n + 1)
        out = np.zeros((x.shape[0], p.out_dim + 1, 2), dtype=np.uint64)
        _check(_lib().tfhe_hip_sns_squash(self._h, _u64(x), x.shape[0], msg_modulus, _u64(out)))
        return out

    def squash_async(self, d_small, B: int, d_out, msg_modulus: int = 16, stream=None) -> None:
        _check(_lib().tfhe_hip_sns_squash_async(self._h, ctypes.c_void_p(d_small.data_ptr()), B, msg_modulus,
                                                ctypes.c_void_p(d_out.data_ptr()),
                                                ctypes.c_void_p(_stream_handle(stream, self.device))))

    def blind_rotate(self, small: np.ndarray, msg_modulus: int = 16) -> np.ndarray:
        p = self.params
        x = _c_u64(small).reshape(-1, p.n + 1)
        out = np.zeros((x.shape[0], p.k + 1, 2, p.N), dtype=np.uint64)
        _check(_lib().tfhe_hip_sns_blind_rotate(self._h, _u64(x), x.shape[0], msg_modulus, _u64(out)))
        return out


def squash_noise(engine, squasher: Squasher, cts: np.ndarray, msg_modulus: Optional[int] = None) -> np.ndarray:
    """P-FHEVM big-key ciphertexts -> squashed 128-bit LWEs: keyswitch + modulus-switch noise
    reduction (engine, KS -> PBS parameter set) then the 128-bit bootstrap (squasher)."""
    mm = msg_modulus or 16
    small = engine.keyswitch(cts)
    small, _ = engine.ms_reduce(small)
    return squasher.squash(small, mm)
