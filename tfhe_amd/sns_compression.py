"""Compression of squashed ciphertexts on the MI355X: the packing keyswitch over the 2^128 torus and the bit-packed
stored form (include/tfhe_hip.h tfhe_hip_sns_pks_*; kernels tfhe_amd/csrc/sns_pks.hip).

fhEVM's sns-worker stores what it squashed in the ct128 bucket (coprocessor-docker-compose.yml:124-140) as a tfhe-rs
CompressedSquashedNoiseCiphertextList: up to lwe_per_glwe squashed LWEs keyswitched into one 128-bit GLWE under a
NoiseSquashingCompressionKey, then the mask and one body per ciphertext bit-packed.  Here:
  SquashedCompressionKey(params, seed, in_key) -> post-packing GLWE key (client / KMS) and the packing key (server)
  SquashedPacker(params).load_key(key).compress_squashed_into_list(lwes) -> [CompressedSquashedGlwe]
  squash_and_compress(engine, squasher, packer, cts): P-FHEVM ciphertexts -> the stored list, the squashed LWEs
      staying on the device between the 128-bit bootstrap and the packing keyswitch
  decrypt_list(key, comp, msg_modulus) -> messages (the client or KMS side)
Words of Z_2^128 travel as (lo, hi) u64 pairs in LWEs and as [lo][N], [hi][N] planes in GLWEs and keys, as in
tfhe_amd.sns.  The preset restates tfhe-rs's parameters from memory: parity unpinned.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np

from . import RngKey, _c_u64, _check, _stream_handle, _u64, lib, rng_key
from .sns import SEEDED_GUARD_WORDS, seed_words

SNS_PKS_PRESET_FHEVM = 0
_U64P = ctypes.POINTER(ctypes.c_uint64)


class SnsPksParams(ctypes.Structure):
    _fields_ = [("in_dim", ctypes.c_uint32), ("out_k", ctypes.c_uint32), ("out_N", ctypes.c_uint32),
                ("base_log", ctypes.c_uint32), ("level", ctypes.c_uint32), ("lwe_per_glwe", ctypes.c_uint32),
                ("storage_log", ctypes.c_uint32), ("noise_log2", ctypes.c_int32)]

    @classmethod
    def preset(cls, which: int = SNS_PKS_PRESET_FHEVM) -> "SnsPksParams":
        p = cls()
        _check(_lib().tfhe_hip_sns_pks_params_preset(which, ctypes.byref(p)))
        return p

    @property
    def glwe_shape(self) -> tuple:
        """(out_k + 1) polynomials of two planes [lo][N], [hi][N]"""
        return (self.out_k + 1, 2, self.out_N)

    @property
    def glwe_len(self) -> int:
        return (self.out_k + 1) * 2 * self.out_N


_BOUND = None


def _lib():
    global _BOUND
    L = lib()
    if _BOUND is None:
        P = ctypes.POINTER(SnsPksParams)
        L.tfhe_hip_sns_pks_params_preset.argtypes = [ctypes.c_int, P]
        L.tfhe_hip_sns_pksk_len.argtypes = [P]
        L.tfhe_hip_sns_pksk_len.restype = ctypes.c_size_t
        L.tfhe_hip_sns_pks_keygen.argtypes = [P, ctypes.c_uint64, _U64P, _U64P, _U64P]
        L.tfhe_hip_sns_pks_keygen_k.argtypes = [P, ctypes.POINTER(RngKey), _U64P, _U64P, _U64P]
        L.tfhe_hip_sns_pks_create.argtypes = [P, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.tfhe_hip_sns_pks_destroy.argtypes = [ctypes.c_void_p]
        L.tfhe_hip_sns_pks_destroy.restype = None
        L.tfhe_hip_sns_pks_load_key.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t]
        L.tfhe_hip_sns_pks_pack.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, _U64P]
        L.tfhe_hip_sns_pks_pack_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                  ctypes.c_void_p]
        L.tfhe_hip_sns_pks_pack_host.argtypes = [P, _U64P, _U64P, ctypes.c_size_t, _U64P]
        L.tfhe_hip_sns_pks_packed_words.argtypes = [P, ctypes.c_uint32]
        L.tfhe_hip_sns_pks_packed_words.restype = ctypes.c_size_t
        L.tfhe_hip_sns_pks_compress.argtypes = [P, _U64P, ctypes.c_uint32, _U64P]
        L.tfhe_hip_sns_pks_extract.argtypes = [P, _U64P, ctypes.c_uint32, _U64P]
        L.tfhe_hip_glwe_phase128.argtypes = [ctypes.c_uint32, ctypes.c_uint32, _U64P, _U64P, _U64P]
        L.tfhe_hip_sns_pks_seeded_bodies_len.argtypes = [P]
        L.tfhe_hip_sns_pks_seeded_bodies_len.restype = ctypes.c_size_t
        L.tfhe_hip_sns_pks_seeded_keygen.argtypes = [P, ctypes.c_uint64, _U64P, _U64P, _U64P, _U64P]
        L.tfhe_hip_sns_pks_seeded_keygen_k.argtypes = [P, ctypes.POINTER(RngKey), _U64P, _U64P, _U64P, _U64P]
        L.tfhe_hip_sns_pks_decompress_key.argtypes = [P, _U64P, _U64P, _U64P]
        L.tfhe_hip_sns_pks_load_key_seeded.argtypes = [ctypes.c_void_p, _U64P, _U64P, ctypes.c_size_t]
        L.tfhe_hip_sns_pks_seeded_load_stats.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_double)] * 3
        L.tfhe_hip_sns_pks_seeded_expand_key.argtypes = [ctypes.c_void_p, _U64P, _U64P, _U64P]
        _BOUND = True
    return L


def _groups(params: SnsPksParams, count: int) -> int:
    return -(-count // params.lwe_per_glwe)


def _lwes(params: SnsPksParams, lwes) -> np.ndarray:
    return _c_u64(lwes).reshape(-1, params.in_dim + 1, 2)


class SquashedCompressionKey:
    """Packing keyswitching key from the squashing GLWE key (read as an LWE key of dimension in_dim) to a fresh
    binary 128-bit GLWE key (`post_packing_key`, held by whoever decrypts)."""

    def __init__(self, params: SnsPksParams, seed: Optional[int], in_key: np.ndarray, with_key: bool = True):
        L = _lib()
        self.params, self.seed = params, seed
        self.in_key = _c_u64(in_key)
        if self.in_key.size != params.in_dim:
            raise ValueError("SquashedCompressionKey: in_key must hold in_dim bits")
        self.post_packing_key = np.zeros(params.out_k * params.out_N, dtype=np.uint64)
        self.pksk = np.zeros(L.tfhe_hip_sns_pksk_len(ctypes.byref(params)), dtype=np.uint64) if with_key else None
        rk = rng_key(seed)  # None: 192 bits of OS entropy (production); an int: the public test stream
        self._rk = rk       # compress() draws the same post-packing key from it
        _check(L.tfhe_hip_sns_pks_keygen_k(ctypes.byref(params), ctypes.byref(rk), _u64(self.in_key),
                                           _u64(self.post_packing_key), _u64(self.pksk) if with_key else None))

    def compress(self, mask_seed: Optional[int] = None) -> "CompressedSquashedCompressionKey":
        """The seeded form of this packing key (the CompressedNoiseSquashingCompressionKey::new role): a fresh key
        to the same post-packing key, bodies only, its masks the 128-bit AES-CTR stream of `mask_seed` (OS entropy
        when None; a given seed makes every mask public, test data only).  Parity with tfhe-rs unpinned."""
        import os
        p = self.params
        ms = int.from_bytes(os.urandom(16), "little") if mask_seed is None else int(mask_seed)
        bodies = np.zeros((p.in_dim, p.level, p.out_N, 2), dtype=np.uint64)
        out_key = np.zeros_like(self.post_packing_key)
        _check(_lib().tfhe_hip_sns_pks_seeded_keygen_k(ctypes.byref(p), ctypes.byref(self._rk), _u64(seed_words(ms)),
                                                       _u64(self.in_key), _u64(out_key), _u64(bodies)))
        assert np.array_equal(out_key, self.post_packing_key)
        return CompressedSquashedCompressionKey(p, ms, bodies)


class CompressedSquashedCompressionKey:
    """The seeded ct128 packing key a server ingests without any secret: bodies [in_dim][level][out_N] of u128 words
    as (lo, hi) pairs, storage row s = decomposition level `level - s`, and the 128-bit seed of their masks
    (include/tfhe_hip.h; parity unpinned).  `SquashedPacker.load_compressed_key` expands it on the device;
    `decompress()` is the host route and its reference."""

    def __init__(self, params: SnsPksParams, seed: int, bodies: np.ndarray):
        b = _c_u64(bodies)
        if b.size != _lib().tfhe_hip_sns_pks_seeded_bodies_len(ctypes.byref(params)) or b.size == 0:
            raise ValueError("CompressedSquashedCompressionKey: the bodies do not match the parameters")
        self.params, self.seed = params, int(seed)
        self.bodies = b.reshape(params.in_dim, params.level, params.out_N, 2)
        seed_words(self.seed)

    def decompress(self) -> "DecompressedSquashedCompressionKey":
        p = self.params
        pksk = np.zeros(_lib().tfhe_hip_sns_pksk_len(ctypes.byref(p)), dtype=np.uint64)
        _check(_lib().tfhe_hip_sns_pks_decompress_key(ctypes.byref(p), _u64(seed_words(self.seed)), _u64(self.bodies),
                                                      _u64(pksk)))
        return DecompressedSquashedCompressionKey(p, pksk)


class DecompressedSquashedCompressionKey:
    """Standard-domain words of a ct128 packing key in the layout `SquashedPacker.load_key` reads."""

    def __init__(self, params: SnsPksParams, pksk: np.ndarray):
        self.params, self.pksk = params, pksk


def pack_host(params: SnsPksParams, pksk: np.ndarray, lwes: np.ndarray) -> np.ndarray:
    """The packing keyswitch on the CPU (no device): count LWEs -> (groups, out_k + 1, 2, N)."""
    x, k = _lwes(params, lwes), _c_u64(pksk)
    if k.size != _lib().tfhe_hip_sns_pksk_len(ctypes.byref(params)):
        raise ValueError("pack_host: the key does not match the parameters")
    out = np.zeros((_groups(params, x.shape[0]),) + params.glwe_shape, dtype=np.uint64)
    _check(_lib().tfhe_hip_sns_pks_pack_host(ctypes.byref(params), _u64(k), _u64(x), x.shape[0], _u64(out)))
    return out


def packed_words(params: SnsPksParams, bodies: int) -> int:
    return _lib().tfhe_hip_sns_pks_packed_words(ctypes.byref(params), bodies)


class CompressedSquashedGlwe:
    """A bit-packed 128-bit GLWE holding `bodies` squashed ciphertexts."""

    def __init__(self, params: SnsPksParams, packed: np.ndarray, bodies: int):
        self.params, self.packed, self.bodies = params, packed, bodies

    def extract(self) -> np.ndarray:
        out = np.zeros(self.params.glwe_shape, dtype=np.uint64)
        _check(_lib().tfhe_hip_sns_pks_extract(ctypes.byref(self.params), _u64(self.packed), self.bodies, _u64(out)))
        return out

    @property
    def nbytes(self) -> int:
        return self.packed.nbytes


def compress_glwe(params: SnsPksParams, glwe: np.ndarray, bodies: int) -> CompressedSquashedGlwe:
    g = _c_u64(glwe)
    if g.size != params.glwe_len:
        raise ValueError("compress_glwe: one GLWE of (out_k + 1) x 2 x N words")
    out = np.zeros(packed_words(params, bodies), dtype=np.uint64)
    _check(_lib().tfhe_hip_sns_pks_compress(ctypes.byref(params), _u64(g), bodies, _u64(out)))
    return CompressedSquashedGlwe(params, out, bodies)


def _compress_groups(params: SnsPksParams, glwes: np.ndarray, count: int) -> List[CompressedSquashedGlwe]:
    return [compress_glwe(params, glwes[g], min(params.lwe_per_glwe, count - g * params.lwe_per_glwe))
            for g in range(glwes.shape[0])]


def glwe_phase128(k: int, N: int, key: np.ndarray, glwe: np.ndarray) -> list:
    """body - sum_c mask_c * S_c of a 128-bit GLWE, as N Python ints."""
    kk, g = _c_u64(key), _c_u64(glwe)
    if kk.size != k * N or g.size != (k + 1) * 2 * N:
        raise ValueError("glwe_phase128: key of k*N bits, GLWE of (k + 1) x 2 x N words")
    out = np.zeros((2, N), dtype=np.uint64)
    _check(_lib().tfhe_hip_glwe_phase128(k, N, _u64(kk), _u64(g), _u64(out)))
    return [int(lo) | (int(hi) << 64) for lo, hi in zip(out[0], out[1])]


def decrypt_list(key: SquashedCompressionKey, comp: List[CompressedSquashedGlwe], msg_modulus: int = 16) -> np.ndarray:
    """The client or KMS side: every ciphertext of the list, round(phase / (2^127 / msg_modulus)) mod msg_modulus."""
    p, delta = key.params, (1 << 127) // msg_modulus
    out = []
    for c in comp:
        ph = glwe_phase128(p.out_k, p.out_N, key.post_packing_key, c.extract())[:c.bodies]
        out += [((x + delta // 2) // delta) % msg_modulus for x in ph]
    return np.array(out, dtype=np.uint64)


class SquashedPacker:
    """Device context for the 128-bit packing keyswitch (one GPU)."""

    def __init__(self, params: SnsPksParams, device: int = 0):
        self.params, self.device = params, device
        h = ctypes.c_void_p()
        _check(_lib().tfhe_hip_sns_pks_create(ctypes.byref(params), device, ctypes.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            _lib().tfhe_hip_sns_pks_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_key(self, key: SquashedCompressionKey) -> "SquashedPacker":
        k = _c_u64(key.pksk)
        _check(_lib().tfhe_hip_sns_pks_load_key(self._h, _u64(k), k.size))
        return self

    def load_compressed_key(self, key: CompressedSquashedCompressionKey) -> "SquashedPacker":
        """Bodies and seed go up and the masks are generated straight into the resident key on the device
        (tfhe_amd/csrc/seeded_keys128.hip): the same resident key as `load_key(key.decompress())`, bit for bit."""
        b = _c_u64(key.bodies).ravel()
        _check(_lib().tfhe_hip_sns_pks_load_key_seeded(self._h, _u64(seed_words(key.seed)), _u64(b), b.size))
        return self

    def seeded_load_stats(self) -> dict:
        """Device milliseconds of the last load_compressed_key: upload, expansion, correction."""
        v = [ctypes.c_double() for _ in range(3)]
        _check(_lib().tfhe_hip_sns_pks_seeded_load_stats(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("upload_ms", "expand_ms", "corr_ms"), (x.value for x in v)))

    def seeded_expand(self, key: CompressedSquashedCompressionKey):
        """Test aid: the loader's expansion alone -> (key words in the loader's layout, guard words behind them)."""
        b = _c_u64(key.bodies).ravel()
        n = _lib().tfhe_hip_sns_pksk_len(ctypes.byref(self.params))
        out = np.zeros(n + SEEDED_GUARD_WORDS, dtype=np.uint64)
        _check(_lib().tfhe_hip_sns_pks_seeded_expand_key(self._h, _u64(seed_words(key.seed)), _u64(b), _u64(out)))
        return out[:n], out[n:]

    def pack(self, lwes: np.ndarray) -> np.ndarray:
        """count squashed LWEs (count, in_dim + 1, 2) -> (ceil(count / lwe_per_glwe), out_k + 1, 2, N) GLWEs."""
        p = self.params
        x = _lwes(p, lwes)
        out = np.zeros((_groups(p, x.shape[0]),) + p.glwe_shape, dtype=np.uint64)
        _check(_lib().tfhe_hip_sns_pks_pack(self._h, _u64(x), x.shape[0], _u64(out)))
        return out

    def pack_async(self, d_lwes, count: int, d_glwes, stream=None) -> None:
        """torch device tensors (int64/uint64), enqueued on `stream` (torch.cuda.Stream, raw handle, or None =
        torch's current stream).  d_glwes holds at least ceil(count / lwe_per_glwe) GLWEs."""
        p = self.params
        if d_lwes.numel() < count * (p.in_dim + 1) * 2 or d_glwes.numel() < _groups(p, count) * p.glwe_len:
            raise ValueError("pack_async: a buffer is smaller than count ciphertexts need")
        _check(_lib().tfhe_hip_sns_pks_pack_async(self._h, ctypes.c_void_p(d_lwes.data_ptr()), count,
                                                  ctypes.c_void_p(d_glwes.data_ptr()),
                                                  ctypes.c_void_p(_stream_handle(stream, self.device))))

    def compress_squashed_into_list(self, lwes: np.ndarray) -> List[CompressedSquashedGlwe]:
        """Pack chunks of lwe_per_glwe on the device, then modulus-switch + bit-pack each GLWE on the host."""
        x = _lwes(self.params, lwes)
        return _compress_groups(self.params, self.pack(x), x.shape[0])


def squash_and_compress(engine, squasher, packer: SquashedPacker, cts: np.ndarray,
                        msg_modulus: Optional[int] = None) -> List[CompressedSquashedGlwe]:
    """P-FHEVM big-key ciphertexts -> the stored list: keyswitch + modulus-switch noise reduction (engine), then
    the 128-bit bootstrap (squasher) and the packing keyswitch (packer) enqueued back to back on one stream.  The
    squashed LWEs (64 KB each) stay on the device; only the packed GLWEs are downloaded."""
    import torch
    mm = msg_modulus or 16
    sp, pp = squasher.params, packer.params
    if sp.out_dim != pp.in_dim or squasher.device != packer.device:
        raise ValueError("squash_and_compress: the packer takes the squasher's LWEs (k*N = in_dim) on its device")
    small, _ = engine.ms_reduce(engine.keyswitch(cts))
    count = small.shape[0]
    if count == 0:
        return []
    dev = torch.device("cuda", packer.device)
    stream = torch.cuda.current_stream(dev)
    d_small = torch.from_numpy(np.ascontiguousarray(small).view(np.int64)).to(dev)
    d_sq = torch.empty((count, sp.out_dim + 1, 2), dtype=torch.int64, device=dev)
    d_glwes = torch.empty((_groups(pp, count),) + pp.glwe_shape, dtype=torch.int64, device=dev)
    squasher.squash_async(d_small, count, d_sq, mm, stream)
    packer.pack_async(d_sq, count, d_glwes, stream)
    glwes = d_glwes.cpu().numpy().view(np.uint64)
    return _compress_groups(pp, glwes, count)
