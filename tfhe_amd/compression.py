"""LWE -> GLWE packing keyswitch and modulus-switched ciphertext compression on the MI355X
(include/tfhe_hip.h tfhe_hip_pks_*; kernels tfhe_amd/csrc/pks.hip).

Mirrors the reference's compression surface (ml/extensions/rust/src/compression.rs):
  CompressionKey.new(input_lwe_secret_key, params) -> (post-packing GLWE key, key)   :159-187
  compress_ciphertexts_into_list(lwes) -> [CompressedGlwe]                           :246-291
  CompressedGlwe.extract() -> GLWE                                                   :134-156
with the packing keyswitch on the GPU (one integer GEMM + negacyclic shift-sum per chunk of GLWEs)
and the modulus switch / bit packing on the host.  Parameters: the reference's PARAMS_8B_2048_NEW
(ml/extensions/rust/src/fhext_classes.rs:98-112).

The return half (tfhe-rs CompressedCiphertextList::get / DecompressionKey::unpack) runs on the GPU:
  DecompressionKey(compute_params, pks_params, post_packing_key, glwe_key, seed) -> a BSK, no KSK
  Decompressor(dk).decompress([CompressedGlwe]) -> LWEs under the compute GLWE key
(unpack + sample extraction: tfhe_amd/csrc/decompress.hip; then a PBS without keyswitch on a BSK-only engine).

The front half, which produces the LWEs that ``Packer`` consumes (the reference's encrypted matrix x clear matrix
product), is ``tfhe_amd.matmul``.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np

from . import Engine, Params, RngKey, _c_u64, _check, _stream_handle, _u64, lib, lut_from_table, rng_key

PKS_PRESET_ML2048 = 0
_U64P = ctypes.POINTER(ctypes.c_uint64)


class PksParams(ctypes.Structure):
    _fields_ = [("in_dim", ctypes.c_uint32), ("out_k", ctypes.c_uint32), ("out_N", ctypes.c_uint32),
                ("base_log", ctypes.c_uint32), ("level", ctypes.c_uint32), ("lwe_per_glwe", ctypes.c_uint32),
                ("storage_log", ctypes.c_uint32), ("noise_log2", ctypes.c_int32)]

    @classmethod
    def preset(cls, which: int = PKS_PRESET_ML2048) -> "PksParams":
        p = cls()
        _check(_lib().tfhe_hip_pks_params_preset(which, ctypes.byref(p)))
        return p

    @property
    def glwe_len(self) -> int:
        return (self.out_k + 1) * self.out_N


_BOUND = None


def _lib():
    global _BOUND
    L = lib()
    if _BOUND is None:
        P = ctypes.POINTER(PksParams)
        L.tfhe_hip_pks_params_preset.argtypes = [ctypes.c_int, P]
        L.tfhe_hip_pksk_len.argtypes = [P]
        L.tfhe_hip_pksk_len.restype = ctypes.c_size_t
        L.tfhe_hip_pks_keygen.argtypes = [P, ctypes.c_uint64, _U64P, _U64P, _U64P]
        L.tfhe_hip_pks_keygen_k.argtypes = [P, ctypes.POINTER(RngKey), _U64P, _U64P, _U64P]
        L.tfhe_hip_pks_create.argtypes = [P, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.tfhe_hip_pks_destroy.argtypes = [ctypes.c_void_p]
        L.tfhe_hip_pks_load_key.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t]
        L.tfhe_hip_pks_pack.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, _U64P]
        L.tfhe_hip_pks_pack_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                              ctypes.c_void_p]
        L.tfhe_hip_pks_packed_words.argtypes = [P, ctypes.c_uint32]
        L.tfhe_hip_pks_packed_words.restype = ctypes.c_size_t
        L.tfhe_hip_pks_compress.argtypes = [P, _U64P, ctypes.c_uint32, _U64P]
        L.tfhe_hip_pks_extract.argtypes = [P, _U64P, ctypes.c_uint32, _U64P]
        L.tfhe_hip_glwe_phase.argtypes = [ctypes.c_uint32, ctypes.c_uint32, _U64P, _U64P, _U64P]
        L.tfhe_hip_pks_unpack_extract.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, ctypes.c_size_t, _U64P]
        L.tfhe_hip_pks_unpack_extract_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                        ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        L.tfhe_hip_decompress.argtypes = [ctypes.c_void_p, P, _U64P, ctypes.c_size_t, ctypes.c_size_t, _U64P,
                                          ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32), _U64P]
        L.tfhe_hip_decompress_async.argtypes = [ctypes.c_void_p, P, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                                ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p]
        _BOUND = True
    return L


class CompressionKey:
    """Packing keyswitching key from an input LWE key (e.g. a GLWE key read as an LWE key) to a fresh
    binary GLWE key (`post_packing_key`, held by the client for decryption)."""

    def __init__(self, params: PksParams, seed: Optional[int], in_key: np.ndarray, with_key: bool = True):
        L = _lib()
        self.params, self.seed = params, seed
        self.in_key = _c_u64(in_key)
        self.post_packing_key = np.zeros(params.out_k * params.out_N, dtype=np.uint64)
        self.pksk = np.zeros(L.tfhe_hip_pksk_len(ctypes.byref(params)), dtype=np.uint64) if with_key else None
        rk = rng_key(seed)  # None: 192 bits of OS entropy (production); an int: the public test stream
        _check(L.tfhe_hip_pks_keygen_k(ctypes.byref(params), ctypes.byref(rk), _u64(self.in_key), _u64(self.post_packing_key),
                                     _u64(self.pksk) if with_key else None))


class CompressedGlwe:
    """A modulus-switched, bit-packed GLWE holding `bodies` ciphertexts (compression.rs:134-156)."""

    def __init__(self, params: PksParams, packed: np.ndarray, bodies: int):
        self.params, self.packed, self.bodies = params, packed, bodies

    def extract(self) -> np.ndarray:
        out = np.zeros(self.params.glwe_len, dtype=np.uint64)
        _check(_lib().tfhe_hip_pks_extract(ctypes.byref(self.params), _u64(self.packed), self.bodies, _u64(out)))
        return out

    @property
    def nbytes(self) -> int:
        return self.packed.nbytes


def compress_glwe(params: PksParams, glwe: np.ndarray, bodies: int) -> CompressedGlwe:
    L = _lib()
    g = _c_u64(glwe)
    out = np.zeros(L.tfhe_hip_pks_packed_words(ctypes.byref(params), bodies), dtype=np.uint64)
    _check(L.tfhe_hip_pks_compress(ctypes.byref(params), _u64(g), bodies, _u64(out)))
    return CompressedGlwe(params, out, bodies)


def glwe_phase(k: int, N: int, key: np.ndarray, glwe: np.ndarray) -> np.ndarray:
    out = np.zeros(N, dtype=np.uint64)
    kk, g = _c_u64(key), _c_u64(glwe)
    _check(_lib().tfhe_hip_glwe_phase(k, N, _u64(kk), _u64(g), _u64(out)))
    return out


class Packer:
    """Device context for the packing keyswitch (one GPU)."""

    def __init__(self, params: PksParams, device: int = 0):
        self.params, self.device = params, device
        h = ctypes.c_void_p()
        _check(_lib().tfhe_hip_pks_create(ctypes.byref(params), device, ctypes.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            _lib().tfhe_hip_pks_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_key(self, key: CompressionKey) -> "Packer":
        k = _c_u64(key.pksk)
        _check(_lib().tfhe_hip_pks_load_key(self._h, _u64(k), k.size))
        return self

    def pack(self, lwes: np.ndarray) -> np.ndarray:
        """count LWEs -> (ceil(count / lwe_per_glwe), (k+1)N) GLWEs."""
        p = self.params
        x = _c_u64(lwes).reshape(-1, p.in_dim + 1)
        groups = -(-x.shape[0] // p.lwe_per_glwe)
        out = np.zeros((groups, p.glwe_len), dtype=np.uint64)
        _check(_lib().tfhe_hip_pks_pack(self._h, _u64(x), x.shape[0], _u64(out)))
        return out

    def pack_async(self, d_lwes, count: int, d_glwes, stream=None) -> None:
        """torch device tensors (int64/uint64), enqueued on `stream` (torch.cuda.Stream, raw handle, or None =
        torch's current stream)."""
        _check(_lib().tfhe_hip_pks_pack_async(self._h, ctypes.c_void_p(d_lwes.data_ptr()), count,
                                              ctypes.c_void_p(d_glwes.data_ptr()),
                                              ctypes.c_void_p(_stream_handle(stream, self.device))))

    def compress_ciphertexts_into_list(self, lwes: np.ndarray) -> List[CompressedGlwe]:
        """compression.rs:246-291: pack chunks of lwe_per_glwe, then modulus-switch + bit-pack each."""
        p = self.params
        x = _c_u64(lwes).reshape(-1, p.in_dim + 1)
        glwes = self.pack(x)
        out = []
        for g in range(glwes.shape[0]):
            bodies = min(p.lwe_per_glwe, x.shape[0] - g * p.lwe_per_glwe)
            out.append(compress_glwe(p, glwes[g], bodies))
        return out

    def unpack_extract(self, comp: List[CompressedGlwe]) -> np.ndarray:
        """Steps 1 and 2 of the decompression on the device (decompress.hip): the list's ciphertexts as LWEs under
        the post-packing key, (count, k*N + 1); row g * lwe_per_glwe + i is ``extract_lwe(comp[g].extract(), i)``."""
        packed, count = concat_list(self.params, comp)
        out = np.zeros((count, self.params.out_k * self.params.out_N + 1), dtype=np.uint64)
        _check(_lib().tfhe_hip_pks_unpack_extract(self._h, _u64(packed), packed.size, count, _u64(out)))
        return out

    def unpack_extract_async(self, d_packed, count: int, d_lwes, stream=None) -> None:
        """The same on torch device tensors (d_packed: the concatenated words, d_lwes: (count, k*N + 1)), enqueued
        on ``stream`` like ``pack_async``."""
        _check(_lib().tfhe_hip_pks_unpack_extract_async(self._h, ctypes.c_void_p(d_packed.data_ptr()),
                                                        d_packed.numel(), count, ctypes.c_void_p(d_lwes.data_ptr()),
                                                        ctypes.c_void_p(_stream_handle(stream, self.device))))


def concat_list(params: PksParams, comp: List[CompressedGlwe]):
    """The list layout of tfhe_hip_pks_unpack_extract / tfhe_hip_decompress: the groups' packed words back to back,
    every group but the last full -> (words, count)."""
    for c in comp[:-1]:
        if c.bodies != params.lwe_per_glwe:
            raise ValueError("every compressed GLWE of a list but the last holds lwe_per_glwe ciphertexts")
    if comp and not 0 < comp[-1].bodies <= params.lwe_per_glwe:
        raise ValueError("the last compressed GLWE of a list holds 1 .. lwe_per_glwe ciphertexts")
    if not comp:
        return np.zeros(0, dtype=np.uint64), 0
    return np.concatenate([_c_u64(c.packed).reshape(-1) for c in comp]), sum(c.bodies for c in comp)


def extract_lwe(params: PksParams, glwe: np.ndarray, index: int) -> np.ndarray:
    """LWE (dim k*N, native q) of coefficient `index` of a GLWE (tfhe-rs extract_lwe_sample_from_glwe_
    ciphertext at MonomialDegree(index); the decompression path before its PBS)."""
    k, N = params.out_k, params.out_N
    g = np.asarray(glwe, dtype=np.uint64).reshape(k + 1, N)
    out = np.zeros(k * N + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for c in range(k):
            a = g[c]
            # a'_{cN + j} = a_c[index - j] for j <= index, -a_c[N + index - j] otherwise
            j = np.arange(N)
            src = index - j
            val = np.where(src >= 0, a[np.where(src >= 0, src, 0)], np.uint64(0) - a[np.where(src < 0, src + N, 0)])
            out[c * N:(c + 1) * N] = val
    out[-1] = g[k][index]
    return out


# ---- decompression: compressed GLWEs back into compute-ready LWEs (tfhe-rs DecompressionKey) ------------------
class DecompressionKey:
    """Bootstrapping key from the post-packing GLWE key (read as an LWE key of dimension out_k * out_N) to the
    compute GLWE key; no keyswitching key.  ``params``: the compute parameters with ``n`` replaced by
    out_k * out_N -- the parameter set of the rotation-only engine.  seed None: OS entropy; an int: the
    reproducible test stream."""

    def __init__(self, compute_params: Params, pks_params: PksParams, post_packing_key: np.ndarray,
                 glwe_key: np.ndarray, seed: Optional[int]):
        self.pks_params, self.seed = pks_params, seed
        self.params = Params.from_buffer_copy(compute_params)
        self.params.n = pks_params.out_k * pks_params.out_N
        lwe, glwe = _c_u64(post_packing_key), _c_u64(glwe_key)
        if lwe.size != self.params.n or glwe.size != self.params.k * self.params.N:
            raise ValueError("DecompressionKey: key sizes do not match the parameters")
        L = lib()
        self.bsk = np.zeros(L.tfhe_hip_bsk_len(ctypes.byref(self.params)), dtype=np.uint64)
        rk = rng_key(seed)
        _check(L.tfhe_hip_server_keygen_k(ctypes.byref(self.params), ctypes.byref(rk), _u64(lwe), _u64(glwe),
                                          _u64(self.bsk), None))


class Decompressor:
    """tfhe-rs ``CompressedCiphertextList::get`` on one GPU: owns a rotation-only engine holding the decompression
    key; every ciphertext of a list comes back as an LWE under the compute GLWE key after one PBS."""

    def __init__(self, dk: DecompressionKey, device: int = 0):
        self.key, self.device = dk, device
        self.engine = Engine(dk.params, device)
        try:
            self.engine.load_bsk(dk.bsk)
        except Exception:
            self.engine.close()
            raise

    def close(self) -> None:
        self.engine.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def identity_lut(self, msg_modulus: int = 16) -> np.ndarray:
        """m -> m over msg_modulus values, one padding bit: delta = 2^64 / (2 * msg_modulus)."""
        return lut_from_table(self.key.params.N, msg_modulus, list(range(msg_modulus)), (1 << 63) // msg_modulus)

    def decompress(self, comp: List[CompressedGlwe], lut: Optional[np.ndarray] = None, msg_modulus: int = 16,
                   lut_index=None) -> np.ndarray:
        """A list of compressed GLWEs -> (count, k*N + 1) LWEs under the compute GLWE key.  lut: one table or
        (n_lut, N) with ``lut_index`` (count entries); None: the identity over ``msg_modulus`` values."""
        p, pp = self.key.params, self.key.pks_params
        packed, count = concat_list(pp, comp)
        luts = _c_u64(self.identity_lut(msg_modulus) if lut is None else lut).reshape(-1, p.N)
        li = None
        if lut_index is not None:
            li = np.ascontiguousarray(np.asarray(lut_index, dtype=np.uint32))
            if li.shape[0] != count:
                raise ValueError("lut_index must have one entry per ciphertext")
        out = np.zeros((count, p.k * p.N + 1), dtype=np.uint64)
        _check(_lib().tfhe_hip_decompress(self.engine._h, ctypes.byref(pp), _u64(packed), packed.size, count,
                                          _u64(luts), luts.shape[0],
                                          li.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if li is not None else None,
                                          _u64(out)))
        return out

    def decompress_async(self, d_packed, count: int, d_luts, d_out, d_lut_index=None, stream=None) -> None:
        """Device tensors (d_packed: the concatenated words of whole groups, d_out: (count, k*N + 1)), enqueued on
        ``stream`` (None: torch's current stream)."""
        _check(_lib().tfhe_hip_decompress_async(
            self.engine._h, ctypes.byref(self.key.pks_params), ctypes.c_void_p(d_packed.data_ptr()), d_packed.numel(),
            count, ctypes.c_void_p(d_luts.data_ptr()), d_luts.numel() // self.key.params.N,
            ctypes.c_void_p(d_lut_index.data_ptr()) if d_lut_index is not None else None,
            ctypes.c_void_p(d_out.data_ptr()), ctypes.c_void_p(_stream_handle(stream, self.device))))

    def decompress_device(self, d_packed, count: int, d_lut, d_lut_index=None):
        """decompress_async into a fresh (count, k*N + 1) tensor on torch's current stream (no host sync)."""
        p = self.key.params
        d_out = d_packed.new_empty((count, p.k * p.N + 1))
        if count:
            self.decompress_async(d_packed.contiguous(), count, d_lut, d_out, d_lut_index)
        return d_out
