"""Encrypted matrix x clear matrix, packed and compressed (include/tfhe_hip.h tfhe_hip_matmul_*; kernels
tfhe_amd/csrc/matmul.hip): the front half of the path whose back half is ``tfhe_amd.compression``.

Mirrors the reference's surface (ml/extensions/rust/src/lib_python.rs:176-428):
  create_private_key        -> PrivateKey(mp, pks_params, seed)
  encrypt_matrix            -> encrypt_matrix(pkey, X) -> EncryptedMatrix (seeds + bit-packed bodies)
  matrix_multiplication     -> MatMul(mp, packer, device).multiply(enc, ClearMatrix(...)) -> rows of CompressedGlwe
  decrypt_matrix            -> decrypt_matrix(result, pkey, C)

A user encrypts the rows of an integer matrix X (R x K), the server holds a clear int32 matrix W (K x C) and returns
the compressed encryption of X.W: expand -> dot -> packing keyswitch stay on the device, only the packed GLWEs come
back and are compressed on the host.  ``device="cpu"`` runs the same chain through the library's host functions
with a ``HostPacker`` for the packing stage, so the chain is testable without a GPU.
"""
from __future__ import annotations

import ctypes
import os
from typing import Callable, List, Optional

import numpy as np

from . import RngKey, _c_u64, _check, _stream_handle, _u64, lib, rng_key
from .compression import CompressedGlwe, CompressionKey, Packer, PksParams, compress_glwe, glwe_phase

MATMUL_PRESET_ML2048 = 0
_U64P = ctypes.POINTER(ctypes.c_uint64)
_I64P = ctypes.POINTER(ctypes.c_int64)
_I32P = ctypes.POINTER(ctypes.c_int32)
LWE_WORKSPACE_BYTES = 256 << 20  # multiply() cuts the encrypted rows into chunks whose LWEs fit this


class MatmulParams(ctypes.Structure):
    _fields_ = [("N", ctypes.c_uint32), ("bits_reserved", ctypes.c_uint32), ("in_storage_log", ctypes.c_uint32),
                ("noise_log2", ctypes.c_int32)]

    @classmethod
    def preset(cls, which: int = MATMUL_PRESET_ML2048) -> "MatmulParams":
        p = cls()
        _check(_lib().tfhe_hip_matmul_params_preset(which, ctypes.byref(p)))
        return p

    @property
    def body_words(self) -> int:
        n = _lib().tfhe_hip_matmul_body_words(ctypes.byref(self))
        if n == 0:
            raise ValueError("invalid matmul parameters")
        return n


_BOUND = None


def _lib():
    global _BOUND
    L = lib()
    if _BOUND is None:
        P, V, Z = ctypes.POINTER(MatmulParams), ctypes.c_void_p, ctypes.c_size_t
        L.tfhe_hip_matmul_params_preset.argtypes = [ctypes.c_int, P]
        L.tfhe_hip_matmul_body_words.argtypes = [P]
        L.tfhe_hip_matmul_body_words.restype = Z
        L.tfhe_hip_matmul_keygen_k.argtypes = [P, ctypes.POINTER(RngKey), _U64P]
        L.tfhe_hip_matmul_encrypt_k.argtypes = [P, _U64P, ctypes.POINTER(RngKey), ctypes.c_uint64, _U64P, _I64P, Z, _U64P]
        L.tfhe_hip_matmul_expand_host.argtypes = [P, _U64P, _U64P, Z, _U64P]
        L.tfhe_hip_matmul_dot_host.argtypes = [P, _I32P, Z, Z, _U64P, Z, Z, _U64P]
        L.tfhe_hip_matmul_decode.argtypes = [P, _U64P, Z, _I64P]
        L.tfhe_hip_matmul_create.argtypes = [P, ctypes.c_int, ctypes.POINTER(V)]
        L.tfhe_hip_matmul_destroy.argtypes = [V]
        L.tfhe_hip_matmul_destroy.restype = None
        L.tfhe_hip_matmul_matrix_create.argtypes = [V, _I32P, Z, Z, ctypes.POINTER(V)]
        L.tfhe_hip_matmul_matrix_destroy.argtypes = [V]
        L.tfhe_hip_matmul_matrix_destroy.restype = None
        L.tfhe_hip_matmul_expand_async.argtypes = [V, V, V, Z, V, V]
        L.tfhe_hip_matmul_expand.argtypes = [V, _U64P, _U64P, Z, _U64P]
        L.tfhe_hip_matmul_dot_async.argtypes = [V, V, V, Z, Z, V, V]
        L.tfhe_hip_matmul_dot.argtypes = [V, V, _U64P, Z, Z, _U64P]
        _BOUND = True
    return L


def _int32_matrix(W) -> np.ndarray:
    """A 2-D integer array as contiguous int32; ValueError if it is empty or a value falls outside int32."""
    w = np.asarray(W)
    if w.ndim != 2 or w.shape[0] == 0 or w.shape[1] == 0:
        raise ValueError("the clear matrix must be K x C with K >= 1 and C >= 1")
    if not np.issubdtype(w.dtype, np.integer):
        raise ValueError("the clear matrix must hold integers")
    if w.size and (int(w.max()) > 2 ** 31 - 1 or int(w.min()) < -2 ** 31):
        raise ValueError("the clear matrix holds a value outside int32")
    return np.ascontiguousarray(w, dtype=np.int32)


# ---- host functions ----------------------------------------------------------------------------------------
def encrypt_glwes(mp: MatmulParams, glwe_key: np.ndarray, rk: RngKey, stream0: int, seeds: np.ndarray,
                  values: np.ndarray) -> np.ndarray:
    """values (G, N) signed, seeds (G, 2) -> packed bodies (G, body_words)."""
    v = np.ascontiguousarray(values, dtype=np.int64).reshape(-1, mp.N)
    s = _c_u64(seeds).reshape(-1, 2)
    if s.shape[0] != v.shape[0]:
        raise ValueError("one seed per GLWE")
    key = _c_u64(glwe_key)
    out = np.zeros((v.shape[0], mp.body_words), dtype=np.uint64)
    _check(_lib().tfhe_hip_matmul_encrypt_k(ctypes.byref(mp), _u64(key), ctypes.byref(rk), int(stream0), _u64(s),
                                            v.ctypes.data_as(_I64P), v.shape[0], _u64(out)))
    return out


def expand_host(mp: MatmulParams, seeds: np.ndarray, packed: np.ndarray) -> np.ndarray:
    """-> (G, 2, N) GLWEs: mask from the seed, body values at the top of the word."""
    s = _c_u64(seeds).reshape(-1, 2)
    p = _c_u64(packed).reshape(s.shape[0], mp.body_words)
    out = np.zeros((s.shape[0], 2, mp.N), dtype=np.uint64)
    _check(_lib().tfhe_hip_matmul_expand_host(ctypes.byref(mp), _u64(s), _u64(p), s.shape[0], _u64(out)))
    return out


def dot_host(mp: MatmulParams, W: np.ndarray, glwes: np.ndarray, col_stride: Optional[int] = None,
             out: Optional[np.ndarray] = None) -> np.ndarray:
    """glwes (R, Kb, 2, N) times the clear K x C matrix on the CPU -> (R, col_stride, N + 1) LWEs."""
    w = _int32_matrix(W)
    K, C = w.shape
    Kb = -(-K // mp.N)
    g = _c_u64(glwes).reshape(-1, Kb, 2, mp.N)
    cs = C if col_stride is None else col_stride
    if out is None:
        out = np.zeros((g.shape[0], cs, mp.N + 1), dtype=np.uint64)
    _check(_lib().tfhe_hip_matmul_dot_host(ctypes.byref(mp), w.ctypes.data_as(_I32P), K, C, _u64(g), g.shape[0], cs,
                                           _u64(out)))
    return out


def decode(mp: MatmulParams, phases: np.ndarray) -> np.ndarray:
    p = _c_u64(phases).reshape(-1)
    out = np.zeros(p.size, dtype=np.int64)
    _check(_lib().tfhe_hip_matmul_decode(ctypes.byref(mp), _u64(p), p.size, out.ctypes.data_as(_I64P)))
    return out


# ---- client side -------------------------------------------------------------------------------------------
class PrivateKey:
    """The client's keys (lib_python.rs create_private_key): a binary GLWE key of N bits and a compression key from
    that key read as an LWE key; ``compression_key.post_packing_key`` decrypts the result.  seed None: OS entropy; an
    int: the reproducible test stream."""

    def __init__(self, mp: MatmulParams, pks_params: PksParams, seed: Optional[int], with_key: bool = True):
        if pks_params.in_dim != mp.N:
            raise ValueError("the packing keyswitch's in_dim must equal the matmul N")
        self.params, self.pks_params, self.seed = mp, pks_params, seed
        self.glwe_key = np.zeros(mp.N, dtype=np.uint64)
        rk = rng_key(seed)
        _check(_lib().tfhe_hip_matmul_keygen_k(ctypes.byref(mp), ctypes.byref(rk), _u64(self.glwe_key)))
        self.compression_key = CompressionKey(pks_params, seed, self.glwe_key, with_key=with_key)

    @property
    def post_packing_key(self) -> np.ndarray:
        return self.compression_key.post_packing_key


class EncryptedMatrix:
    """R x K values as R * Kb seeded GLWEs: seeds (R * Kb, 2), packed bodies (R * Kb, body_words)."""

    def __init__(self, mp: MatmulParams, seeds: np.ndarray, packed: np.ndarray, shape):
        self.params, self.seeds, self.packed, self.shape = mp, seeds, packed, tuple(shape)

    @property
    def blocks(self) -> int:
        return -(-self.shape[1] // self.params.N)

    @property
    def nbytes(self) -> int:
        return self.seeds.nbytes + self.packed.nbytes


def encrypt_matrix(pkey: PrivateKey, X, seed: Optional[int] = None, stream0: int = 0) -> EncryptedMatrix:
    """Encrypt the rows of the integer matrix X (R x K).  seed None: mask seeds and noise from OS entropy; an int: the
    reproducible test stream (mask seeds = words of that seed's AES-CTR stream, noise from ChaCha streams stream0 + g)."""
    mp = pkey.params
    x = np.asarray(X)
    if x.ndim != 2 or x.shape[0] == 0 or x.shape[1] == 0:
        raise ValueError("the matrix must be R x K with R >= 1 and K >= 1")
    R, K = x.shape
    Kb = -(-K // mp.N)
    v = np.zeros((R, Kb * mp.N), dtype=np.int64)
    v[:, :K] = x.astype(np.int64)
    G = R * Kb
    if seed is None:
        seeds = np.frombuffer(os.urandom(16 * G), dtype=np.uint64).reshape(G, 2).copy()
    else:
        s = np.array([seed & (2 ** 64 - 1), (seed >> 64) ^ 0x6D61746D756C], dtype=np.uint64)  # "matmul"
        seeds = np.zeros((G, 2), dtype=np.uint64)
        _check(lib().tfhe_hip_csprng_words(_u64(s), 0, seeds.size, _u64(seeds)))
    packed = encrypt_glwes(mp, pkey.glwe_key, rng_key(seed), stream0, seeds, v.reshape(G, mp.N))
    return EncryptedMatrix(mp, seeds, packed, (R, K))


def decrypt_matrix(result: List[List[CompressedGlwe]], pkey: PrivateKey, C: int) -> np.ndarray:
    """Rows of compressed GLWEs (``MatMul.multiply``) -> (R, C) int64."""
    pp = pkey.pks_params
    out = np.zeros((len(result), C), dtype=np.int64)
    for r, row in enumerate(result):
        vals = []
        for cg in row:
            phase = glwe_phase(pp.out_k, pp.out_N, pkey.post_packing_key, cg.extract())
            vals.append(decode(pkey.params, phase[:cg.bodies]))
        got = np.concatenate(vals)
        if got.size != C:
            raise ValueError(f"row {r} holds {got.size} values, expected {C}")
        out[r] = got
    return out


# ---- server side -------------------------------------------------------------------------------------------
class HostPacker:
    """The packing stage of the CPU chain: ``pack_group(lwes)`` maps up to lwe_per_glwe LWEs (count, in_dim + 1) to one
    GLWE of (k + 1) N words under ``params``."""

    def __init__(self, params: PksParams, pack_group: Callable[[np.ndarray], np.ndarray]):
        self.params, self.pack_group = params, pack_group


class ClearMatrix:
    """A clear int32 matrix W (K x C).  With a device ``MatMul`` it is uploaded once and stays resident (a model has
    many layers: several may live on one context); with a CPU one it only holds the values."""

    def __init__(self, ctx: "MatMul", W):
        self.w = _int32_matrix(W)
        self.K, self.C = self.w.shape
        self.ctx, self._h = ctx, None
        if ctx._h is not None:
            h = ctypes.c_void_p()
            _check(_lib().tfhe_hip_matmul_matrix_create(ctx._h, self.w.ctypes.data_as(_I32P), self.K, self.C,
                                                        ctypes.byref(h)))
            self._h = h
            ctx._matrices.append(self)  # closed with the context at the latest

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value and self.ctx._h is not None:
            _lib().tfhe_hip_matmul_matrix_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MatMul:
    """The server: ``MatMul(mp, packer, device)``.  device an int: a GPU ordinal and ``packer`` a ``compression.Packer``
    with its key loaded on that device; device "cpu": ``packer`` a ``HostPacker``.  Without a packer only the stage
    calls (expand, dot) work."""

    def __init__(self, mp: MatmulParams, packer=None, device=0):
        if packer is not None and packer.params.in_dim != mp.N:
            raise ValueError("the packing keyswitch's in_dim must equal the matmul N")
        mp.body_words  # ValueError on invalid parameters
        self.params, self.packer, self.device = mp, packer, device
        self.rows_per_chunk: Optional[int] = None  # override of the workspace bound (tests force 1)
        self._h = None
        self._matrices: List[ClearMatrix] = []
        if device != "cpu":
            if packer is not None and (not isinstance(packer, Packer) or packer.device != device):
                raise ValueError("a device MatMul needs a compression.Packer on the same device")
            h = ctypes.c_void_p()
            _check(_lib().tfhe_hip_matmul_create(ctypes.byref(mp), int(device), ctypes.byref(h)))
            self._h = h
        elif packer is not None and not isinstance(packer, HostPacker):
            raise ValueError("a CPU MatMul needs a HostPacker")

    def clear_matrix(self, W) -> ClearMatrix:
        return ClearMatrix(self, W)

    def close(self) -> None:
        for m in getattr(self, "_matrices", []):
            m.close()
        self._matrices = []
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib().tfhe_hip_matmul_destroy(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- stage calls on torch device tensors (int64 / uint64), enqueued on `stream` (None: torch's current stream)
    def expand_async(self, d_seeds, d_packed, G: int, d_glwes, stream=None) -> None:
        _check(_lib().tfhe_hip_matmul_expand_async(self._h, ctypes.c_void_p(d_seeds.data_ptr()),
                                                   ctypes.c_void_p(d_packed.data_ptr()), G,
                                                   ctypes.c_void_p(d_glwes.data_ptr()),
                                                   ctypes.c_void_p(_stream_handle(stream, self.device))))

    def dot_async(self, clear: ClearMatrix, d_glwes, R: int, col_stride: int, d_lwes, stream=None) -> None:
        _check(_lib().tfhe_hip_matmul_dot_async(self._h, clear._h, ctypes.c_void_p(d_glwes.data_ptr()), R, col_stride,
                                                ctypes.c_void_p(d_lwes.data_ptr()),
                                                ctypes.c_void_p(_stream_handle(stream, self.device))))

    # -- the same on host buffers, synchronous
    def expand(self, seeds: np.ndarray, packed: np.ndarray) -> np.ndarray:
        mp = self.params
        s = _c_u64(seeds).reshape(-1, 2)
        p = _c_u64(packed).reshape(s.shape[0], mp.body_words)
        out = np.zeros((s.shape[0], 2, mp.N), dtype=np.uint64)
        _check(_lib().tfhe_hip_matmul_expand(self._h, _u64(s), _u64(p), s.shape[0], _u64(out)))
        return out

    def dot(self, clear: ClearMatrix, glwes: np.ndarray, col_stride: Optional[int] = None,
            out: Optional[np.ndarray] = None) -> np.ndarray:
        """glwes (R, Kb, 2, N) -> (R, col_stride, N + 1); with ``out`` given, its LWEs C .. col_stride - 1 are kept."""
        mp = self.params
        g = _c_u64(glwes).reshape(-1, -(-clear.K // mp.N), 2, mp.N)
        cs = clear.C if col_stride is None else col_stride
        if out is None:
            out = np.zeros((g.shape[0], cs, mp.N + 1), dtype=np.uint64)
        _check(_lib().tfhe_hip_matmul_dot(self._h, clear._h, _u64(g), g.shape[0], cs, _u64(out)))
        return out

    def _rows_per_chunk(self, R: int, col_stride: int) -> int:
        if self.rows_per_chunk is not None:
            return max(1, min(R, int(self.rows_per_chunk)))
        return max(1, min(R, LWE_WORKSPACE_BYTES // (col_stride * (self.params.N + 1) * 8)))

    def multiply(self, enc: EncryptedMatrix, clear: ClearMatrix) -> List[List[CompressedGlwe]]:
        """-> one list of CompressedGlwe per encrypted row: ceil(C / lwe_per_glwe) groups, the last one holding the
        remainder (groups never straddle two rows)."""
        if self.packer is None:
            raise ValueError("multiply needs a packer")
        mp, pp = self.params, self.packer.params
        R, K = enc.shape
        if clear.ctx is not self or K != clear.K:
            raise ValueError("the clear matrix belongs to another MatMul or its K differs from the encrypted matrix's")
        lpg, C = pp.lwe_per_glwe, clear.C
        groups = -(-C // lpg)
        if self._h is None:
            glwes = self._multiply_cpu(enc, clear, groups)
        else:
            glwes = self._multiply_device(enc, clear, groups)
        return [[compress_glwe(pp, glwes[r, g], min(lpg, C - g * lpg)) for g in range(groups)] for r in range(R)]

    def _multiply_cpu(self, enc, clear, groups) -> np.ndarray:
        mp, pp = self.params, self.packer.params
        R, lpg = enc.shape[0], pp.lwe_per_glwe
        lwes = dot_host(mp, clear.w, expand_host(mp, enc.seeds, enc.packed).reshape(R, enc.blocks, 2, mp.N))
        out = np.zeros((R, groups, pp.glwe_len), dtype=np.uint64)
        for r in range(R):
            for g in range(groups):
                out[r, g] = self.packer.pack_group(lwes[r, g * lpg:(g + 1) * lpg])
        return out

    def _multiply_device(self, enc, clear, groups) -> np.ndarray:
        import torch
        mp, pp = self.params, self.packer.params
        R, Kb, lpg = enc.shape[0], enc.blocks, pp.lwe_per_glwe
        col_stride = groups * lpg
        dev = torch.device("cuda", self.device)
        rows = self._rows_per_chunk(R, col_stride)
        d_seeds = torch.from_numpy(_c_u64(enc.seeds).view(np.int64)).to(dev)
        d_packed = torch.from_numpy(_c_u64(enc.packed).view(np.int64)).to(dev)
        with torch.cuda.device(dev):
            d_glwes = torch.empty((rows * Kb, 2, mp.N), dtype=torch.int64, device=dev)
            # zero once: the dot never writes the LWEs C .. col_stride - 1 of a row, and a zero LWE adds nothing
            d_lwes = torch.zeros((rows, col_stride, mp.N + 1), dtype=torch.int64, device=dev)
            d_out = torch.empty((R * groups, pp.glwe_len), dtype=torch.int64, device=dev)
            for r0 in range(0, R, rows):
                n = min(rows, R - r0)
                self.expand_async(d_seeds[r0 * Kb:], d_packed[r0 * Kb:], n * Kb, d_glwes)
                self.dot_async(clear, d_glwes, n, col_stride, d_lwes)
                self.packer.pack_async(d_lwes, n * col_stride, d_out[r0 * groups:])
            out = d_out.cpu().numpy().view(np.uint64)
        return out.reshape(R, groups, pp.glwe_len)
