"""tfhe_amd — MI355X-native TFHE programmable bootstrapping, Python host side.

A thin ctypes layer over ``libtfhe_hip.so`` (C ABI: ``include/tfhe_hip.h``) plus a host-side
mirror of the reference's operator surface for this path:

* ``ClientKey`` / ``ServerKey`` / ``gen_keys`` — tfhe-rs ``gen_keys(PARAMS)`` as used by
  ``ml/biometrics/notebooks/main.rs:48`` and ``TfheClientKey.generate`` (sdk/relayer/src/tfhe.ts:20-28).
* ``Engine.generate_accumulator(f)`` + ``Engine.keyswitch_programmable_bootstrap(ct, acc)`` —
  ``ServerKey::generate_accumulator`` / ``keyswitch_programmable_bootstrap``
  (ml/biometrics/notebooks/main.rs:65-71), batched.
* ``FheBool`` gate bootstrapping (nand/and/or/xor/not) — the ``FheBool`` operator surface of
  packages/wasm (tfhe-rs high-level API) used by the Solidity ``fheBitAnd`` etc.
* ``FheUint8`` — 8 boolean ciphertexts; ``map_bits`` evaluates one LUT per bit (8 PBS / value).

Every compute call goes to the HIP library; there is no CPU fallback.  If the library is
missing the import of the engine raises ``RuntimeError``.
"""
from __future__ import annotations

import ctypes
import os
from typing import Callable, Optional, Sequence

import numpy as np

__all__ = [
    "Params", "TfheError", "lib", "ClientKey", "ServerKey", "gen_keys", "Engine", "FheBool", "FheUint8",
    "PRESET_GATE", "PRESET_FHEVM", "PRESET_GATE_FFT", "PRESET_FHEVM_FFT", "PRESET_FHEVM_MB_FFT", "TRANSFORM_NTT", "TRANSFORM_FFT64", "MU", "encode_bool",
    "decode_bool",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
# TFHE_HIP_LIB overrides the in-tree library (A/B builds of kernel variants in tools/ab.sh).
LIB_PATH = os.environ.get("TFHE_HIP_LIB") or os.path.join(_HERE, "libtfhe_hip.so")
PRESET_GATE = 0
PRESET_FHEVM = 1
PRESET_GATE_FFT = 2  # P-GATE on the FFT64 transform (tfhe-rs's f64-FFT external product)
PRESET_FHEVM_FFT = 3  # P-FHEVM on the FFT64 transform (N = 2048 as two 512-point halves)
PRESET_FHEVM_MB_FFT = 4  # preset 3 with n = 924 (divisible by 2, 3 and 4): multi-bit PBS keys (gen_keys grouping=;
                         # documented default grouping 3, the fastest at a batch of 32: DESIGN §4o)
TRANSFORM_NTT = 0
TRANSFORM_FFT64 = 1
MU = 1 << 61  # gate encoding: true = +1/8, false = -1/8 of the 2^64 torus
_U64P = ctypes.POINTER(ctypes.c_uint64)
_U32P = ctypes.POINTER(ctypes.c_uint32)

_ERRORS = {-1: "EINVAL", -2: "ENOMEM", -3: "EDEVICE", -4: "ENOKEYS", -5: "EUNSUPPORTED"}


class TfheError(RuntimeError):
    """Raised for a negative status from the C ABI (``code`` holds the TFHE_HIP_E* value)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"{_ERRORS.get(code, code)}: {msg}")
        self.code = code


class Params(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint32), ("k", ctypes.c_uint32), ("N", ctypes.c_uint32),
        ("pbs_base_log", ctypes.c_uint32), ("pbs_level", ctypes.c_uint32),
        ("ks_base_log", ctypes.c_uint32), ("ks_level", ctypes.c_uint32),
        ("lwe_noise_log2", ctypes.c_int32), ("glwe_noise_log2", ctypes.c_int32),
        ("order", ctypes.c_uint32), ("transform", ctypes.c_uint32),
    ]

    @classmethod
    def preset(cls, which: int = PRESET_GATE) -> "Params":
        p = cls()
        _check(lib().tfhe_hip_params_preset(which, ctypes.byref(p)))
        return p

    @property
    def io_dim(self) -> int:
        return self.n if self.order == 0 else self.k * self.N

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_}


class RngKey(ctypes.Structure):
    """192-bit ChaCha20 key material (tfhe_rng_key)."""
    _fields_ = [("w", ctypes.c_uint32 * 6)]


def rng_key(seed: Optional[int] = None) -> RngKey:
    """seed None: 192 bits of OS entropy (production keys and encryptions); an int: the REPRODUCIBLE
    seeded stream that tests, golden vectors and the oracle use (public knowledge -- test data only)."""
    k = RngKey()
    if seed is None:
        _check(lib().tfhe_hip_rng_key_entropy(ctypes.byref(k)))
    else:
        _check(lib().tfhe_hip_rng_key_from_seed(ctypes.c_uint64(seed), ctypes.byref(k)))
    return k


_LIB = None

# Every symbol declared in include/tfhe_hip.h (tests check the .so exports all of them).
ABI_SYMBOLS = (
    "tfhe_hip_params_preset", "tfhe_hip_bsk_len", "tfhe_hip_ksk_len", "tfhe_hip_io_dim", "tfhe_hip_keygen",
    "tfhe_hip_lwe_encrypt", "tfhe_hip_lwe_phase", "tfhe_hip_lut_constant", "tfhe_hip_lut_from_table",
    "tfhe_hip_create", "tfhe_hip_destroy", "tfhe_hip_last_error", "tfhe_hip_device", "tfhe_hip_load_keys",
    "tfhe_hip_load_keys_device", "tfhe_hip_pbs", "tfhe_hip_pbs_async", "tfhe_hip_blind_rotate",
    "tfhe_hip_sample_extract", "tfhe_hip_keyswitch", "tfhe_hip_ntt_fwd", "tfhe_hip_ntt_inv", "tfhe_hip_nand",
    "tfhe_hip_sync", "tfhe_hip_timing_enable", "tfhe_hip_timing_reset", "tfhe_hip_timing_stats",
    "tfhe_hip_server_keygen", "tfhe_hip_set_latency_batch", "tfhe_hip_ms_zeros_keygen", "tfhe_hip_load_ms_key",
    "tfhe_hip_ms_reduce", "tfhe_hip_pks_params_preset", "tfhe_hip_pksk_len", "tfhe_hip_pks_keygen", "tfhe_hip_pks_keygen_k", "tfhe_hip_bcast_plan",
    "tfhe_hip_pks_create", "tfhe_hip_pks_destroy", "tfhe_hip_pks_load_key", "tfhe_hip_pks_pack",
    "tfhe_hip_pks_pack_async", "tfhe_hip_pks_packed_words", "tfhe_hip_pks_compress", "tfhe_hip_pks_extract",
    "tfhe_hip_glwe_phase", "tfhe_hip_sns_params_preset", "tfhe_hip_sns_bsk_len", "tfhe_hip_sns_keygen", "tfhe_hip_sns_keygen_k",
    "tfhe_hip_sns_create", "tfhe_hip_sns_destroy", "tfhe_hip_sns_load_key", "tfhe_hip_sns_squash",
    "tfhe_hip_sns_squash_async", "tfhe_hip_sns_blind_rotate", "tfhe_hip_sns_phase", "tfhe_hip_fft_fwd",
    "tfhe_hip_fft_inv", "tfhe_hip_rng_key_entropy", "tfhe_hip_rng_key_from_seed", "tfhe_hip_keygen_k",
    "tfhe_hip_server_keygen_k", "tfhe_hip_ms_zeros_keygen_k", "tfhe_hip_lwe_encrypt_k", "tfhe_hip_ndev",
    "tfhe_hip_device_at", "tfhe_hip_key_bcast_mode", "tfhe_hip_br_kernel", "tfhe_hip_aes128_block",
    "tfhe_hip_csprng_words", "tfhe_hip_seeded_server_keygen_k", "tfhe_hip_seeded_lwe_list_k", "tfhe_hip_decompress_bsk",
    "tfhe_hip_decompress_ksk", "tfhe_hip_decompress_lwe_list", "tfhe_hip_pbs_many", "tfhe_hip_pbs_many_async",
    "tfhe_hip_sample_extract_many", "tfhe_hip_load_bsk", "tfhe_hip_load_bsk_device", "tfhe_hip_bootstrap",
    "tfhe_hip_bootstrap_async", "tfhe_hip_pks_unpack_extract", "tfhe_hip_pks_unpack_extract_async",
    "tfhe_hip_decompress", "tfhe_hip_decompress_async", "tfhe_hip_compact_list_words", "tfhe_hip_expand_compact",
    "tfhe_hip_expand_compact_async", "tfhe_hip_expand_cast", "tfhe_hip_expand_cast_async",
    "tfhe_hip_sns_pks_params_preset", "tfhe_hip_sns_pksk_len", "tfhe_hip_sns_pks_keygen", "tfhe_hip_sns_pks_keygen_k",
    "tfhe_hip_sns_pks_create", "tfhe_hip_sns_pks_destroy", "tfhe_hip_sns_pks_load_key", "tfhe_hip_sns_pks_pack",
    "tfhe_hip_sns_pks_pack_async", "tfhe_hip_sns_pks_pack_host", "tfhe_hip_sns_pks_packed_words",
    "tfhe_hip_sns_pks_compress", "tfhe_hip_sns_pks_extract", "tfhe_hip_glwe_phase128",
    "tfhe_hip_sns_seeded_bodies_len", "tfhe_hip_sns_seeded_keygen", "tfhe_hip_sns_seeded_keygen_k",
    "tfhe_hip_sns_decompress_bsk", "tfhe_hip_csprng_words128", "tfhe_hip_sns_load_key_seeded",
    "tfhe_hip_sns_seeded_load_stats", "tfhe_hip_sns_seeded_expand_bsk", "tfhe_hip_sns_pks_seeded_bodies_len",
    "tfhe_hip_sns_pks_seeded_keygen", "tfhe_hip_sns_pks_seeded_keygen_k", "tfhe_hip_sns_pks_decompress_key",
    "tfhe_hip_sns_pks_load_key_seeded", "tfhe_hip_sns_pks_seeded_load_stats", "tfhe_hip_sns_pks_seeded_expand_key",
    "tfhe_hip_lut_oprf", "tfhe_hip_csprng_rows", "tfhe_hip_csprng_rows_async", "tfhe_hip_oprf", "tfhe_hip_oprf_async",
    "tfhe_hip_lwe_lincomb", "tfhe_hip_lwe_lincomb_async", "tfhe_hip_lincomb_pbs_async",
    "tfhe_hip_matmul_params_preset", "tfhe_hip_matmul_body_words", "tfhe_hip_matmul_keygen_k", "tfhe_hip_matmul_encrypt_k",
    "tfhe_hip_matmul_expand_host", "tfhe_hip_matmul_dot_host", "tfhe_hip_matmul_decode", "tfhe_hip_matmul_create",
    "tfhe_hip_matmul_destroy", "tfhe_hip_matmul_matrix_create", "tfhe_hip_matmul_matrix_destroy",
    "tfhe_hip_matmul_expand_async", "tfhe_hip_matmul_expand", "tfhe_hip_matmul_dot_async", "tfhe_hip_matmul_dot",
    "tfhe_hip_mb_bsk_len", "tfhe_hip_mb_server_keygen_k", "tfhe_hip_mb_server_keygen", "tfhe_hip_load_keys_mb",
    "tfhe_hip_grouping", "tfhe_hip_seeded_mb_bodies_len", "tfhe_hip_seeded_mb_server_keygen_k",
    "tfhe_hip_decompress_bsk_mb", "tfhe_hip_load_keys_seeded", "tfhe_hip_load_bsk_seeded",
    "tfhe_hip_load_keys_mb_seeded", "tfhe_hip_load_ms_key_seeded", "tfhe_hip_seeded_load_stats",
    "tfhe_hip_seeded_expand_bsk", "tfhe_hip_seeded_expand_ksk", "tfhe_hip_seeded_expand_lwe_list",
)

# P-FHEVM modulus-switch noise reduction key (include/tfhe_hip.h TFHE_HIP_MS_FHEVM_*)
MS_FHEVM = dict(count=1449, bound=2.0 ** 58, r_sigma=13.179852282053789, input_variance=2.63039184094559e-07)


def _share_hip_runtime_with_torch() -> None:
    """torch (ROCm wheel) bundles its own libamdhip64 (SONAME libamdhip64.so.7) and loads it by the
    unversioned file name.  If libtfhe_hip.so were loaded first, /opt/rocm's copy would come in under
    the same SONAME and torch would then load a SECOND HIP runtime into the process (torch.cuda then
    reports "No HIP GPUs are available").  Importing torch first makes our NEEDED libamdhip64.so.7
    resolve to the copy torch already loaded: one HIP runtime per process.  Without torch the
    library uses /opt/rocm's runtime (RUNPATH)."""
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def lib():
    """Load libtfhe_hip.so (built in-tree by ``make -C tfhe_amd``).  Raises if it is missing."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built: run `make -C tfhe_amd` (or __graft_entry__.build())")
        _share_hip_runtime_with_torch()
        L = ctypes.CDLL(LIB_PATH)
        L.tfhe_hip_last_error.restype = ctypes.c_char_p
        L.tfhe_hip_bsk_len.restype = ctypes.c_size_t
        L.tfhe_hip_ksk_len.restype = ctypes.c_size_t
        L.tfhe_hip_io_dim.restype = ctypes.c_uint32
        L.tfhe_hip_destroy.restype = None
        L.tfhe_hip_keygen.argtypes = [ctypes.c_void_p, ctypes.c_uint64, _U64P, _U64P, _U64P, _U64P]
        L.tfhe_hip_server_keygen.argtypes = [ctypes.c_void_p, ctypes.c_uint64, _U64P, _U64P, _U64P, _U64P]
        L.tfhe_hip_ms_zeros_keygen.argtypes = [ctypes.c_void_p, ctypes.c_uint64, _U64P, ctypes.c_uint32, _U64P]
        L.tfhe_hip_load_ms_key.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_uint32, ctypes.c_double, ctypes.c_double,
                                           ctypes.c_double]
        L.tfhe_hip_ms_reduce.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, _U64P,
                                         ctypes.POINTER(ctypes.c_int32)]
        L.tfhe_hip_lwe_encrypt.argtypes = [ctypes.c_uint32, _U64P, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64,
                                           _U64P, ctypes.c_size_t, _U64P]
        L.tfhe_hip_lwe_phase.argtypes = [ctypes.c_uint32, _U64P, _U64P, ctypes.c_size_t, _U64P]
        L.tfhe_hip_lut_constant.argtypes = [ctypes.c_uint32, ctypes.c_uint64, _U64P]
        L.tfhe_hip_lut_from_table.argtypes = [ctypes.c_uint32, ctypes.c_uint32, _U64P, ctypes.c_uint64, _U64P]
        L.tfhe_hip_create.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_void_p)]
        L.tfhe_hip_ndev.argtypes = [ctypes.c_void_p]
        L.tfhe_hip_device_at.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.tfhe_hip_key_bcast_mode.argtypes = [ctypes.c_void_p]
        L.tfhe_hip_br_kernel.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
        L.tfhe_hip_br_kernel.restype = ctypes.c_char_p
        _RKP = ctypes.POINTER(RngKey)
        L.tfhe_hip_rng_key_entropy.argtypes = [_RKP]
        L.tfhe_hip_rng_key_from_seed.argtypes = [ctypes.c_uint64, _RKP]
        L.tfhe_hip_keygen_k.argtypes = [ctypes.c_void_p, _RKP, _U64P, _U64P, _U64P, _U64P]
        L.tfhe_hip_server_keygen_k.argtypes = [ctypes.c_void_p, _RKP, _U64P, _U64P, _U64P, _U64P]
        L.tfhe_hip_ms_zeros_keygen_k.argtypes = [ctypes.c_void_p, _RKP, _U64P, ctypes.c_uint32, _U64P]
        L.tfhe_hip_mb_bsk_len.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.tfhe_hip_mb_bsk_len.restype = ctypes.c_size_t
        L.tfhe_hip_mb_server_keygen_k.argtypes = [ctypes.c_void_p, ctypes.c_uint32, _RKP, _U64P, _U64P, _U64P, _U64P]
        L.tfhe_hip_mb_server_keygen.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, _U64P, _U64P, _U64P,
                                                _U64P]
        L.tfhe_hip_load_keys_mb.argtypes = [ctypes.c_void_p, ctypes.c_uint32, _U64P, ctypes.c_size_t, _U64P,
                                            ctypes.c_size_t]
        L.tfhe_hip_grouping.argtypes = [ctypes.c_void_p]
        L.tfhe_hip_seeded_mb_bodies_len.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.tfhe_hip_seeded_mb_bodies_len.restype = ctypes.c_size_t
        L.tfhe_hip_seeded_mb_server_keygen_k.argtypes = [ctypes.c_void_p, ctypes.c_uint32, _RKP, _U64P, _U64P, _U64P, _U64P]
        L.tfhe_hip_decompress_bsk_mb.argtypes = [ctypes.c_void_p, ctypes.c_uint32, _U64P, _U64P, _U64P]
        L.tfhe_hip_load_keys_seeded.argtypes = [ctypes.c_void_p, _U64P, _U64P, ctypes.c_size_t, _U64P, _U64P,
                                                ctypes.c_size_t]
        L.tfhe_hip_load_bsk_seeded.argtypes = [ctypes.c_void_p, _U64P, _U64P, ctypes.c_size_t]
        L.tfhe_hip_load_keys_mb_seeded.argtypes = [ctypes.c_void_p, ctypes.c_uint32, _U64P, _U64P, ctypes.c_size_t, _U64P,
                                                   _U64P, ctypes.c_size_t]
        L.tfhe_hip_load_ms_key_seeded.argtypes = [ctypes.c_void_p, _U64P, _U64P, ctypes.c_uint32, ctypes.c_double,
                                                  ctypes.c_double, ctypes.c_double]
        _dp = ctypes.POINTER(ctypes.c_double)
        L.tfhe_hip_seeded_load_stats.argtypes = [ctypes.c_void_p, _dp, _dp, _dp]
        L.tfhe_hip_seeded_expand_bsk.argtypes = [ctypes.c_void_p, ctypes.c_uint32, _U64P, _U64P, _U64P]
        L.tfhe_hip_seeded_expand_ksk.argtypes = [ctypes.c_void_p, _U64P, _U64P, _U64P]
        L.tfhe_hip_seeded_expand_lwe_list.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, _U64P, _U64P,
                                                      _U64P]
        L.tfhe_hip_aes128_block.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p]
        L.tfhe_hip_csprng_words.argtypes = [_U64P, ctypes.c_uint64, ctypes.c_size_t, _U64P]
        L.tfhe_hip_seeded_server_keygen_k.argtypes = [ctypes.c_void_p, _RKP, _U64P, _U64P, _U64P, _U64P, _U64P, _U64P]
        L.tfhe_hip_seeded_lwe_list_k.argtypes = [ctypes.c_uint32, ctypes.c_uint32, _U64P, ctypes.c_int32, _RKP,
                                                 ctypes.c_uint64, _U64P, _U64P, _U64P]
        L.tfhe_hip_decompress_bsk.argtypes = [ctypes.c_void_p, _U64P, _U64P, _U64P]
        L.tfhe_hip_decompress_ksk.argtypes = [ctypes.c_void_p, _U64P, _U64P, _U64P]
        L.tfhe_hip_decompress_lwe_list.argtypes = [ctypes.c_uint32, ctypes.c_uint32, _U64P, _U64P, _U64P]
        L.tfhe_hip_lwe_encrypt_k.argtypes = [ctypes.c_uint32, _U64P, ctypes.c_int32, _RKP, ctypes.c_uint64, _U64P,
                                             ctypes.c_size_t, _U64P]
        L.tfhe_hip_destroy.argtypes = [ctypes.c_void_p]
        L.tfhe_hip_load_keys.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, _U64P, ctypes.c_size_t]
        L.tfhe_hip_load_keys_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                ctypes.c_size_t]
        L.tfhe_hip_load_bsk.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t]
        L.tfhe_hip_load_bsk_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        L.tfhe_hip_pbs.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, _U64P, ctypes.c_size_t, _U32P, _U64P]
        L.tfhe_hip_bootstrap.argtypes = L.tfhe_hip_pbs.argtypes
        L.tfhe_hip_bootstrap_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                               ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.tfhe_hip_fft_fwd.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, ctypes.c_void_p]
        L.tfhe_hip_fft_inv.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.tfhe_hip_pbs_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                         ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.tfhe_hip_blind_rotate.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, _U64P, ctypes.c_size_t, _U32P,
                                            _U64P]
        L.tfhe_hip_sample_extract.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, _U64P]
        L.tfhe_hip_pbs_many.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, _U64P, ctypes.c_size_t, _U32P,
                                        ctypes.c_uint32, ctypes.c_uint32, _U64P]
        L.tfhe_hip_pbs_many_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                              ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.c_void_p, ctypes.c_void_p]
        L.tfhe_hip_sample_extract_many.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, ctypes.c_uint32,
                                                   ctypes.c_uint32, _U64P]
        L.tfhe_hip_keyswitch.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, _U64P]
        L.tfhe_hip_ntt_fwd.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t]
        L.tfhe_hip_ntt_inv.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t]
        L.tfhe_hip_nand.argtypes = [ctypes.c_void_p, _U64P, _U64P, ctypes.c_size_t, _U64P]
        L.tfhe_hip_sync.argtypes = [ctypes.c_void_p]
        L.tfhe_hip_timing_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.tfhe_hip_timing_reset.argtypes = [ctypes.c_void_p]
        L.tfhe_hip_timing_stats.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_int)]
        L.tfhe_hip_device.argtypes = [ctypes.c_void_p]
        L.tfhe_hip_compact_list_words.argtypes = [ctypes.c_uint32, ctypes.c_size_t]
        L.tfhe_hip_compact_list_words.restype = ctypes.c_size_t
        L.tfhe_hip_expand_compact.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_size_t,
                                              ctypes.c_uint32, ctypes.c_size_t, _U64P]
        L.tfhe_hip_expand_compact_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                                                    ctypes.c_size_t, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_void_p,
                                                    ctypes.c_void_p]
        L.tfhe_hip_expand_cast.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32,
                                           ctypes.c_size_t, _U64P, ctypes.c_size_t, _U32P, _U64P]
        L.tfhe_hip_expand_cast_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                                 ctypes.c_uint32, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.tfhe_hip_lut_oprf.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _U64P, _U64P]
        L.tfhe_hip_csprng_rows.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32,
                                           _U64P]
        L.tfhe_hip_csprng_rows_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64,
                                                 ctypes.c_uint32, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        L.tfhe_hip_oprf.argtypes = [ctypes.c_void_p, _U64P, ctypes.c_size_t, _U64P, _U64P, ctypes.c_size_t, _U32P,
                                    _U64P]
        L.tfhe_hip_oprf_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p]
        _terms = [_U32P, _U32P, _U32P, _U64P, _U64P, ctypes.c_size_t]  # row_start, term_buf, term_row, term_coef, bias, rows
        _bufs = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t]
        L.tfhe_hip_lwe_lincomb.argtypes = [ctypes.c_void_p, ctypes.c_uint32, _U64P, ctypes.c_size_t, _U32P, _U32P, _U64P,
                                           _U64P, ctypes.c_size_t, _U64P]
        L.tfhe_hip_lwe_lincomb_async.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + _bufs + _terms + [
            ctypes.c_void_p, ctypes.c_void_p]
        L.tfhe_hip_lincomb_pbs_async.argtypes = [ctypes.c_void_p] + _bufs + _terms + [
            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _LIB = L
    return _LIB


def source_id() -> str:
    """Content hash of everything that goes into libtfhe_hip.so (kernel + host sources, build flags,
    the ABI header).  Profiles under profiles/ carry the source_id of the tree they were measured on;
    bench.py only uses counter figures whose source_id equals the running tree's (a stale profile of
    another build is never reported as this build's)."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(_HERE, "csrc")
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc))
    files += [os.path.join(_HERE, "Makefile"), os.path.join(os.path.dirname(_HERE), "include", "tfhe_hip.h")]
    for f in files:
        h.update(os.path.relpath(f, os.path.dirname(_HERE)).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


NULL_STREAM = ctypes.c_void_p(-1).value  # TFHE_HIP_NULL_STREAM: the device's legacy null stream


def _stream_handle(stream, device: int) -> int:
    """torch.cuda.Stream / raw handle / None (torch's current stream) -> the C-ABI stream argument.
    torch's default stream has handle 0, which the C ABI reads as "ctx stream": map it to
    TFHE_HIP_NULL_STREAM so the work really is ordered with torch's default stream."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(device)
    h = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream or 0)
    return h if h else NULL_STREAM


def _check(rc: int) -> None:
    if rc != 0:
        raise TfheError(rc, lib().tfhe_hip_last_error().decode(errors="replace"))


def _u64(a: np.ndarray):
    return a.ctypes.data_as(_U64P)


def _c_u64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


def _dptr(t):
    """The C argument of an optional device tensor: its address, or a null pointer for None."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _lut_index(lut_index, rows: int, noun: str):
    """The C argument of the optional ``lut_index`` of a host entry point: contiguous uint32, one entry per row (each
    ``noun`` of the call), or a null pointer for None.  The pointer keeps its array alive."""
    if lut_index is None:
        return None
    li = np.ascontiguousarray(np.asarray(lut_index, dtype=np.uint32))
    if li.shape[0] != rows:
        raise ValueError(f"lut_index must have one entry per {noun}")
    return li.ctypes.data_as(_U32P)


def encode_bool(b) -> np.ndarray:
    b = np.asarray(b, dtype=bool)
    return np.where(b, np.uint64(MU), np.uint64((1 << 64) - MU)).astype(np.uint64)


def decode_bool(phase) -> np.ndarray:
    return np.asarray(phase, dtype=np.uint64) < np.uint64(1 << 63)


# --------------------------------------------------------------------------------------- keys
class ClientKey:
    """Secret key material: LWE key s (dim n) and GLWE key S (k*N).  ``seed`` is the test seed the keys
    were derived from, or None for keys drawn from OS entropy."""

    def __init__(self, params: Params, seed: Optional[int], lwe_key: np.ndarray, glwe_key: np.ndarray):
        self.params, self.seed, self.lwe_key, self.glwe_key = params, seed, lwe_key, glwe_key

    # keys of the PBS input/output ciphertexts
    @property
    def io_key(self) -> np.ndarray:
        return self.lwe_key if self.params.order == 0 else self.glwe_key

    @property
    def io_noise_log2(self) -> int:
        return self.params.lwe_noise_log2 if self.params.order == 0 else self.params.glwe_noise_log2

    def encrypt_torus(self, msgs, seed: Optional[int] = None, stream0: int = 0) -> np.ndarray:
        """seed None (default): masks and noise from a fresh 192-bit OS-entropy ChaCha key per call;
        an int seed: the reproducible test stream (ciphertext q on stream stream0 + q)."""
        m = _c_u64(msgs).reshape(-1)
        dim = self.params.io_dim
        out = np.zeros((m.shape[0], dim + 1), dtype=np.uint64)
        key = _c_u64(self.io_key)
        rk = rng_key(seed)
        _check(lib().tfhe_hip_lwe_encrypt_k(dim, _u64(key), self.io_noise_log2, ctypes.byref(rk), stream0, _u64(m),
                                            m.shape[0], _u64(out)))
        return out

    def phase(self, cts: np.ndarray, key: Optional[np.ndarray] = None) -> np.ndarray:
        key = _c_u64(self.io_key if key is None else key)
        dim = key.shape[0]
        cts = _c_u64(cts).reshape(-1, dim + 1)
        out = np.zeros(cts.shape[0], dtype=np.uint64)
        _check(lib().tfhe_hip_lwe_phase(dim, _u64(key), _u64(cts), cts.shape[0], _u64(out)))
        return out

    def encrypt_bool(self, bits, seed: Optional[int] = None, stream0: int = 0) -> np.ndarray:
        return self.encrypt_torus(encode_bool(bits), seed, stream0)

    def decrypt_bool(self, cts) -> np.ndarray:
        return decode_bool(self.phase(cts))

    def encrypt(self, msgs, msg_modulus: int, seed: Optional[int] = None, stream0: int = 0) -> np.ndarray:
        """Shortint-style encoding with one padding bit: m * 2^63 / msg_modulus (encryption.rs:5-22)."""
        delta = (1 << 63) // msg_modulus
        m = (np.asarray(msgs, dtype=np.uint64) % np.uint64(msg_modulus)) * np.uint64(delta)
        return self.encrypt_torus(m, seed, stream0)

    def decrypt(self, cts, msg_modulus: int) -> np.ndarray:
        """closest_representable(phase) / delta mod msg_modulus (encryption.rs:176-203)."""
        delta = (1 << 63) // msg_modulus
        ph = self.phase(cts).astype(object)
        return np.array([((int(v) + delta // 2) // delta) % msg_modulus for v in ph], dtype=np.uint64)


class ServerKey:
    """Public evaluation keys in the standard domain: BSK over Z_p and KSK over Z_2^64; for KS -> PBS
    parameter sets (P-FHEVM) also the modulus-switch noise-reduction zeros (count x (n+1)).  ``grouping`` > 1: ``bsk``
    is a multi-bit key of that grouping factor (include/tfhe_hip.h), ``ksk`` may be None (rotation-only) and there
    are no zeros (the noise-reduction pick is defined for the per-element switch)."""

    def __init__(self, params: Params, bsk: np.ndarray, ksk: np.ndarray, ms_zeros: Optional[np.ndarray] = None,
                 grouping: int = 1):
        self.params, self.bsk, self.ksk, self.ms_zeros, self.grouping = params, bsk, ksk, ms_zeros, int(grouping)


def ms_zeros_keygen(params: Params, seed: Optional[int], lwe_key: np.ndarray,
                    count: int = MS_FHEVM["count"]) -> np.ndarray:
    """Encryptions of zero under the small key for the modulus-switch noise reduction (seed None:
    OS entropy)."""
    z = np.zeros((count, params.n + 1), dtype=np.uint64)
    lwe = _c_u64(lwe_key)
    rk = rng_key(seed)
    _check(lib().tfhe_hip_ms_zeros_keygen_k(ctypes.byref(params), ctypes.byref(rk), _u64(lwe), count, _u64(z)))
    return z


def _mb_server_key(p: Params, rk: RngKey, lwe: np.ndarray, glwe: np.ndarray, grouping: int) -> ServerKey:
    L = lib()
    g = int(grouping)
    if not 0 <= g < 1 << 32:
        raise ValueError(f"grouping = {grouping} must fit 32 bits")
    bsk = np.zeros(max(L.tfhe_hip_mb_bsk_len(ctypes.byref(p), g), 1), dtype=np.uint64)
    ksk = np.zeros(L.tfhe_hip_ksk_len(ctypes.byref(p)), dtype=np.uint64)
    _check(L.tfhe_hip_mb_server_keygen_k(ctypes.byref(p), g, ctypes.byref(rk), _u64(lwe), _u64(glwe), _u64(bsk),
                                         _u64(ksk)))
    return ServerKey(p, bsk, ksk, None, grouping=g)


def gen_keys(params: Optional[Params] = None, seed: Optional[int] = None, with_server_key: bool = True,
             grouping: int = 1):
    """Key generation (tfhe-rs ``gen_keys`` analogue).  Returns (ClientKey, ServerKey).

    seed None (default): every key and the server-key randomness come from a fresh 192-bit OS-entropy
    ChaCha20 key.  An int seed gives the REPRODUCIBLE test key set (same streams as the oracle) --
    anyone who knows the seed knows the secret key, so seeded keys are for tests and benchmarks only.

    grouping 2, 3 or 4: a multi-bit server key of that grouping factor (the same secret keys and KSK as grouping 1)."""
    params = params or Params.preset(PRESET_GATE)
    L = lib()
    lwe = np.zeros(params.n, dtype=np.uint64)
    glwe = np.zeros(params.k * params.N, dtype=np.uint64)
    bsk = ksk = None
    if with_server_key and grouping != 1:
        rk = rng_key(seed)
        _check(L.tfhe_hip_keygen_k(ctypes.byref(params), ctypes.byref(rk), _u64(lwe), _u64(glwe), None, None))
        return ClientKey(params, seed, lwe, glwe), _mb_server_key(params, rk, lwe, glwe, grouping)
    if with_server_key:
        bsk = np.zeros(L.tfhe_hip_bsk_len(ctypes.byref(params)), dtype=np.uint64)
        ksk = np.zeros(L.tfhe_hip_ksk_len(ctypes.byref(params)), dtype=np.uint64)
    rk = rng_key(seed)
    _check(L.tfhe_hip_keygen_k(ctypes.byref(params), ctypes.byref(rk), _u64(lwe), _u64(glwe),
                               _u64(bsk) if bsk is not None else None, _u64(ksk) if ksk is not None else None))
    ck = ClientKey(params, seed, lwe, glwe)
    if not with_server_key:
        return ck, None
    zeros = None
    if params.order == 1:
        zeros = np.zeros((MS_FHEVM["count"], params.n + 1), dtype=np.uint64)
        _check(L.tfhe_hip_ms_zeros_keygen_k(ctypes.byref(params), ctypes.byref(rk), _u64(lwe), zeros.shape[0],
                                            _u64(zeros)))
    return ck, ServerKey(params, bsk, ksk, zeros)


def server_keygen(ck: "ClientKey", seed: Optional[int] = None, grouping: int = 1) -> ServerKey:
    """BSK / KSK (+ MS zeros) for the secret keys of ``ck`` (e.g. a tfhe-rs ClientKey ingested by
    tfhe_amd.keyio).  seed None (default): fresh 192-bit OS entropy, so the published evaluation keys
    reveal nothing reproducible; an int seed only for tests.  grouping 2, 3 or 4: a multi-bit key."""
    p = ck.params
    L = lib()
    if grouping != 1:
        return _mb_server_key(p, rng_key(seed), _c_u64(ck.lwe_key), _c_u64(ck.glwe_key), grouping)
    bsk = np.zeros(L.tfhe_hip_bsk_len(ctypes.byref(p)), dtype=np.uint64)
    ksk = np.zeros(L.tfhe_hip_ksk_len(ctypes.byref(p)), dtype=np.uint64)
    lwe, glwe = _c_u64(ck.lwe_key), _c_u64(ck.glwe_key)
    rk = rng_key(seed)
    _check(L.tfhe_hip_server_keygen_k(ctypes.byref(p), ctypes.byref(rk), _u64(lwe), _u64(glwe), _u64(bsk), _u64(ksk)))
    zeros = None
    if p.order == 1:
        zeros = np.zeros((MS_FHEVM["count"], p.n + 1), dtype=np.uint64)
        _check(L.tfhe_hip_ms_zeros_keygen_k(ctypes.byref(p), ctypes.byref(rk), _u64(lwe), zeros.shape[0], _u64(zeros)))
    return ServerKey(p, bsk, ksk, zeros)


def lut_constant(N: int, torus_value: int) -> np.ndarray:
    out = np.zeros(N, dtype=np.uint64)
    _check(lib().tfhe_hip_lut_constant(N, torus_value, _u64(out)))
    return out


def lut_from_table(N: int, msg_modulus: int, table: Sequence[int], delta_out: int) -> np.ndarray:
    t = _c_u64([int(v) % (1 << 64) for v in table])
    out = np.zeros(N, dtype=np.uint64)
    _check(lib().tfhe_hip_lut_from_table(N, msg_modulus, _u64(t), delta_out, _u64(out)))
    return out


def lut_many(N: int, msg_modulus: int, tables: Sequence[Sequence[int]], delta_out: int):
    """tfhe-rs ``generate_many_lookup_table``: n_fn tables of ``msg_modulus // n_fn`` entries side by side in
    one accumulator -> (lut, stride).  After one blind rotation of an input that uses only the first
    ``1/n_fn`` of the message space, function f is the sample at degree ``f * stride``
    (``Engine.pbs_many``).  The LUT is ``lut_from_table`` of the concatenated tables."""
    n_fn = len(tables)
    if n_fn < 1 or n_fn & (n_fn - 1) or msg_modulus % n_fn or N % n_fn:
        raise ValueError(f"lut_many: n_fn = {n_fn} must be a power of two dividing msg_modulus = {msg_modulus}")
    per = msg_modulus // n_fn
    for f, t in enumerate(tables):
        if len(t) != per:
            raise ValueError(f"lut_many: table {f} has {len(t)} entries, expected msg_modulus / n_fn = {per}")
    flat = [v for t in tables for v in t]
    return lut_from_table(N, msg_modulus, flat, delta_out), N // n_fn


def lut_oprf(N: int, random_bits: int, full_bits: int):
    """The staircase LUT and post-add of tfhe-rs ``generate_oblivious_pseudo_random*`` (include/tfhe_hip.h, PARITY
    UNPINNED): with p = 2^random_bits and delta = 2^(64 - full_bits), ``lut[x] = (2 (x // (2N/p)) + 1) delta/2`` and
    ``post_add = (p - 1) delta/2`` -> (lut, post_add)."""
    for v in (N, random_bits, full_bits):
        if not 0 <= int(v) < 1 << 32:
            raise ValueError("lut_oprf: arguments must fit 32 bits")
    lut = np.zeros(max(int(N), 1), dtype=np.uint64)
    post = ctypes.c_uint64()
    _check(lib().tfhe_hip_lut_oprf(int(N), int(random_bits), int(full_bits), _u64(lut), ctypes.byref(post)))
    return lut, int(post.value)


def oprf_block_seeds(seed, count: int) -> np.ndarray:
    """The row seeds of one rand request: block j uses (lo, hi) = words (2j, 2j + 1) of the stream of the parent
    ``seed`` = (lo, hi) (tfhe-rs DeterministicSeeder, PARITY UNPINNED) -> (count, 2) uint64."""
    s = _c_u64([int(seed[0]) % (1 << 64), int(seed[1]) % (1 << 64)])
    out = np.zeros((int(count), 2), dtype=np.uint64)
    _check(lib().tfhe_hip_csprng_words(_u64(s), 0, out.size, _u64(out)))
    return out


# ------------------------------------------------------------------------------------- engine
class Engine:
    """A device engine over one or more GPUs (``device``: an ordinal or a sequence of ordinals, one
    shard each; include/tfhe_hip.h).  Host-array batches split into per-device slices that run
    concurrently; keys are uploaded once and broadcast to every shard (RCCL for distinct ordinals).
    Mirrors the server-side operator surface of the path."""

    def __init__(self, params: Optional[Params] = None, device=0):
        self.params = params or Params.preset(PRESET_GATE)
        devs = [int(device)] if isinstance(device, (int, np.integer)) else [int(d) for d in device]
        arr = (ctypes.c_int * len(devs))(*devs)
        h = ctypes.c_void_p()
        _check(lib().tfhe_hip_create(ctypes.byref(self.params), arr, len(devs), ctypes.byref(h)))
        self._h = h
        self.devices = devs
        self.device = devs[0]

    CUS_PER_DEVICE = 256  # MI355X; the fallback when the device cannot be queried

    @property
    def cus_per_device(self) -> int:
        """Compute units of the engine's first device (hipDeviceProp_t::multiProcessorCount, 256 on MI355X)."""
        if getattr(self, "_cus", None) is None:
            try:
                import torch
                self._cus = int(torch.cuda.get_device_properties(self.device).multi_processor_count)
            except Exception:  # noqa: BLE001 - no torch device view: the MI355X figure
                self._cus = self.CUS_PER_DEVICE
        return self._cus

    @property
    def round_size(self) -> int:
        """PBS one round of this engine's batch kernel holds across its shards (one workgroup per CU): 4
        ciphertexts per workgroup on the FFT64 kernels (N = 1024 component pairs, N = 2048 parity pairs) and on
        the N = 2048 NTT kernel, 8 on the N = 1024 NTT kernel.  The carry-out circuit's launch-round cost model
        (integer.Circuit) reads it."""
        per_wg = 8 if (self.params.transform == 0 and self.params.N == 1024) else 4
        return per_wg * self.cus_per_device * len(self.devices)

    @property
    def grouping(self) -> int:
        """Grouping factor of the resident bootstrapping key: 1 = classic (or none), 2..4 = multi-bit."""
        return int(lib().tfhe_hip_grouping(self._h))

    @property
    def key_bcast_mode(self) -> str:
        return {0: "single", 1: "copy", 2: "rccl"}.get(lib().tfhe_hip_key_bcast_mode(self._h), "?")

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            lib().tfhe_hip_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- keys -------------------------------------------------------------------------------
    def load_keys(self, sk: ServerKey) -> "Engine":
        """Classic or multi-bit keys, by ``sk.grouping``."""
        if getattr(sk, "grouping", 1) != 1:
            bsk = _c_u64(sk.bsk)
            ksk = _c_u64(sk.ksk) if sk.ksk is not None else None
            _check(lib().tfhe_hip_load_keys_mb(self._h, int(sk.grouping), _u64(bsk), bsk.size,
                                               _u64(ksk) if ksk is not None else None, ksk.size if ksk is not None else 0))
            return self
        bsk, ksk = _c_u64(sk.bsk), _c_u64(sk.ksk)
        _check(lib().tfhe_hip_load_keys(self._h, _u64(bsk), bsk.size, _u64(ksk), ksk.size))
        if getattr(sk, "ms_zeros", None) is not None:
            self.load_ms_key(sk.ms_zeros)
        return self

    def load_bsk(self, bsk: np.ndarray) -> "Engine":
        """The bootstrapping key alone (a decompression key has no keyswitching key).  The engine is then
        rotation-only: ``blind_rotate``, ``bootstrap*`` and decompression work; ``pbs`` / ``keyswitch`` / ``nand``
        raise ENOKEYS until ``load_keys``."""
        b = _c_u64(bsk)
        _check(lib().tfhe_hip_load_bsk(self._h, _u64(b), b.size))
        return self

    def load_compressed_keys(self, csk) -> "Engine":
        """A whole ``keyio.CompressedServerKey`` through the seeded loaders: bodies and seeds go up, the masks are
        generated into the key layouts on the device (tfhe_amd/csrc/seeded_keys.hip) and the usual conversion follows.
        Multi-bit when ``csk.grouping > 1``; the modulus-switch zeros are loaded when the key carries them and is
        classic.  Same resident keys as ``keyio.decompress_server_key`` + ``load_keys``, word for word."""
        from . import keyio
        L = lib()
        g = int(getattr(csk, "grouping", 1))
        bb, kb = _c_u64(csk.bsk_bodies).ravel(), _c_u64(csk.ksk_bodies).ravel()
        bs, ks = keyio._seed2(csk.bsk_seed), keyio._seed2(csk.ksk_seed)
        if g != 1:
            if not 0 <= g < 1 << 32:
                raise ValueError(f"grouping = {g} must fit 32 bits")
            _check(L.tfhe_hip_load_keys_mb_seeded(self._h, g, _u64(bs), _u64(bb), bb.size, _u64(ks), _u64(kb), kb.size))
            return self
        _check(L.tfhe_hip_load_keys_seeded(self._h, _u64(bs), _u64(bb), bb.size, _u64(ks), _u64(kb), kb.size))
        if csk.ms_bodies is not None and csk.ms_seed is not None:
            mb = _c_u64(csk.ms_bodies).ravel()
            ms = {**{k: MS_FHEVM[k] for k in ("bound", "r_sigma", "input_variance")}, **(csk.ms or {})}
            _check(L.tfhe_hip_load_ms_key_seeded(self._h, _u64(keyio._seed2(csk.ms_seed)), _u64(mb), mb.size,
                                                 ms["bound"], ms["r_sigma"], ms["input_variance"]))
        return self

    def load_compressed_bsk(self, seed: int, bodies: np.ndarray) -> "Engine":
        """The rotation-only form of ``load_compressed_keys``: a seeded classic bootstrapping key alone (bodies
        [n][L][k+1][N]), e.g. a decompression key.  The engine is then rotation-only as after ``load_bsk``."""
        from . import keyio
        b = _c_u64(bodies).ravel()
        _check(lib().tfhe_hip_load_bsk_seeded(self._h, _u64(keyio._seed2(seed)), _u64(b), b.size))
        return self

    def seeded_load_stats(self) -> dict:
        """Device milliseconds of the last seeded key load on shard 0: upload, expansion kernels, conversion."""
        v = [ctypes.c_double() for _ in range(3)]
        _check(lib().tfhe_hip_seeded_load_stats(self._h, *[ctypes.byref(x) for x in v]))
        return {"upload_ms": v[0].value, "expand_ms": v[1].value, "convert_ms": v[2].value}

    def load_ms_key(self, zeros: Optional[np.ndarray], bound: float = MS_FHEVM["bound"],
                    r_sigma: float = MS_FHEVM["r_sigma"], input_variance: float = MS_FHEVM["input_variance"]):
        """Modulus-switch noise reduction between keyswitch and blind rotation (None: disable)."""
        if zeros is None:
            _check(lib().tfhe_hip_load_ms_key(self._h, None, 0, 0.0, 0.0, 0.0))
            return self
        z = _c_u64(zeros).reshape(-1, self.params.n + 1)
        _check(lib().tfhe_hip_load_ms_key(self._h, _u64(z), z.shape[0], bound, r_sigma, input_variance))
        return self

    def ms_reduce(self, small: np.ndarray):
        """Stage-level noise reduction on small-key ciphertexts -> (ciphertexts, chosen zero index or -1)."""
        x = _c_u64(small).reshape(-1, self.params.n + 1)
        out = np.zeros_like(x)
        picks = np.zeros(x.shape[0], dtype=np.int32)
        _check(lib().tfhe_hip_ms_reduce(self._h, _u64(x), x.shape[0], _u64(out),
                                        picks.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return out, picks

    def load_keys_device(self, d_bsk, d_ksk) -> "Engine":
        """Keys already in HBM on this device (torch tensors of dtype int64/uint64, e.g. after an
        RCCL broadcast)."""
        _check(lib().tfhe_hip_load_keys_device(self._h, _dptr(d_bsk), d_bsk.numel(), _dptr(d_ksk), d_ksk.numel()))
        return self

    # -- LUTs -------------------------------------------------------------------------------
    def generate_accumulator(self, f: Callable[[int], int], msg_modulus: int = 4,
                             delta_out: Optional[int] = None) -> np.ndarray:
        """tfhe-rs ServerKey::generate_accumulator (main.rs:65-68): LUT for m -> f(m)."""
        delta_out = delta_out if delta_out is not None else (1 << 63) // msg_modulus
        table = [f(m) % msg_modulus for m in range(msg_modulus)]
        return lut_from_table(self.params.N, msg_modulus, table, delta_out)

    def gate_lut(self) -> np.ndarray:
        return lut_constant(self.params.N, MU)

    # -- hot path ---------------------------------------------------------------------------
    def _pbs_host_args(self, cts, luts, lut_index, row_len):
        """Host arrays of pbs / pbs_many / bootstrap / blind_rotate -> (the (B, row_len) ciphertexts, the C arguments
        up to ``lut_index``)."""
        cts = _c_u64(cts).reshape(-1, row_len)
        luts = _c_u64(luts).reshape(-1, self.params.N)
        return cts, (self._h, _u64(cts), cts.shape[0], _u64(luts), luts.shape[0],
                     _lut_index(lut_index, cts.shape[0], "ciphertext"))

    def _pbs_async_args(self, d_in, d_luts, d_lut_index, d_out, stream):
        """Device tensors of pbs_async / pbs_many_async -> the C arguments (up to ``d_idx``, from ``d_out`` on)."""
        head = (self._h, _dptr(d_in), d_in.shape[0], _dptr(d_luts), d_luts.numel() // self.params.N, _dptr(d_lut_index))
        return head, (_dptr(d_out), ctypes.c_void_p(_stream_handle(stream, self.device)))

    def pbs(self, cts: np.ndarray, luts: np.ndarray, lut_index=None) -> np.ndarray:
        """Batched keyswitch_programmable_bootstrap over host arrays: (B, dim+1) -> (B, dim+1)."""
        cts, head = self._pbs_host_args(cts, luts, lut_index, self.params.io_dim + 1)
        out = np.zeros_like(cts)
        _check(lib().tfhe_hip_pbs(*head, _u64(out)))
        return out

    def keyswitch_programmable_bootstrap(self, ct: np.ndarray, acc: np.ndarray) -> np.ndarray:
        return self.pbs(ct, acc)

    def pbs_async(self, d_in, d_luts, d_out, d_lut_index=None, stream=None) -> None:
        """Device-resident batch (torch tensors on this device), enqueued on ``stream``
        (a torch.cuda.Stream or raw handle; default torch's current stream if torch is loaded).  The call writes
        exactly the B rows of ``d_out`` and nothing else, and reads nothing past row B of ``d_in``.  The kernels access
        ``d_in``, ``d_luts`` and ``d_out`` as 8-byte words: the natural alignment of the words is all they need."""
        head, tail = self._pbs_async_args(d_in, d_luts, d_lut_index, d_out, stream)
        _check(lib().tfhe_hip_pbs_async(*head, *tail))

    def pbs_device(self, d_in, d_luts, d_lut_index=None):
        """pbs_async into a fresh tensor: (B, dim+1) int64 on this device -> the same shape, queued on torch's
        current stream (no host synchronisation)."""
        d_out = d_in.new_empty(d_in.shape)
        if d_in.shape[0]:
            self.pbs_async(d_in.contiguous(), d_luts, d_out, d_lut_index)
        return d_out

    def bootstrap(self, cts: np.ndarray, luts: np.ndarray, lut_index=None) -> np.ndarray:
        """tfhe-rs ``programmable_bootstrap_lwe_ciphertext``, batched over host arrays: blind rotation and sample
        extraction with no keyswitch, (B, n+1) under the small key -> (B, kN+1) under the GLWE key.  Needs the
        bootstrapping key only (``load_bsk`` or ``load_keys``)."""
        p = self.params
        cts, head = self._pbs_host_args(cts, luts, lut_index, p.n + 1)
        out = np.zeros((cts.shape[0], p.k * p.N + 1), dtype=np.uint64)
        _check(lib().tfhe_hip_bootstrap(*head, _u64(out)))
        return out

    def bootstrap_async(self, d_in, d_luts, d_out, d_lut_index=None, stream=None) -> None:
        """Device-resident ``bootstrap`` (torch tensors on this device: d_in (B, n+1), d_out (B, kN+1)), enqueued
        on ``stream`` like ``pbs_async``.  The call writes exactly the B rows of ``d_out`` and nothing else, and reads
        nothing past row B of ``d_in``; 8-byte alignment of ``d_in``, ``d_luts`` and ``d_out`` is all the kernels need."""
        head, tail = self._pbs_async_args(d_in, d_luts, d_lut_index, d_out, stream)
        _check(lib().tfhe_hip_bootstrap_async(*head, *tail))

    def bootstrap_device(self, d_in, d_luts, d_lut_index=None):
        """bootstrap_async into a fresh tensor: (B, n+1) on this device -> (B, kN+1), queued on torch's current
        stream (no host synchronisation)."""
        d_out = d_in.new_empty((d_in.shape[0], self.params.k * self.params.N + 1))
        if d_in.shape[0]:
            self.bootstrap_async(d_in.contiguous(), d_luts, d_out, d_lut_index)
        return d_out

    def pbs_many(self, cts: np.ndarray, luts: np.ndarray, n_fn: int, stride: int, lut_index=None) -> np.ndarray:
        """tfhe-rs ``apply_many_lookup_table``, batched over host arrays: one blind rotation per input and
        ``n_fn`` outputs, function f extracted at degree ``f * stride`` (``lut_many`` builds the LUTs):
        (B, dim+1) -> (B, n_fn, dim+1)."""
        cts, head = self._pbs_host_args(cts, luts, lut_index, self.params.io_dim + 1)
        n_fn, stride = int(n_fn), int(stride)
        if not (0 <= n_fn < 1 << 32 and 0 <= stride < 1 << 32):
            raise ValueError("n_fn and stride must fit 32 bits")
        out = np.zeros((cts.shape[0], n_fn, cts.shape[1]), dtype=np.uint64)
        _check(lib().tfhe_hip_pbs_many(*head, n_fn, stride, _u64(out)))
        return out

    def pbs_many_async(self, d_in, d_luts, d_out, n_fn: int, stride: int, d_lut_index=None, stream=None) -> None:
        """Device-resident ``pbs_many`` (torch tensors on this device; d_out: (B, n_fn, dim+1)), enqueued on
        ``stream`` like ``pbs_async``.  The call writes exactly the B * n_fn rows of ``d_out`` and nothing else, and
        reads nothing past row B of ``d_in``; 8-byte alignment of ``d_in``, ``d_luts`` and ``d_out`` is all the kernels
        need (the 16-byte loads of the extraction read the engine's own accumulator workspace)."""
        head, tail = self._pbs_async_args(d_in, d_luts, d_lut_index, d_out, stream)
        _check(lib().tfhe_hip_pbs_many_async(*head, int(n_fn), int(stride), *tail))

    def pbs_many_device(self, d_in, d_luts, n_fn: int, stride: int, d_lut_index=None):
        """pbs_many_async into a fresh tensor: (B, dim+1) on this device -> (B, n_fn, dim+1), queued on torch's
        current stream (no host synchronisation)."""
        d_out = d_in.new_empty((d_in.shape[0], int(n_fn), d_in.shape[1]))
        if d_in.shape[0]:
            self.pbs_many_async(d_in.contiguous(), d_luts, d_out, n_fn, stride, d_lut_index)
        return d_out

    # -- compact ciphertext lists (tfhe_amd/ctlist.py builds the words) ----------------------------------
    @staticmethod
    def _rows(count: int, rep: int, rows) -> int:
        return int(count) * int(rep) if rows is None else int(rows)

    def expand_compact(self, words: np.ndarray, lwe_dim: int, count: int, rep: int = 1, rows=None) -> np.ndarray:
        """tfhe-rs ``CompactCiphertextList::expand`` on the device, over host arrays: the list's words (masks then
        bodies) -> (rows, lwe_dim + 1) LWEs, row r = list entry ``r // rep`` (``rows`` defaults to ``count * rep``).
        Needs no key."""
        w = _c_u64(words).reshape(-1)
        rows = self._rows(count, rep, rows)
        out = np.zeros((max(rows, 0), int(lwe_dim) + 1), dtype=np.uint64)
        _check(lib().tfhe_hip_expand_compact(self._h, _u64(w), w.size, int(lwe_dim), int(count), int(rep), rows,
                                             _u64(out)))
        return out

    def expand_compact_async(self, d_words, lwe_dim: int, count: int, d_out, rep: int = 1, rows=None,
                             stream=None) -> None:
        """Device-resident ``expand_compact`` (torch tensors on this device; d_out: (rows, lwe_dim + 1)), enqueued on
        ``stream`` like ``pbs_async``."""
        _check(lib().tfhe_hip_expand_compact_async(
            self._h, _dptr(d_words), d_words.numel(), int(lwe_dim), int(count), int(rep), self._rows(count, rep, rows),
            _dptr(d_out), ctypes.c_void_p(_stream_handle(stream, self.device))))

    def expand_compact_device(self, d_words, lwe_dim: int, count: int, rep: int = 1, rows=None):
        """expand_compact_async into a fresh (rows, lwe_dim + 1) tensor on torch's current stream (no host
        synchronisation)."""
        rows = self._rows(count, rep, rows)
        d_out = d_words.new_empty((max(rows, 0), int(lwe_dim) + 1))
        self.expand_compact_async(d_words.contiguous(), lwe_dim, count, d_out, rep, rows)
        return d_out

    def expand_cast(self, words: np.ndarray, count: int, luts: np.ndarray, rep: int = 1, rows=None,
                    lut_index=None) -> np.ndarray:
        """Expansion of a compact list of dimension ``io_dim`` followed by this engine's full PBS, in one call over
        host arrays: (rows, io_dim + 1).  With the casting key as the engine's keyswitch key this is the ingest of
        an fhEVM input (``ctlist.cast_list_to_blocks``)."""
        w = _c_u64(words).reshape(-1)
        luts = _c_u64(luts).reshape(-1, self.params.N)
        rows = self._rows(count, rep, rows)
        li = _lut_index(lut_index, rows, "output row")
        out = np.zeros((max(rows, 0), self.params.io_dim + 1), dtype=np.uint64)
        _check(lib().tfhe_hip_expand_cast(self._h, _u64(w), w.size, int(count), int(rep), rows, _u64(luts),
                                          luts.shape[0], li, _u64(out)))
        return out

    def expand_cast_async(self, d_words, count: int, d_luts, d_out, rep: int = 1, rows=None, d_lut_index=None,
                          stream=None) -> None:
        """Device-resident ``expand_cast`` (torch tensors on this device; d_out: (rows, io_dim + 1)), enqueued on
        ``stream`` like ``pbs_async``."""
        _check(lib().tfhe_hip_expand_cast_async(
            self._h, _dptr(d_words), d_words.numel(), int(count), int(rep), self._rows(count, rep, rows), _dptr(d_luts),
            d_luts.numel() // self.params.N, _dptr(d_lut_index), _dptr(d_out),
            ctypes.c_void_p(_stream_handle(stream, self.device))))

    def expand_cast_device(self, d_words, count: int, d_luts, rep: int = 1, rows=None, d_lut_index=None):
        """expand_cast_async into a fresh (rows, io_dim + 1) tensor on torch's current stream (no host
        synchronisation); the result is an input of ``pbs_device``."""
        rows = self._rows(count, rep, rows)
        d_out = d_words.new_empty((max(rows, 0), self.params.io_dim + 1))
        self.expand_cast_async(d_words.contiguous(), count, d_luts, d_out, rep, rows, d_lut_index)
        return d_out

    # -- oblivious pseudo-random ciphertexts (fhEVM rand / randBounded; radix.py and integer.py build on these) ----
    def csprng_rows(self, seeds: np.ndarray, dim: int, first_word: int = 0) -> np.ndarray:
        """Stage-level: the device's seeded mask stream over host arrays, (rows, 2) seeds -> (rows, dim), row r =
        words ``first_word .. first_word + dim - 1`` of seed r's stream (``tfhe_hip_csprng_words``).  Needs no key."""
        s = _c_u64(seeds).reshape(-1, 2)
        if not (0 <= int(dim) < 1 << 32 and 0 <= int(first_word) < 1 << 64):
            raise ValueError("csprng_rows: dim must fit 32 bits and first_word 64")
        out = np.zeros((s.shape[0], int(dim)), dtype=np.uint64)
        _check(lib().tfhe_hip_csprng_rows(self._h, _u64(s), s.shape[0], int(first_word), int(dim), _u64(out)))
        return out

    def csprng_rows_async(self, d_seeds, dim: int, d_out, first_word: int = 0, stream=None) -> None:
        """Device-resident ``csprng_rows`` (torch tensors on this device: d_seeds (rows, 2), d_out (rows, stride) with
        stride >= dim; words past ``dim`` of a row are left alone), enqueued on ``stream`` like ``pbs_async``."""
        _check(lib().tfhe_hip_csprng_rows_async(
            self._h, _dptr(d_seeds), d_seeds.shape[0], int(first_word), int(dim), d_out.shape[1], _dptr(d_out),
            ctypes.c_void_p(_stream_handle(stream, self.device))))

    def _oprf_tables(self, luts, post_adds):
        luts = _c_u64(luts).reshape(-1, self.params.N)
        post = _c_u64([int(v) % (1 << 64) for v in np.atleast_1d(post_adds)])
        if post.shape[0] != luts.shape[0]:
            raise ValueError("oprf: one post_add per LUT")
        return luts, post

    def oprf(self, seeds: np.ndarray, luts: np.ndarray, post_adds, lut_index=None) -> np.ndarray:
        """tfhe-rs ``generate_oblivious_pseudo_random*``, batched over host arrays: (rows, 2) row seeds -> (rows,
        io_dim + 1) encryptions of pseudo-random values that nobody without the secret key knows.  Row r's mask comes
        from its seed on the device, is rotated through ``luts[lut_index[r]]`` (``lut_oprf``, or the gate LUT with
        post-add 0) and gets ``post_adds[lut_index[r]]`` added.  KS -> PBS parameter sets need the bootstrapping key
        only."""
        s = _c_u64(seeds).reshape(-1, 2)
        luts, post = self._oprf_tables(luts, post_adds)
        li = _lut_index(lut_index, s.shape[0], "seed")
        out = np.zeros((s.shape[0], self.params.io_dim + 1), dtype=np.uint64)
        _check(lib().tfhe_hip_oprf(self._h, _u64(s), s.shape[0], _u64(luts), _u64(post), luts.shape[0], li, _u64(out)))
        return out

    def oprf_async(self, d_seeds, d_luts, d_post_adds, d_out, d_lut_index=None, stream=None) -> None:
        """Device-resident ``oprf`` (torch tensors on this device: d_seeds (rows, 2), d_post_adds one word per LUT,
        d_out (rows, io_dim + 1)), enqueued on ``stream`` like ``pbs_async``."""
        _check(lib().tfhe_hip_oprf_async(
            self._h, _dptr(d_seeds), d_seeds.shape[0], _dptr(d_luts), _dptr(d_post_adds), d_luts.numel() // self.params.N,
            _dptr(d_lut_index), _dptr(d_out), ctypes.c_void_p(_stream_handle(stream, self.device))))

    def oprf_device(self, d_seeds, d_luts, d_post_adds, d_lut_index=None):
        """oprf_async into a fresh tensor: (rows, 2) seeds on this device -> (rows, io_dim + 1), queued on torch's
        current stream (no host synchronisation)."""
        d_out = d_seeds.new_empty((d_seeds.shape[0], self.params.io_dim + 1))
        if d_seeds.shape[0]:
            self.oprf_async(d_seeds.contiguous(), d_luts, d_post_adds, d_out, d_lut_index)
        return d_out

    # -- sparse linear combinations of rows: the linear part of a radix level (radix.LinBlocks builds the terms) ----
    @staticmethod
    def _lincomb_terms(row_start, term_buf, term_row, term_coef, bias):
        """The host term description -> (arrays to keep alive, the C arguments row_start .. rows).  Only what the C
        checks cannot see is checked here: that the arrays are as long as ``row_start`` says."""
        rs = np.ascontiguousarray(np.asarray(row_start, dtype=np.uint32)).reshape(-1)
        tb = np.ascontiguousarray(np.asarray(term_buf, dtype=np.uint32)).reshape(-1)
        tr = np.ascontiguousarray(np.asarray(term_row, dtype=np.uint32)).reshape(-1)
        tc = _c_u64(term_coef).reshape(-1)
        bs = None if bias is None else _c_u64(bias).reshape(-1)
        rows = max(rs.shape[0] - 1, 0)
        need = int(rs.max(initial=0))
        if min(tb.shape[0], tr.shape[0], tc.shape[0]) < need:
            raise ValueError("lincomb: row_start names more terms than the term arrays hold")
        if bs is not None and bs.shape[0] != rows:
            raise ValueError("lincomb: one bias per output row")
        args = (rs.ctypes.data_as(_U32P), tb.ctypes.data_as(_U32P), tr.ctypes.data_as(_U32P), _u64(tc),
                _u64(bs) if bs is not None else None, rows)
        return (rs, tb, tr, tc, bs), args

    @staticmethod
    def _lincomb_bufs(d_bufs, dim: int):
        """Device tensors -> (tensors to keep alive, the C arguments d_bufs, buf_rows, n_buf)."""
        keep = [b if b.is_contiguous() else b.contiguous() for b in d_bufs]
        ptrs = (ctypes.c_void_p * max(len(keep), 1))(*[b.data_ptr() for b in keep])
        nrow = (ctypes.c_size_t * max(len(keep), 1))(*[b.numel() // dim for b in keep])
        return keep, (ptrs, nrow, len(keep))

    def lincomb(self, bufs, row_start, term_buf, term_row, term_coef, bias=None, dim: Optional[int] = None) -> np.ndarray:
        """Sparse linear combinations of LWE rows over host arrays, mod 2^64 (``radix.lincomb_ref`` states the map):
        output row r = the sum over its terms t of ``term_coef[t]`` times row ``term_row[t]`` of ``bufs[term_buf[t]]``,
        plus ``bias[r]`` on the body; a row without terms is trivial.  ``bufs``: arrays of (rows_b, dim) words.  The
        C host form takes one source buffer, so the buffers are joined here.  Needs no key."""
        bufs = [_c_u64(b) for b in bufs]
        dim = int(dim if dim is not None else (bufs[0].shape[-1] if bufs else self.params.io_dim + 1))
        bufs = [b.reshape(-1, dim) for b in bufs]
        base = np.concatenate([[0], np.cumsum([b.shape[0] for b in bufs])]).astype(np.int64)
        src = np.concatenate(bufs, axis=0) if bufs else np.zeros((0, dim), dtype=np.uint64)
        tb = np.asarray(term_buf, dtype=np.int64).reshape(-1)
        tr = np.asarray(term_row, dtype=np.int64).reshape(-1)
        if tb.size and (tb.min() < 0 or tb.max() >= len(bufs) or np.any(tr >= base[tb + 1] - base[tb])):
            raise ValueError("lincomb: a term names a buffer or a row that does not exist")
        keep, (rs, _, trp, tc, bs, rows) = self._lincomb_terms(row_start, np.zeros_like(tb), tr + base[tb], term_coef, bias)
        out = np.zeros((rows, dim), dtype=np.uint64)
        _check(lib().tfhe_hip_lwe_lincomb(self._h, dim, _u64(src), src.shape[0], rs, trp, tc, bs, rows, _u64(out)))
        del keep
        return out

    def lincomb_async(self, d_bufs, row_start, term_buf, term_row, term_coef, bias, d_out, stream=None) -> None:
        """Device-resident ``lincomb`` (``d_bufs``: torch tensors of (rows_b, dim) words on this device, d_out: (rows,
        dim), overlapping none of them), enqueued on ``stream`` like ``pbs_async``.  The term arrays stay host
        arrays: the library checks them and resolves the addresses itself."""
        dim = int(d_out.shape[-1])
        keep_b, bufs = self._lincomb_bufs(d_bufs, dim)
        keep_t, terms = self._lincomb_terms(row_start, term_buf, term_row, term_coef, bias)
        _check(lib().tfhe_hip_lwe_lincomb_async(self._h, dim, *bufs, *terms, _dptr(d_out),
                                                ctypes.c_void_p(_stream_handle(stream, self.device))))
        del keep_b, keep_t

    def _lincomb_out(self, d_bufs, rows: int, dim: int):
        if d_bufs:
            return d_bufs[0].new_empty((rows, dim))
        import torch
        return torch.empty((rows, dim), dtype=torch.int64, device=f"cuda:{self.device}")

    def lincomb_device(self, d_bufs, row_start, term_buf, term_row, term_coef, bias=None, dim: Optional[int] = None):
        """lincomb_async into a fresh (rows, dim) tensor on torch's current stream (no host synchronisation); ``dim``
        defaults to the row length of the first buffer, or io_dim + 1 without buffers."""
        dim = int(dim if dim is not None else (d_bufs[0].shape[-1] if d_bufs else self.params.io_dim + 1))
        rows = max(len(row_start) - 1, 0)
        d_out = self._lincomb_out(d_bufs, rows, dim)
        if rows:
            self.lincomb_async(d_bufs, row_start, term_buf, term_row, term_coef, bias, d_out)
        return d_out

    def lincomb_pbs_device(self, d_bufs, row_start, term_buf, term_row, term_coef, bias, d_luts, d_lut_index=None):
        """``lincomb_device`` at dim = io_dim + 1 into a workspace of the engine, then ``pbs_device`` of the assembled
        rows, in one call: a fresh (rows, io_dim + 1) tensor, queued on torch's current stream."""
        dim = self.params.io_dim + 1
        rows = max(len(row_start) - 1, 0)
        d_out = self._lincomb_out(d_bufs, rows, dim)
        if rows:
            keep_b, bufs = self._lincomb_bufs(d_bufs, dim)
            keep_t, terms = self._lincomb_terms(row_start, term_buf, term_row, term_coef, bias)
            _check(lib().tfhe_hip_lincomb_pbs_async(
                self._h, *bufs, *terms, _dptr(d_luts), d_luts.numel() // self.params.N, _dptr(d_lut_index), _dptr(d_out),
                ctypes.c_void_p(_stream_handle(None, self.device))))
            del keep_b, keep_t
        return d_out

    def sample_extract_many(self, acc: np.ndarray, n_fn: int, stride: int) -> np.ndarray:
        """Samples of each accumulator at degrees ``f * stride``, f < n_fn: (B, (k+1)N) -> (B, n_fn, kN+1)."""
        p = self.params
        acc = _c_u64(acc).reshape(-1, (p.k + 1) * p.N)
        out = np.zeros((acc.shape[0], max(int(n_fn), 0), p.k * p.N + 1), dtype=np.uint64)
        _check(lib().tfhe_hip_sample_extract_many(self._h, _u64(acc), acc.shape[0], int(n_fn), int(stride), _u64(out)))
        return out

    def blind_rotate(self, cts: np.ndarray, luts: np.ndarray, lut_index=None) -> np.ndarray:
        p = self.params
        cts, head = self._pbs_host_args(cts, luts, lut_index, p.n + 1)
        out = np.zeros((cts.shape[0], (p.k + 1) * p.N), dtype=np.uint64)
        _check(lib().tfhe_hip_blind_rotate(*head, _u64(out)))
        return out

    def sample_extract(self, acc: np.ndarray) -> np.ndarray:
        p = self.params
        acc = _c_u64(acc).reshape(-1, (p.k + 1) * p.N)
        out = np.zeros((acc.shape[0], p.k * p.N + 1), dtype=np.uint64)
        _check(lib().tfhe_hip_sample_extract(self._h, _u64(acc), acc.shape[0], _u64(out)))
        return out

    def keyswitch(self, big: np.ndarray) -> np.ndarray:
        p = self.params
        big = _c_u64(big).reshape(-1, p.k * p.N + 1)
        out = np.zeros((big.shape[0], p.n + 1), dtype=np.uint64)
        _check(lib().tfhe_hip_keyswitch(self._h, _u64(big), big.shape[0], _u64(out)))
        return out

    def ntt_fwd(self, polys: np.ndarray) -> np.ndarray:
        x = _c_u64(polys).copy()
        _check(lib().tfhe_hip_ntt_fwd(self._h, _u64(x), x.size // self.params.N))
        return x

    def ntt_inv(self, polys: np.ndarray) -> np.ndarray:
        x = _c_u64(polys).copy()
        _check(lib().tfhe_hip_ntt_inv(self._h, _u64(x), x.size // self.params.N))
        return x

    def fft_fwd(self, polys: np.ndarray) -> np.ndarray:
        """FFT64 ctx: N torus values (read as int64) per polynomial -> N/2 complex128, natural order."""
        x = _c_u64(polys).reshape(-1, self.params.N)
        out = np.zeros((x.shape[0], self.params.N // 2), dtype=np.complex128)
        _check(lib().tfhe_hip_fft_fwd(self._h, _u64(x), x.shape[0], ctypes.c_void_p(out.ctypes.data)))
        return out

    def fft_inv(self, spec: np.ndarray) -> np.ndarray:
        """FFT64 ctx: N/2 complex -> N doubles (no 1/M, no rounding)."""
        z = np.ascontiguousarray(spec, dtype=np.complex128).reshape(-1, self.params.N // 2)
        out = np.zeros((z.shape[0], self.params.N), dtype=np.float64)
        _check(lib().tfhe_hip_fft_inv(self._h, ctypes.c_void_p(z.ctypes.data), z.shape[0],
                                      ctypes.c_void_p(out.ctypes.data)))
        return out

    def nand(self, c1: np.ndarray, c2: np.ndarray) -> np.ndarray:
        dim = self.params.n + 1
        c1, c2 = _c_u64(c1).reshape(-1, dim), _c_u64(c2).reshape(-1, dim)
        out = np.zeros_like(c1)
        _check(lib().tfhe_hip_nand(self._h, _u64(c1), _u64(c2), c1.shape[0], _u64(out)))
        return out

    def sync(self) -> None:
        _check(lib().tfhe_hip_sync(self._h))

    def set_latency_batch(self, max_batch: int) -> None:
        """Batches up to ``max_batch`` use the latency blind-rotate kernel (0: always the batch kernel)."""
        _check(lib().tfhe_hip_set_latency_batch(self._h, ctypes.c_size_t(max_batch)))

    def br_kernel(self, batch: int) -> str:
        """Name of the blind-rotate kernel the dispatch launches for a per-shard batch of ``batch``."""
        return lib().tfhe_hip_br_kernel(self._h, ctypes.c_size_t(batch)).decode()

    # -- timing (HIP events around each kernel launch) -----------------------------------------
    def timing(self, enable: bool = True) -> None:
        _check(lib().tfhe_hip_timing_enable(self._h, 1 if enable else 0))

    def timing_reset(self) -> None:
        _check(lib().tfhe_hip_timing_reset(self._h))

    def timing_stats(self, which: int = 0):
        ms, cnt = ctypes.c_double(), ctypes.c_int()
        _check(lib().tfhe_hip_timing_stats(self._h, which, ctypes.byref(ms), ctypes.byref(cnt)))
        return ms.value, cnt.value


# ------------------------------------------------------------------------------ FheBool / FheUint8
def _gate_lin(c1: np.ndarray, c2: Optional[np.ndarray], k1: int, k2: int, const: int) -> np.ndarray:
    """(0, const) + k1*c1 + k2*c2 over Z_2^64 (TFHE-lib gate linear parts)."""
    with np.errstate(over="ignore"):
        out = c1 * np.uint64(k1 % (1 << 64))
        if c2 is not None:
            out = out + c2 * np.uint64(k2 % (1 << 64))
        out[..., -1] = out[..., -1] + np.uint64(const % (1 << 64))
    return out


class FheBool:
    """Encrypted booleans (a batch), gate-bootstrapped on the GPU.  NOT is free (negation)."""

    def __init__(self, engine: Engine, ct: np.ndarray):
        self.engine, self.ct = engine, _c_u64(ct).reshape(-1, engine.params.n + 1)

    @classmethod
    def encrypt(cls, values, ck: ClientKey, engine: Engine, seed: Optional[int] = None, stream0: int = 0) -> "FheBool":
        return cls(engine, ck.encrypt_bool(np.atleast_1d(values), seed, stream0))

    def decrypt(self, ck: ClientKey) -> np.ndarray:
        return ck.decrypt_bool(self.ct)

    def _boot(self, lin: np.ndarray) -> "FheBool":
        return FheBool(self.engine, self.engine.pbs(lin, self.engine.gate_lut()))

    def nand(self, other: "FheBool") -> "FheBool":
        return FheBool(self.engine, self.engine.nand(self.ct, other.ct))

    def __and__(self, other: "FheBool") -> "FheBool":
        return self._boot(_gate_lin(self.ct, other.ct, 1, 1, -MU))

    def __or__(self, other: "FheBool") -> "FheBool":
        return self._boot(_gate_lin(self.ct, other.ct, 1, 1, MU))

    def __xor__(self, other: "FheBool") -> "FheBool":
        return self._boot(_gate_lin(self.ct, other.ct, 2, 2, 2 * MU))

    def __invert__(self) -> "FheBool":
        with np.errstate(over="ignore"):
            return FheBool(self.engine, (np.uint64(0) - self.ct).astype(np.uint64))


class FheUint8:
    """Encrypted 8-bit unsigned integers as 8 gate-encoded bits (LSB first): shape (B, 8, n+1)."""

    def __init__(self, engine: Engine, bits: np.ndarray):
        self.engine = engine
        self.bits = _c_u64(bits).reshape(-1, 8, engine.params.n + 1)

    @classmethod
    def encrypt(cls, values, ck: ClientKey, engine: Engine, seed: Optional[int] = None, stream0: int = 0) -> "FheUint8":
        v = np.atleast_1d(np.asarray(values, dtype=np.uint64))
        bits = ((v[:, None] >> np.arange(8, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
        return cls(engine, ck.encrypt_bool(bits.reshape(-1), seed, stream0))

    def decrypt(self, ck: ClientKey) -> np.ndarray:
        b = ck.decrypt_bool(self.bits.reshape(-1, self.engine.params.n + 1)).reshape(-1, 8).astype(np.uint64)
        return (b << np.arange(8, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64)

    def map_bits(self, luts: np.ndarray) -> "FheUint8":
        """Bootstrap every bit with its own LUT (luts: 8 x N; bit j uses LUT j): 8 PBS per value."""
        B = self.bits.shape[0]
        idx = np.tile(np.arange(8, dtype=np.uint32), B)
        out = self.engine.pbs(self.bits.reshape(B * 8, -1), luts, idx)
        return FheUint8(self.engine, out)

    def refresh(self) -> "FheUint8":
        """Identity bootstrap of every bit (noise refresh)."""
        return self.map_bits(np.tile(self.engine.gate_lut(), (8, 1)))
