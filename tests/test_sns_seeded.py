"""Seeded noise-squashing and ct128 packing keys on the CPU (include/tfhe_hip.h the seeded squashing key / the seeded
ct128 packing key, tfhe_amd/csrc/seeded.cpp, tfhe_amd/keyio.py; DESIGN §7h'').

Pins: the 128-bit mask stream against its definition (bytes 16 w + 1 .. 16 w + 16 of the AES-CTR table, and words 2 w,
2 w + 1 of the 64-bit stream); every row of a host-decompressed squashing key, in the engine's [c L + l] order, decrypts
under the GLWE key to the GGSW plaintext and carries the stream words of its row; the decompressed key squashes on the
CPU oracle; the decompressed packing key packs at level 3 and a key whose storage order is left unreversed does not;
the container round-trips with and without the new parts and rejects truncation and wrong body counts.  The byte
layout of the real tfhe-rs structures is PARITY UNPINNED, as for every seeded path."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import sns_inputs as I
import sns_pks_ref as R
import sns_seeded_cases as C
import tfhe_amd
from tfhe_amd import keyio
from tfhe_amd import sns as S
from tfhe_amd import sns_compression as SC
from conftest import ROOT
from test_decompress import with_n

U128 = (1 << 128) - 1
EINVAL = -1                     # TFHE_HIP_EINVAL


def _aes(key: bytes, block: int) -> bytes:
    out = ctypes.create_string_buffer(16)
    tfhe_amd._check(tfhe_amd.lib().tfhe_hip_aes128_block(key, block.to_bytes(16, "little"), out))
    return out.raw


def _words64(seed: int, first: int, count: int) -> np.ndarray:
    out = np.zeros(count, dtype=np.uint64)
    tfhe_amd._check(tfhe_amd.lib().tfhe_hip_csprng_words(tfhe_amd._u64(keyio._seed2(seed)), first, count,
                                                          tfhe_amd._u64(out)))
    return out


@pytest.mark.parametrize("first", [0, 5, (1 << 33) + 3])
def test_stream128_definition(first):
    """u128 word w = table bytes 16 w + 1 .. 16 w + 16, little endian = words (2 w, 2 w + 1) of the 64-bit stream"""
    seed, count = C.MASK_SEED, 37
    key = seed.to_bytes(16, "little")
    table = b"".join(_aes(key, b) for b in range(first, first + count + 1))
    got = S.stream_words128(seed, first, count)
    for w in range(count):
        want = int.from_bytes(table[16 * w + 1:16 * w + 17], "little")
        assert int(got[w, 0]) | (int(got[w, 1]) << 64) == want, w
    assert np.array_equal(got.reshape(-1), _words64(seed, 2 * first, 2 * count))
    assert not np.array_equal(got, S.stream_words128(C.MASK_SEED_TOP, first, count))


def _signed(x: int) -> int:
    x &= U128
    return x - (1 << 128) if x >> 127 else x


def test_squashing_rows_decrypt_and_carry_their_stream_words():
    """n = 3, every one of the 27 rows.  Noise bound: the bodies carry round(N(0,1) 2^(64 + noise_log2)), 27 x 2048
    samples; 8 sigma = 2^(67 + noise_log2) is beyond them and 2^23 below the smallest plaintext g_2 = 2^56."""
    sp, key, ckey, dk = C.squash_keys(3)
    n, k, N, L = sp.n, sp.k, sp.N, sp.level
    assert ckey.bodies.shape == (n, L, k + 1, N, 2) and ckey.bodies.size == n * L * (k + 1) * 2 * N
    bound = 2 ** (67 + sp.noise_log2)
    assert bound < 2 ** (128 - sp.base_log * L - 20)
    bsk = dk.bsk.reshape(n, (k + 1) * L, k + 1, 2, N)              # the engine's [i][c L + l][j][lo, hi][N]
    Sk = key.glwe_key.reshape(k, N)
    assert set(int(v) for v in key.lwe_key) == {0, 1}
    for i in range(n):
        for c in range(k + 1):
            for l in range(L):
                row = bsk[i, c * L + l]
                rho = (i * L + l) * (k + 1) + c
                for j in range(k):                                      # masks: the stream words of row rho
                    w = S.stream_words128(ckey.seed, (rho * k + j) * N, N)
                    assert np.array_equal(row[j, 0], w[:, 0]) and np.array_equal(row[j, 1], w[:, 1]), (i, c, l, j)
                assert np.array_equal(row[k].transpose(1, 0), ckey.bodies[i, l, c])   # the stored body, de-interleaved
                ph = SC.glwe_phase128(k, N, key.glwe_key, row)
                g = 1 << (128 - sp.base_log * (l + 1))
                want = [0] * N
                if key.lwe_key[i]:
                    if c < k:
                        want = [-g * int(b) for b in Sk[c]]
                    else:
                        want[0] = g
                err = max(abs(_signed(p - w)) for p, w in zip(ph, want))
                assert err < bound, (i, c, l, err)
                if key.lwe_key[i]:                                      # and the plaintext is not noise
                    assert max(abs(_signed(p)) for p in ph) >= g - bound


def test_decompressed_key_squashes_on_the_oracle(oracle_mod):
    """n = 2: the oracle's blind rotation with the decompressed key words decrypts every message"""
    sp, key, ckey, dk = C.squash_keys(2)
    _, osp = I.small_params(oracle_mod, 2)
    okeys = oracle_mod.SnsKeys(osp, C.RNG_SEED, key.lwe_key, with_bsk=True)
    assert np.array_equal(okeys.glwe_key, key.glwe_key)
    okeys.bsk = np.array(dk.bsk)
    okeys._bsk_limb = None
    msgs = np.array([0, 1, 7, 8, 15], dtype=np.uint64)
    out = oracle_mod.sns_squash(osp, okeys, C.small_inputs(2, msgs), 16)
    assert np.array_equal(key.decrypt(out), msgs)


def _pack_and_decrypt(pp, key, pksk, msgs):
    lwes = R.encrypt(pp, key.in_key, msgs)
    glwes = SC.pack_host(pp, pksk, lwes)
    return SC.decrypt_list(key, SC._compress_groups(pp, glwes, len(msgs)))


def test_packing_key_level_reversal():
    """level 3: storage row s is decomposition level 3 - s and must land in engine row 2 - s.  The decompressed key
    packs and decrypts; the same rows left in storage order do not, so the check sees the order."""
    pp, key, ckey, dk = C.packing_keys(16, 1, 64, 3)
    assert (pp.level, pp.base_log) == (3, 40)
    assert ckey.bodies.shape == (16, 3, 64, 2)
    msgs = np.arange(pp.lwe_per_glwe + 3, dtype=np.uint64) % 16
    assert np.array_equal(_pack_and_decrypt(pp, key, dk.pksk, msgs), msgs)
    rows = dk.pksk.reshape(pp.in_dim, pp.level, pp.out_k + 1, 2, pp.out_N)
    for j in range(pp.in_dim):                                          # row l holds storage row level - 1 - l
        for l in range(pp.level):
            assert np.array_equal(rows[j, l, pp.out_k].transpose(1, 0), ckey.bodies[j, pp.level - 1 - l])
            w = S.stream_words128(ckey.seed, (j * pp.level + pp.level - 1 - l) * pp.out_k * pp.out_N, pp.out_N)
            assert np.array_equal(rows[j, l, 0, 0], w[:, 0]) and np.array_equal(rows[j, l, 0, 1], w[:, 1])
    unreversed = np.ascontiguousarray(rows[:, ::-1]).reshape(-1)
    assert not np.array_equal(_pack_and_decrypt(pp, key, unreversed, msgs), msgs)


# ---- the container -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def containers():
    """(csk with both parts, squashing only, neither) over one client key at n = 3, and the multi-bit twin at n = 4"""
    ck, _ = tfhe_amd.gen_keys(with_n(tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_FFT), 3), 0x5EED0C01,
                              with_server_key=False)
    sq = S.SquashedKey(C.squash_params(3), C.RNG_SEED, ck.lwe_key, with_bsk=False)
    comp = SC.SquashedCompressionKey(C.packing_params(4096, 1, 32, 1), C.RNG_SEED, sq.glwe_key, with_key=False)
    both = keyio.compress_server_key(ck, seed=0x5EED0C02, squashing=sq, squashed_compression=comp)
    only = keyio.compress_server_key(ck, seed=0x5EED0C02, squashing=sq)
    none = keyio.compress_server_key(ck, seed=0x5EED0C02)
    ck_mb, _ = tfhe_amd.gen_keys(with_n(tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_MB_FFT), 4), 0x5EED0C03,
                                 with_server_key=False)
    sq_mb = S.SquashedKey(C.squash_params(4), C.RNG_SEED, ck_mb.lwe_key, with_bsk=False)
    mb_with = keyio.compress_server_key(ck_mb, seed=0x5EED0C04, grouping=2, squashing=sq_mb)
    mb_none = keyio.compress_server_key(ck_mb, seed=0x5EED0C04, grouping=2)
    return both, only, none, mb_with, mb_none


# container bytes behind the shortint key's bootstrapping part when no new part is present (tests/test_seeded_mb.py
# TAIL): moduli 32, ciphertext modulus 24, order 4, four Option bytes, Tag 4 + 8
TAIL = 32 + 24 + 4 + 4 + 4 + 8


def _same_128(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.seed == b.seed and np.array_equal(a.bodies, b.bodies) and bytes(a.params) == bytes(b.params)


def test_container_roundtrip_and_prefix(containers):
    both, only, none, mb_with, mb_none = containers
    blobs = [keyio.dumps_compressed_server_key(c) for c in (both, only, none)]
    prefix = len(blobs[2]) - 13                               # through the three Options in front of the squashing key
    assert blobs[0][:prefix] == blobs[1][:prefix] == blobs[2][:prefix]
    assert blobs[2][prefix:] == b"\x00" + bytes(12) and blobs[1][prefix] == 1 and blobs[0][prefix] == 1
    assert blobs[0][-12:] == blobs[1][-12:] == bytes(12)         # the Tag follows the new part
    for csk, blob in zip((both, only, none), blobs):
        back = keyio.loads_compressed_server_key(blob)
        assert back.params == csk.params and (back.bsk_seed, back.ksk_seed) == (csk.bsk_seed, csk.ksk_seed)
        assert np.array_equal(back.bsk_bodies, csk.bsk_bodies) and np.array_equal(back.ksk_bodies, csk.ksk_bodies)
        assert _same_128(back.squashing, csk.squashing)
        assert _same_128(back.squashed_compression, csk.squashed_compression)
        assert keyio.dumps_compressed_server_key(back) == blob
    assert both.squashing is not None and both.squashed_compression is not None
    assert only.squashing is not None and only.squashed_compression is None and none.squashing is None
    # the bodies are 1 / (k + 1) of the standard-domain keys
    assert both.squashing.bodies.size * 3 == S._lib().tfhe_hip_sns_bsk_len(ctypes.byref(both.squashing.params))
    assert both.squashed_compression.bodies.size * 2 == \
        SC._lib().tfhe_hip_sns_pksk_len(ctypes.byref(both.squashed_compression.params))


def test_container_without_the_parts_keeps_its_bytes(containers):
    """classic and multi-bit: no new part -> the earlier layout, Option<noise-squashing key> = None, to the byte"""
    both, only, none, mb_with, mb_none = containers
    for csk, g in ((none, 1), (mb_none, 2)):
        blob = keyio.dumps_compressed_server_key(csk)
        head = 8 + 3 + 4 + 8 + 3 + 8 + len(keyio.COMPRESSED_SERVER_KEY_TYPE) + 16
        ksk_end = head + 8 + 8 * csk.ksk_bodies.size + 24 + 4 + 16 + 24
        bsk_end = ksk_end + 12 + 8 + 8 * csk.bsk_bodies.size + 32 + 4 + 16 + 24
        after = bsk_end + (1 if g == 1 else 8)                  # Option<MS key> = None / the grouping factor
        assert len(blob) == after + TAIL
        assert blob[after + 32 + 24 + 4:] == bytes(4) + bytes(12)
        back = keyio.loads_compressed_server_key(blob)
        assert back.squashing is None and back.squashed_compression is None and back.grouping == g
    blob = keyio.dumps_compressed_server_key(mb_with)
    back = keyio.loads_compressed_server_key(blob)
    assert back.grouping == 2 and _same_128(back.squashing, mb_with.squashing)
    plain = keyio.dumps_compressed_server_key(mb_none)
    assert blob[:len(plain) - 13] == plain[:-13] and blob[len(plain) - 13] == 1


def test_container_rejects_truncation_and_wrong_counts(containers):
    both, only, none, *_ = containers
    blob = keyio.dumps_compressed_server_key(both)
    start = len(keyio.dumps_compressed_server_key(none)) - 13   # the Option byte of the noise-squashing key
    end = len(blob) - 12                                         # the Tag behind the new part
    assert blob[start] == 1
    sq_bytes = 16 * both.squashing.bodies.size // 2
    comp_at = start + 1 + 8 + 8 + sq_bytes + 40 + 4 + 16 + 24    # the nested Option byte
    assert blob[comp_at] == 1
    cuts = {start, start + 1, start + 5, start + 9, start + 17, start + 17 + sq_bytes // 2, comp_at - 30, comp_at - 1,
            comp_at, comp_at + 1, comp_at + 5, comp_at + 13, (comp_at + end) // 2, end - 45, end - 21, end - 1}
    cuts |= set(int(c) for c in np.random.default_rng(9).integers(start, end, 24))
    for cut in sorted(cuts):
        with pytest.raises(keyio.KeyFormatError):
            keyio.loads_compressed_server_key(blob[:cut])
    keyio.loads_compressed_server_key(blob[:end])                # the whole new part: accepted
    # a body count that does not match the parameters: the level count of either key, the squashing key's Vec length
    lvl_sq = start + 1 + 8 + 8 + sq_bytes + 24
    lvl_comp = end - 24 - 20 - 24 - 8
    assert struct.unpack_from("<Q", blob, lvl_sq)[0] == 3 and struct.unpack_from("<Q", blob, lvl_comp)[0] == 1
    for at, wrong in ((lvl_sq, 2), (lvl_comp, 2), (lvl_sq - 24, 2)):
        bad = bytearray(blob)
        struct.pack_into("<Q", bad, at, wrong)
        with pytest.raises(keyio.KeyFormatError):
            keyio.loads_compressed_server_key(bytes(bad))
    bad = bytearray(blob)
    struct.pack_into("<Q", bad, start + 9, both.squashing.bodies.size // 2 - 1)      # one u128 word short
    with pytest.raises(keyio.KeyFormatError):
        keyio.loads_compressed_server_key(bytes(bad))
    with pytest.raises(keyio.KeyFormatError):                    # the packing key travels inside the squashing key
        keyio.dumps_compressed_server_key(keyio.CompressedServerKey(
            none.params, none.bsk_seed, none.bsk_bodies, none.ksk_seed, none.ksk_bodies,
            squashed_compression=both.squashed_compression))


def test_refusals_on_the_host():
    """lengths are 0 for parameters outside the device kernels; the host calls refuse nulls and non-binary keys"""
    sp = C.squash_params(3)
    L = S._lib()
    assert L.tfhe_hip_sns_seeded_bodies_len(ctypes.byref(sp)) == 3 * 3 * 3 * 2 * 2048
    bad = C.squash_params(3)
    bad.N = 1024
    assert L.tfhe_hip_sns_seeded_bodies_len(ctypes.byref(bad)) == 0
    pp = C.packing_params(16, 1, 64, 3)
    assert SC._lib().tfhe_hip_sns_pks_seeded_bodies_len(ctypes.byref(pp)) == 16 * 3 * 2 * 64
    badp = C.packing_params(16, 1, 48, 3)
    assert SC._lib().tfhe_hip_sns_pks_seeded_bodies_len(ctypes.byref(badp)) == 0
    seed = tfhe_amd._u64(S.seed_words(C.MASK_SEED))
    key = np.array([1, 0, 2], dtype=np.uint64)
    glwe = np.zeros(sp.k * sp.N, dtype=np.uint64)
    assert L.tfhe_hip_sns_seeded_keygen(ctypes.byref(sp), 1, seed, tfhe_amd._u64(key), tfhe_amd._u64(glwe), None) \
        == EINVAL
    assert L.tfhe_hip_sns_decompress_bsk(ctypes.byref(sp), seed, None, tfhe_amd._u64(glwe)) == EINVAL
    assert SC._lib().tfhe_hip_sns_pks_decompress_key(ctypes.byref(pp), None, tfhe_amd._u64(glwe), tfhe_amd._u64(glwe)) \
        == EINVAL
    with pytest.raises(ValueError):
        S.CompressedSquashedKey(sp, C.MASK_SEED, np.zeros(10, dtype=np.uint64))
    with pytest.raises(ValueError):
        SC.CompressedSquashedCompressionKey(pp, 1 << 128, np.zeros((16, 3, 64, 2), dtype=np.uint64))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_new_host_code_clean_under_asan_ubsan(tmp_path):
    """the 128-bit stream, both seeded keygens and both host decompressions at the smallest shapes, as a stand-alone
    program built with -fsanitize=address,undefined (tools/sanitize/sns_seeded_san.cpp; no Python, no preload)"""
    exe = str(tmp_path / "sns_seeded_san")
    csrc = os.path.join(ROOT, "tfhe_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tools", "sanitize", "sns_seeded_san.cpp"), os.path.join(csrc, "seeded.cpp"),
                    os.path.join(csrc, "client.cpp"), "-o", exe, "-pthread"], check=True, capture_output=True,
                   timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "SNS SEEDED SANITIZE OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
