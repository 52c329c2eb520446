"""Noise squashing on the MI355X (tfhe_amd/csrc/sns.hip, sns_api.cpp) off its preset: small LWE dimensions, where the
oracle restates whole batches, so every comparison is integer equality of ALL accumulator / output words.  Covered:
the chunked host loop around its chunk size, the MAC's walk of ciphertext groups over slots at its edges, n = 1..7
on the edges of the modulus switch, the message moduli and the LUT cache, synthetic keys on the edges of the load
rounding / limb split / 72-bit decomposition (tests/sns_inputs.py; certified on the CPU by tests/test_sns.py), the
device-buffer form with guard rows, the cross-stream ordering contract of tfhe_hip_sns_squash_async, and the errors."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import sns_inputs as I
import tfhe_amd
from conftest import KEY_SEED
from tfhe_amd import sns as S

pytestmark = pytest.mark.gpu

CHUNK = I.chunk_size()
SENTINEL = 0xA5A5A5A55A5A5A5A
EINVAL, ENOKEYS = -1, -4
_POOL = ThreadPoolExecutor(min(16, os.cpu_count() or 1))


def oracle_batch(O, osp, okeys, cts, mm=16):
    """(accumulators B x (k+1) x 2 x N, squashed LWEs B x (kN+1) x 2) of the oracle, one ciphertext per task."""
    lut = O.sns_lut_identity(osp, mm)
    assert okeys.bsk_limb.size  # built once, before the threads ask for it
    acc = np.stack(list(_POOL.map(lambda ct: O.sns_blind_rotate(osp, okeys, ct, lut), cts)))
    return acc, np.stack([O.sns_sample_extract(osp, a) for a in acc])


def same(got, want, what):
    if not np.array_equal(got, want):
        rows = np.nonzero((got != want).reshape(got.shape[0], -1).any(1))[0]
        pytest.fail(f"{what}: {rows.size} of {got.shape[0]} rows differ, first {rows[:8]}")


class Setup:
    """Keys of both sides at one n, a device context with the key resident, and the oracle's results by input."""

    def __init__(self, O, n):
        self.O, self.n = O, n
        self.sp, self.osp, self.key, self.okeys = I.small_keys(O, n, KEY_SEED + n)
        self.sq = S.Squasher(self.sp, 0).load_key(self.key)
        self._ref = {}

    def ref(self, tag, cts, mm=16):
        if (tag, mm) not in self._ref:
            r = oracle_batch(self.O, self.osp, self.okeys, cts, mm)
            for a in r:
                a.setflags(write=False)
            self._ref[tag, mm] = r
        return self._ref[tag, mm]


@pytest.fixture(scope="module")
def setups(oracle_mod):
    made = {}

    def get(n):
        if n not in made:
            made[n] = Setup(oracle_mod, n)
        return made[n]

    yield get
    for s in made.values():
        s.sq.close()


# ---- the chunk loop of run_device -------------------------------------------------------------------------------
def chunk_pool(s):
    """2c + 37 ciphertexts at n = 2; a batch of B is the LAST B rows, so that row q of one batch is never row q of
    another (a result left over from an earlier call cannot pass for this one's)."""
    cts = I.edge_inputs(2, 2 * CHUNK + 37, 0xC4A2)
    return cts, s.ref("chunks", cts)


@pytest.mark.parametrize("B", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 37], ids=["c-1", "c", "c+1", "2c+37"])
def test_chunks(setups, B):
    """One chunk short of full, exactly full, a second chunk of one ciphertext, and two full chunks plus a ragged
    third: the input, output and accumulator offsets of the later chunks and their reuse of the workspaces."""
    s = setups(2)
    cts, (acc, out) = chunk_pool(s)
    same(s.sq.squash(cts[-B:]), out[-B:], f"squash B={B}")
    if B == CHUNK + 1:
        same(s.sq.blind_rotate(cts[-B:]), acc[-B:], f"blind_rotate B={B}")


# ---- the group walk of sns_mac_kernel ---------------------------------------------------------------------------
def test_mac_groups_and_slots(setups, oracle_mod):
    """Groups of 32 over 8 slots: one ciphertext, one short of a group, a full group, a second group with one valid
    ciphertext (first store of a lane pair valid, second not), one short of 8 groups, exactly 8, and a ninth group
    that slot 0 walks; on ONE fresh context in an order that grows the workspaces and then reuses them for smaller
    batches.  Batches are suffixes of one pool (see chunk_pool)."""
    s = setups(3)
    cts = I.edge_inputs(3, 257, 0x3AC)
    acc, out = s.ref("mac", cts)
    sq = S.Squasher(s.sp, 0).load_key(s.key)
    try:
        for B in (33, 257, 1, 256, 31, 255, 32):
            same(sq.squash(cts[-B:]), out[-B:], f"squash B={B}")
            same(sq.blind_rotate(cts[-B:]), acc[-B:], f"blind_rotate B={B}")
    finally:
        sq.close()


# ---- LWE dimension ----------------------------------------------------------------------------------------------
def dim_inputs(n):
    return I.edge_inputs(n, 16, 0xED6E + n)


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_lwe_dimension(setups, n):
    s = setups(n)
    cts = dim_inputs(n)
    acc, out = s.ref("dim", cts)
    same(s.sq.blind_rotate(cts), acc, f"blind_rotate n={n}")
    same(s.sq.squash(cts), out, f"squash n={n}")


def test_valid_encryptions_decrypt(setups):
    """n = 7: encryptions of every message 0..15 under the 7-dimensional key (tfhe_hip_lwe_encrypt through
    ClientKey.encrypt) squash to the oracle's words and decrypt under the 128-bit GLWE key."""
    s = setups(7)
    prm = tfhe_amd.Params.preset(tfhe_amd.PRESET_GATE)
    prm.n = 7
    assert prm.order == 0 and prm.io_dim == 7
    ck = tfhe_amd.ClientKey(prm, None, s.key.lwe_key, None)
    msgs = np.arange(16, dtype=np.uint64)
    cts = ck.encrypt(msgs, 16, seed=0xC0FFEE77)
    assert np.array_equal(ck.decrypt(cts, 16), msgs)
    got = s.sq.squash(cts)
    same(got, s.ref("valid", cts)[1], "squash of valid encryptions")
    assert np.array_equal(s.key.decrypt(got), msgs)


# ---- message moduli and the LUT cache ---------------------------------------------------------------------------
def test_message_moduli_on_one_context(setups):
    """Every modulus against the oracle with that modulus, on one context, in an order that returns to earlier
    values (the LUT cache is keyed on the modulus and rewritten on a change).  Modulus 1 is valid on both sides: the
    client library and the oracle state the identity LUT with the same expression, all zero for one message."""
    s = setups(3)
    cts = dim_inputs(3)
    for mm in (16, 4, 16, 2048, 2, 16, 256, 1, 16):
        acc, out = s.ref("dim", cts, mm)
        same(s.sq.squash(cts, mm), out, f"squash msg_modulus={mm}")
        same(s.sq.blind_rotate(cts, mm), acc, f"blind_rotate msg_modulus={mm}")
    assert not s.ref("dim", cts, 1)[0].any()
    assert not np.array_equal(s.ref("dim", cts, 2)[1], s.ref("dim", cts, 4)[1])


def raw_squash(sq, cts, B, mm, out):
    return S._lib().tfhe_hip_sns_squash(sq._h, cts.ctypes.data_as(S._U64P), B, mm, out.ctypes.data_as(S._U64P))


@pytest.mark.parametrize("mm", [0, 3, 4096])
def test_invalid_modulus_writes_nothing(setups, mm):
    import torch
    s = setups(3)
    cts = dim_inputs(3)
    out = np.full((16, 4097, 2), SENTINEL, dtype=np.uint64)
    assert raw_squash(s.sq, cts, 16, mm, out) == EINVAL
    assert (out == np.uint64(SENTINEL)).all()
    acc = np.full((16, 3, 2, 2048), SENTINEL, dtype=np.uint64)
    assert S._lib().tfhe_hip_sns_blind_rotate(s.sq._h, cts.ctypes.data_as(S._U64P), 16, mm,
                                              acc.ctypes.data_as(S._U64P)) == EINVAL
    assert (acc == np.uint64(SENTINEL)).all()
    d_in, d_out = to_device(cts), device_out(16, 0)
    with pytest.raises(tfhe_amd.TfheError) as e:
        s.sq.squash_async(d_in, 16, d_out, mm)
    assert e.value.code == EINVAL
    torch.cuda.synchronize()
    assert (from_device(d_out) == np.uint64(SENTINEL)).all()
    same(s.sq.squash(cts), s.ref("dim", cts)[1], "squash after a refused call")


# ---- synthetic keys ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", I.KINDS)
def test_synthetic_keys(setups, oracle_mod, kind):
    """Key words on the edges (sns_inputs.synthetic_key) with edge_inputs and the inputs whose rounding ties
    tests/test_sns.py counts; then the real key loaded over the resident synthetic one."""
    s = setups(I.TIE_N)
    O = oracle_mod
    bsk = I.synthetic_key(s.sp, kind, I.TIE_SEED)
    okeys = I.load_synthetic(O.SnsKeys(s.osp, KEY_SEED, s.key.lwe_key), bsk)
    cts = np.concatenate([I.tie_inputs(), I.edge_inputs(I.TIE_N, 16, 0x5E7)])
    acc, out = oracle_batch(O, s.osp, okeys, cts)
    try:
        s.sq.load_key(I.KeyWords(bsk))
        same(s.sq.blind_rotate(cts), acc, f"blind_rotate, {kind} key")
        same(s.sq.squash(cts), out, f"squash, {kind} key")
    finally:
        s.sq.load_key(s.key)
    real = dim_inputs(I.TIE_N)
    same(s.sq.squash(real), s.ref("dim", real)[1], f"squash, real key loaded over the {kind} key")


# ---- device buffers ---------------------------------------------------------------------------------------------
def to_device(cts):
    import torch
    return torch.from_numpy(np.ascontiguousarray(cts).view(np.int64)).cuda()


def device_out(B, guard=2):
    import torch
    return torch.full((B + guard, 4097, 2), SENTINEL - (1 << 64), dtype=torch.int64, device="cuda")


def from_device(t):
    return t.cpu().numpy().view(np.uint64)


def test_async_form(setups):
    """B = c + 1 device ciphertexts (two chunks) on torch's current stream (stream=None: the legacy null stream), on
    a torch side stream and on the context's own stream (a NULL stream argument): each equals the host form and the
    oracle, and the two guard rows after the output keep their sentinel."""
    import torch
    s = setups(2)
    pool, (_, ref) = chunk_pool(s)
    B = CHUNK + 1
    cts, ref = pool[-B:], ref[-B:]
    same(s.sq.squash(cts), ref, "host form")
    d_in = to_device(cts)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for name, stream in (("current stream", None), ("side stream", side), ("context stream", "ctx")):
        d_out = device_out(B)
        torch.cuda.synchronize()
        if stream == "ctx":
            S._check(S._lib().tfhe_hip_sns_squash_async(s.sq._h, ctypes.c_void_p(d_in.data_ptr()), B, 16,
                                                        ctypes.c_void_p(d_out.data_ptr()), None))
        else:
            s.sq.squash_async(d_in, B, d_out, 16, stream)
        torch.cuda.synchronize()
        got = from_device(d_out)
        same(got[:B], ref, f"squash_async on the {name}")
        assert (got[B:] == np.uint64(SENTINEL)).all(), f"guard rows written ({name})"


def test_stream_ordering(setups):
    """The contract of tfhe_hip_sns_squash_async: calls on different streams are ordered on the context's
    workspaces.  An async squash of c + 1 ciphertexts on a side stream, then AT ONCE, without a synchronisation, a
    host squash of another batch; then the same with the second call async on a second side stream under another
    message modulus (the LUT is rewritten while the first call may still read it).  Every result equals the
    oracle's."""
    import torch
    s = setups(3)
    X = I.edge_inputs(3, CHUNK + 1, 0x0DE2)
    Y = I.edge_inputs(3, 64, 0x0DE3)
    ref_x = s.ref("order-x", X)[1]
    d_x, d_y = to_device(X), to_device(Y)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    same(s.sq.squash(Y[:1]), s.ref("order-y", Y)[1][:1], "warm-up")   # the LUT of modulus 16 is resident
    out_x = device_out(X.shape[0], 0)
    torch.cuda.synchronize()
    s.sq.squash_async(d_x, X.shape[0], out_x, 16, s1)
    got_y = s.sq.squash(Y)
    s1.synchronize()
    same(got_y, s.ref("order-y", Y)[1], "host squash issued behind an async call")
    same(from_device(out_x), ref_x, "async squash with a host call issued behind it")
    out_x, out_y = device_out(X.shape[0], 0), device_out(Y.shape[0], 0)
    torch.cuda.synchronize()
    s.sq.squash_async(d_x, X.shape[0], out_x, 16, s1)
    s.sq.squash_async(d_y, Y.shape[0], out_y, 4, s2)
    s1.synchronize()
    s2.synchronize()
    same(from_device(out_y), s.ref("order-y", Y, 4)[1], "async squash (modulus 4) issued behind an async call")
    same(from_device(out_x), ref_x, "async squash (modulus 16) with another modulus issued behind it")


# ---- errors -----------------------------------------------------------------------------------------------------
def test_errors(setups):
    s = setups(1)
    cts = dim_inputs(1)
    want = s.ref("dim", cts)[1]
    sq = S.Squasher(s.sp, 0)
    try:
        with pytest.raises(tfhe_amd.TfheError) as e:
            sq.squash(cts)
        assert e.value.code == ENOKEYS
        with pytest.raises(tfhe_amd.TfheError) as e:
            sq.blind_rotate(cts)
        assert e.value.code == ENOKEYS
        sq.load_key(s.key)
        same(sq.squash(cts), want, "squash")
        for bad in (s.key.bsk[:-1], np.concatenate([s.key.bsk, s.key.bsk[:1]])):
            with pytest.raises(tfhe_amd.TfheError) as e:
                sq.load_key(I.KeyWords(bad))
            assert e.value.code == EINVAL
            same(sq.squash(cts), want, "squash after a refused key")
        out = np.full((1, 4097, 2), SENTINEL, dtype=np.uint64)
        assert raw_squash(sq, cts, 0, 16, out) == 0
        assert (out == np.uint64(SENTINEL)).all()
        assert sq.squash(cts[:0]).shape == (0, 4097, 2)
    finally:
        sq.close()
