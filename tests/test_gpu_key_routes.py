"""Every key source of the engine against the host route, on one shard and on two (tfhe_amd/csrc/api.cpp: the key-load
pipeline behind tfhe_hip_load_keys*, tfhe_hip_load_bsk* and tfhe_hip_load_ms_key*).  The reference of a case is
decompress_server_key + load_keys (+ load_ms_key) on Engine(p, 0); every other route (device buffers, seeded bodies)
and every route on Engine(p, [0, 0]) must leave keys that compute the same words.  The shapes are those of
test_gpu_seeded_load.py: the code under test is plumbing whose branches depend on the source, the shard count and the
grouping factor, not on n."""
import numpy as np
import pytest

import tfhe_amd
from test_gpu_seeded_load import Case, P2, P3, P4, _s2

pytestmark = pytest.mark.gpu

ENOKEYS = -4
SHARDS = {"one": 0, "two": [0, 0]}
BCAST = {"one": "single", "two": "copy"}


class Ref:
    """a case and what the host route computes for it on one shard (computed once, never changed)"""

    def __init__(self, key, salt):
        preset, n, ms_count, g = key
        self.case = case = Case(preset, n, ms_count, g, salt=salt)
        with case.host_engine() as host:
            self.grouping = host.grouping
            self.pbs, self.ks = case.outputs(host)
            self.boot = host.bootstrap(case.small, case.lut)
        for a in (self.pbs, self.ks, self.boot):
            a.setflags(write=False)

    def check(self, eng, shards):
        case = self.case
        assert eng.grouping == self.grouping == case.g
        assert eng.key_bcast_mode == BCAST[shards]
        out, ks = case.outputs(eng)
        assert np.array_equal(out, self.pbs)
        assert np.array_equal(ks, self.ks)
        assert np.array_equal(eng.bootstrap(case.small, case.lut), self.boot)

    def check_rotation_only(self, eng, shards):
        case = self.case
        assert eng.grouping == case.g
        assert eng.key_bcast_mode == BCAST[shards]
        assert np.array_equal(eng.bootstrap(case.small, case.lut), self.boot)
        with pytest.raises(tfhe_amd.TfheError) as e:
            eng.pbs(case.cts, case.lut)
        assert e.value.code == ENOKEYS


KEYS = {"gate": (P2, 16, 0, 1), "fhevm_zeros": (P3, 16, 24, 1), "multibit_g2": (P4, 12, 0, 2)}


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Ref(KEYS[name], salt=40 + len(cache))
        return cache[name]

    return get


def _on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(torch.device("cuda", 0))


# ------------------------------------------------------------------ whole key sets
def _host(case, eng):
    case.host_load(eng)


def _device(case, eng):
    d_bsk, d_ksk = _on_device(case.sk.bsk), _on_device(case.sk.ksk)
    eng.load_keys_device(d_bsk, d_ksk)
    if case.sk.ms_zeros is not None:                     # the zeros have no device-buffer entry point
        eng.load_ms_key(case.sk.ms_zeros, **case.csk.ms)


def _seeded(case, eng):
    eng.load_compressed_keys(case.csk)


ROUTES = {"host": _host, "device": _device, "seeded": _seeded}
# every route that exists for a case: there is no multi-bit device entry point
EXISTING = [(name, route) for name, key in KEYS.items() for route in ROUTES if route != "device" or key[3] == 1]


@pytest.mark.parametrize("shards", list(SHARDS))
@pytest.mark.parametrize("name,route", EXISTING)
def test_key_routes_agree(refs, name, route, shards):
    ref = refs(name)
    with tfhe_amd.Engine(ref.case.p2, SHARDS[shards]) as eng:
        ROUTES[route](ref.case, eng)
        ref.check(eng, shards)


# ------------------------------------------------------------------ rotation-only engines
def _bsk_host(case, eng):
    if case.g == 1:
        eng.load_bsk(case.sk.bsk)
    else:
        b = tfhe_amd._c_u64(case.sk.bsk).ravel()
        tfhe_amd._check(tfhe_amd.lib().tfhe_hip_load_keys_mb(eng._h, case.g, tfhe_amd._u64(b), b.size, None, 0))


def _bsk_device(case, eng):
    d_bsk = _on_device(case.sk.bsk)
    tfhe_amd._check(tfhe_amd.lib().tfhe_hip_load_bsk_device(eng._h, tfhe_amd._dptr(d_bsk), d_bsk.numel()))


def _bsk_seeded(case, eng):
    if case.g == 1:
        eng.load_compressed_bsk(case.csk.bsk_seed, case.csk.bsk_bodies)
    else:
        bb = tfhe_amd._c_u64(case.csk.bsk_bodies).ravel()
        tfhe_amd._check(tfhe_amd.lib().tfhe_hip_load_keys_mb_seeded(eng._h, case.g, _s2(case.csk.bsk_seed),
                                                                    tfhe_amd._u64(bb), bb.size, None, None, 0))


BSK_ROUTES = {"host": _bsk_host, "device": _bsk_device, "seeded": _bsk_seeded}


@pytest.mark.parametrize("shards", list(SHARDS))
@pytest.mark.parametrize("name,route", EXISTING)
def test_rotation_only_routes_agree(refs, name, route, shards):
    ref = refs(name)
    with tfhe_amd.Engine(ref.case.p2, SHARDS[shards]) as eng:
        BSK_ROUTES[route](ref.case, eng)
        ref.check_rotation_only(eng, shards)


def test_bsk_only_load_drops_an_earlier_ksk(refs):
    """after a BSK-only load the resident KSK belongs to another key set: the engine is rotation-only again"""
    ref = refs("gate")
    with tfhe_amd.Engine(ref.case.p2, [0, 0]) as eng:
        _host(ref.case, eng)
        ref.check(eng, "two")
        _bsk_device(ref.case, eng)
        ref.check_rotation_only(eng, "two")
        _device(ref.case, eng)
        ref.check(eng, "two")


# ------------------------------------------------------------------ the zeros on two shards
def test_zeros_on_two_shards(refs):
    ref = refs("fhevm_zeros")
    case = ref.case
    with case.host_engine(zeros=False) as bare:
        assert not np.array_equal(bare.pbs(case.cts, case.lut), ref.pbs)      # the reduction is live
    with tfhe_amd.Engine(case.p2, [0, 0]) as eng:
        case.host_load(eng, zeros=False)
        bare2 = eng.pbs(case.cts, case.lut)
        assert not np.array_equal(bare2, ref.pbs)
        eng.load_ms_key(case.sk.ms_zeros, **case.csk.ms)                      # host rows
        assert np.array_equal(eng.pbs(case.cts, case.lut), ref.pbs)
        eng.load_ms_key(None)                                                 # count 0 disables it on every shard
        assert np.array_equal(eng.pbs(case.cts, case.lut), bare2)
        eng.load_compressed_keys(case.csk)                                    # seeded rows
        assert np.array_equal(eng.pbs(case.cts, case.lut), ref.pbs)
